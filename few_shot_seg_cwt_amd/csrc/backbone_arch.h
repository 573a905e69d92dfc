// The architecture of the PSPNet backbone, once: the ordered conv + BatchNorm pairs of the dilated
// ResNet-50/101 with the deep-base stem, the PPM 1x1 convs and the bottleneck conv, and which
// operand forms the extractor builds for each at load.  The extractor's loader and planner
// (api_extract.hip, extract_plan.h) and the pretraining model (pretrain.hip) all read this table.
// Host only: no HIP call, includable from a plain C++ file.
#pragma once
#include <string>
#include <vector>

namespace cwt {

constexpr int kBlocks50[4] = {3, 4, 6, 3};
constexpr int kBlocks101[4] = {3, 4, 23, 3};

enum ConvRole : int {
  ROLE_STEM,  // layer0 conv bi (0..2)
  ROLE_C1,    // bottleneck block li.bi: conv1 / conv2 / conv3 / downsample conv
  ROLE_C2,
  ROLE_C3,
  ROLE_DOWN,
  ROLE_PPM,   // PPM bin bi's 1x1 conv
  ROLE_BOTT,  // the 3x3 bottleneck conv over [layer4 | PPM] = 4096 channels
};

struct ConvSpec {
  ConvRole role;
  int li, bi;  // layer (0..3, blocks only) and index within the role
  std::string wname, bnp;  // weight tensor, BatchNorm prefix (the reference's state_dict names)
  int Ci, Co, k, stride, pad, dil;
};

inline bool is_block_role(ConvRole r) { return r == ROLE_C1 || r == ROLE_C2 || r == ROLE_C3 || r == ROLE_DOWN; }

// In the reference's state_dict order.  layers: 50 or 101 (anything else: empty).
inline std::vector<ConvSpec> backbone_arch(int layers) {
  std::vector<ConvSpec> a;
  if (layers != 50 && layers != 101) return a;
  // layer0: deep-base stem (resnet.py:110-118)
  a.push_back({ROLE_STEM, -1, 0, "layer0.0.weight", "layer0.1", 3, 64, 3, 2, 1, 1});
  a.push_back({ROLE_STEM, -1, 1, "layer0.3.weight", "layer0.4", 64, 64, 3, 1, 1, 1});
  a.push_back({ROLE_STEM, -1, 2, "layer0.6.weight", "layer0.7", 64, 128, 3, 1, 1, 1});
  const int* nb = layers == 50 ? kBlocks50 : kBlocks101;
  const int planes_of[4] = {64, 128, 256, 512};
  int inplanes = 128;
  for (int li = 0; li < 4; ++li) {
    const int planes = planes_of[li];
    for (int bi = 0; bi < nb[li]; ++bi) {
      // dilation surgery (pspnet.py:103-112): layer3 conv2 d2 s1, layer4 conv2 d4 s1, downsample s1
      int s2 = 1, d2 = 1, sd = 1;
      if (li == 1 && bi == 0) s2 = sd = 2;
      if (li == 2) d2 = 2;
      if (li == 3) d2 = 4;
      const std::string p = "layer" + std::to_string(li + 1) + "." + std::to_string(bi);
      a.push_back({ROLE_C1, li, bi, p + ".conv1.weight", p + ".bn1", inplanes, planes, 1, 1, 0, 1});
      a.push_back({ROLE_C2, li, bi, p + ".conv2.weight", p + ".bn2", planes, planes, 3, s2, d2, d2});
      a.push_back({ROLE_C3, li, bi, p + ".conv3.weight", p + ".bn3", planes, planes * 4, 1, 1, 0, 1});
      if (bi == 0)
        a.push_back(
            {ROLE_DOWN, li, bi, p + ".downsample.0.weight", p + ".downsample.1", inplanes, planes * 4, 1, sd, 0, 1});
      inplanes = planes * 4;
    }
  }
  for (int i = 0; i < 4; ++i) {
    const std::string p = "ppm.features." + std::to_string(i);
    a.push_back({ROLE_PPM, -1, i, p + ".1.weight", p + ".2", 2048, 512, 1, 1, 0, 1});
  }
  a.push_back({ROLE_BOTT, -1, 0, "bottleneck.0.weight", "bottleneck.1", 4096, 512, 3, 1, 1, 1});
  return a;
}

// The operand forms the extractor's loader builds for a conv of Ci input channels beside its packed
// fp32 weights and their bf16x3 split (the stem's conv1 has neither form: its own kernel)
struct ConvForms {
  bool w_l = false;    // x6: the third term of the split, [Co][K/32][32]
  bool wino2 = false;  // x6 Winograd F(2x2,3x3): transformed weights.  Stride-1 3x3 layers with Ci >= 256 (at
                       // Ci = 128 the 16 thin GEMMs and the transforms measured slower than the direct conv:
                       // 35.9 vs 29.1 us, profiles/r5/sweeps)
  bool wino4 = false;  // F(4x4,3x3), only on request at load (CWT_WINO=4): faster in the pipeline but ~20x the
                       // rounding error of F(2x2) / the fp32 conv (DESIGN.md §3 "Measured and not kept")
  bool w_b = false;    // plain bf16 operand of the bf16 conv stack, K in packed_k64 order
};

inline ConvForms conv_forms_built(int Ci, int k, int stride, bool wino4_requested) {
  ConvForms f;
  f.w_l = (k * k * Ci) % 32 == 0;
  const bool wino = k == 3 && stride == 1 && Ci % 32 == 0;
  f.wino2 = wino && Ci >= 256;
  f.wino4 = wino && Ci >= 128 && wino4_requested;
  f.w_b = Ci % 64 == 0;
  return f;
}

}  // namespace cwt
