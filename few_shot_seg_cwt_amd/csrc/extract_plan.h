// The host-side plan of one pass of the frozen extractor (api_extract.hip run_extract): the conv
// family the pass runs in, the ordered steps with each conv's geometry, tile plan, Winograd tile and
// split-K hand-over, every step's profile record, and the workspace sizes.  One value, computed once
// per API call by extract_plan() from the architecture (backbone_arch.h), the operand forms built at
// load, the batch, the mode and the environment's knobs; run_extract executes it and
// cwt_debug_extract_plan prints it.  Host only: no HIP runtime call (the pure planners it calls --
// plan_conv*, wino_geom, bn_train_part_floats -- are declared in kernels.h).
#pragma once
#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/cwt.h"
#include "backbone_arch.h"
#include "kernels.h"

namespace cwt {

constexpr int kBins[4] = {1, 2, 3, 6};

inline int down2(int x) { return (x - 1) / 2 + 1; }  // 3x3 s2 p1 conv / maxpool output size

inline int conv_out_size(int in, int k, int stride, int pad, int dil) {
  return (in + 2 * pad - dil * (k - 1) - 1) / stride + 1;
}

// The input channels the extractor's conv of a spec reads: all of them, except that its bottleneck conv
// runs over the layer4 half (the first 2048 of 4096) alone -- the PPM half enters as the folded field FB
inline int extractor_ci(const ConvSpec& s) { return s.role == ROLE_BOTT ? 2048 : s.Ci; }

// Per spec, the operand forms the extractor's loader builds (the stem's conv1 none: its own kernel)
inline std::vector<ConvForms> extractor_forms(const std::vector<ConvSpec>& arch, bool wino4_requested) {
  std::vector<ConvForms> f;
  for (const ConvSpec& s : arch)
    f.push_back(s.role == ROLE_STEM && s.bi == 0 ? ConvForms{}
                                                 : conv_forms_built(extractor_ci(s), s.k, s.stride, wino4_requested));
  return f;
}

// ---- the conv family of a pass ----
enum ExtractMode : int {
  EM_F32 = 0,  // exact fp32, register-staged (conv_igemm_f32): CWT_CONV_F32D=0, and every training-mode BN pass
  EM_F32D,     // exact fp32 on the LDS-DMA conv body (conv_igemm_f32d: fp32 NHWC activations, f32 MFMA)
  EM_X6,       // fp32 width on the bf16 matrix cores (conv_igemm_x6): f32d's operands, split in registers
  EM_X3S,      // bf16x3 over S-layout activations
  EM_B16,      // plain bf16 (cwt_backbone_set_precision)
};
constexpr int EM_NMODES = 5;

struct ExtractModeTraits {
  const char* kernel;  // the conv kernel's name in the profile records
  int layout;          // activation storage between the convs (ActLayout)
  int prec;            // launch_conv_x3s / plan_conv_s family: 0, 1, 3 or 6
  bool dma;            // runs on the LDS-DMA body (conv_x3s.hip kernels)
  bool out_f32;        // every conv writes fp32 NHWC (else only the bottleneck conv does)
  double elem_bytes;   // accounting: 4 B per element (fp32 or the bf16x3 S-layout), 2 B for the bf16 stack
};
constexpr ExtractModeTraits extract_mode_traits(int mode) {
  switch (mode) {
    case EM_F32D: return {"conv_igemm_f32d", ACT_F32, 0, true, true, 4.0};
    case EM_X6: return {"conv_igemm_x6", ACT_F32, 6, true, true, 4.0};
    case EM_X3S: return {"conv_igemm_x3s", ACT_SPLIT, 3, true, false, 4.0};
    case EM_B16: return {"conv_igemm_b16", ACT_BF16, 1, true, false, 2.0};
    default: return {"conv_igemm_f32", ACT_F32, 0, false, true, 4.0};
  }
}

// The environment's say in the plan.  Read once per API call and never cached.
struct ExtractKnobs {
  bool f32d = true;         // CWT_CONV_F32D=0: the exact-fp32 path on the register-staged conv_igemm_f32
  // CWT_WINO: 0 every conv direct, 2 / 4 every Winograd-eligible conv in F(2x2) / F(4x4), else (-1) the default
  // tile.  F(4x4) needs its weights, which the loader builds only if the value began with '4' at load
  int wino = -1;
  bool wino4_at_load = false;
  // x6 (eval mode) only.  CWT_FUSE_DOWN=0 restores the downsample conv as a launch of its own (through D),
  // CWT_FUSE_SPLITK_WINO=0 the split-K epilogue launch in front of a Winograd conv
  bool fuse_down = true;
  bool fuse_splitk_wino = true;
  bool ppm_splitk = false;  // CWT_PPM_SPLITK (set): the split-K form of the two PPM GEMMs at any cell count
};

inline ExtractKnobs extract_knobs_from_env() {
  ExtractKnobs kn;
  const auto off = [](const char* name) {
    const char* v = getenv(name);
    return v && v[0] == '0';
  };
  kn.f32d = !off("CWT_CONV_F32D");
  const char* w = getenv("CWT_WINO");
  kn.wino = w && w[0] ? atoi(w) : -1;
  kn.wino4_at_load = w && w[0] == '4';
  kn.fuse_down = !off("CWT_FUSE_DOWN");
  kn.fuse_splitk_wino = !off("CWT_FUSE_SPLITK_WINO");
  kn.ppm_splitk = getenv("CWT_PPM_SPLITK") != nullptr;
  return kn;
}

// conv arithmetic / activation storage: plain bf16 (cwt_backbone_set_precision), else the context's
// fp32-accurate mode.
// The training-mode BN pass (once per epoch) amplifies conv rounding ~100x through its batch
// statistics: it runs the exact-fp32 conv path in either precision (a bf16 backbone
// too: the CPU emulation of its roundings, tests/bf16_ref.py, is 0.6 off the exact features at R50
// S = 65)
inline ExtractMode extract_mode(int precision, int conv_arith, bool train_bn, const ExtractKnobs& kn) {
  if (train_bn) return EM_F32;
  if (precision == CWT_CONV_BF16) return EM_B16;
  if (conv_arith == CWT_CONV_ARITH_BF16X3) return EM_X3S;
  if (conv_arith == CWT_CONV_ARITH_BF16X6) return EM_X6;
  return kn.f32d ? EM_F32D : EM_F32;
}

// ---- steps ----
struct ExtractRec {  // a profile record: Prof's arguments (level 0: the step has none)
  int level = 0;
  std::string name;
  double flops = 0.0, bytes = 0.0;
};

// One Winograd conv F(m x m, 3x3): its geometry, the batched GEMMs' plan and kernel stage tag, and the
// sub-records (the executed work of the form): the transforms' algorithmic bytes
// and the batched GEMMs' executed FLOPs, at profile level 3 only (their event pairs would add ~10 us
// of gaps to each Winograd conv's own bracket at levels 1 and 2)
struct WinoPlan {
  WinoGeom g;
  ConvPlan gemm;
  int gemm_stage = 7;
  ExtractRec in, mm, out;
};

// nsplit_in > 0: the input arrives as that many split-K partial planes, summed by the input transform
inline WinoPlan wino_plan(int N, int H, int W, int Ci, int Co, int d, int m, int stage, int nsplit_in, bool has_res,
                          bool names = true) {
  WinoPlan wp;
  const WinoGeom g = wp.g = wino_geom(N, H, W, d, m);
  wp.gemm = plan_conv_s(6, (int)g.T, Co, Ci, g.P);
  // the batched GEMMs are the stage-7 (F(2x2)) / stage-8 (F(4x4)) instantiations, the bottleneck's
  // (stage 6) its own: their own rocprofv3 statistics
  wp.gemm_stage = m == 4 ? 8 : stage == 6 ? 6 : 7;
  const double vb = 4.0 * g.P * g.T * Ci, mb = 4.0 * g.P * g.T * Co;
  wp.in.level = wp.mm.level = wp.out.level = 3;
  wp.in.bytes = 4.0 * N * H * W * Ci * (nsplit_in > 0 ? nsplit_in : 1) + vb;
  wp.mm.flops = 2.0 * g.P * g.T * Ci * Co;
  wp.mm.bytes = vb + 6.0 * g.P * Co * Ci + mb;
  const double ob = 4.0 * N * H * W * Co * (has_res ? 2.0 : 1.0);
  wp.out.bytes = mb + ob;
  if (names) {
    wp.in.name = "wino_in " + std::to_string(Ci) + "@" + std::to_string(H);
    wp.mm.name = "wino_gemm " + std::to_string(Ci) + "x" + std::to_string(Co) + "@" + std::to_string(H);
    wp.out.name = "wino_out " + std::to_string(Co) + "@" + std::to_string(H);
  }
  return wp;
}

enum ExtractBuf : int {  // the pass's buffers, resolved to pointers by the executor
  XB_NONE = 0, XB_IMG, XB_A, XB_B, XB_T1, XB_T2, XB_D, XB_COL, XB_POOL, XB_PPM, XB_Q, XB_R, XB_FB, XB_PARTS,
  XB_PART, XB_FEAT, XB_COUNT
};

enum ExtractStepKind : int {
  XS_STEM1,        // the stem's conv1 (its own kernel)
  XS_CONV_DIRECT,  // a conv on the register-staged fp32 kernel
  XS_CONV_DMA,     // ... on the LDS-DMA body, in the mode's family
  XS_CONV_DUAL,    // x6: a block's conv3 + downsample conv as one two-source GEMM (fold_down)
  XS_CONV_WINO,    // x6: a stride-1 3x3 conv in the Winograd form
  XS_BN_TRAIN,     // training-mode BN of the raw conv output before it (residual and ReLU after it)
  XS_MAXPOOL,
  XS_MID_COPY,     // fp32 NHWC copy of a block's output into the caller's buffer mid_slot (cwt_extract_features_mid / _blocks)
  XS_PPM_POOL,
  XS_PPM_CONV,     // PPM 1x1 conv + BN + ReLU over the pooled cells (pspnet.py:27-29)
  XS_PPM_FOLD,     // per-tap products of the bottleneck's PPM channels with the cells
  XS_PPM_FIELD,    // separable interpolation of the per-tap products: the PPM half of the bottleneck conv
  XS_REFOLD_PPM,   // after a training-mode BN pass: the bottleneck's new eval BN scale into the PPM-branch weights
  XS_REFOLD_DOWN,  // ... and the new conv3 / downsample eval folds into the fused rows
};

struct ExtractStep {
  ExtractStepKind kind;
  ExtractRec rec;
  int spec = -1;   // index into the architecture: the conv (a dual conv's conv3; a BN step's layer)
  int stage = 0;   // kernel symbol tag: 0 stem, 1-4 layer1-4, 6 bottleneck
  // conv geometry: x [N][Hi][Wi][Ci] -> y [N][Ho][Wo][Co], M = N Ho Wo rows, K = k k Ci (+ Ci2)
  int N = 0, Hi = 0, Wi = 0, Ci = 0, Co = 0, k = 1, stride = 1, pad = 0, dil = 1, Ho = 0, Wo = 0, M = 0, K = 0;
  ExtractBuf x = XB_NONE, y = XB_NONE, res = XB_NONE;
  int x_ld = 0, y_ld = 0, y_off = 0, res_ld = 0, relu = 0;
  bool out_f32 = false;  // this conv writes fp32 (and takes an fp32 residual) in every mode: the bottleneck
  // training-mode BN: the conv / PPM GEMM runs raw (scale 1, shift 0, no ReLU; the bottleneck alone keeps its
  // residual, the raw PPM half of the same conv), its XS_BN_TRAIN step follows
  bool raw = false;
  ConvPlan plan;         // the direct conv's tile plan (a Winograd conv's: see wino)
  // the second source of a dual conv: Ci2 more input channels from x2 [N][Hi2][Wi2][Ci2] at stride2
  ExtractBuf x2 = XB_NONE;
  int Hi2 = 0, Wi2 = 0, Ci2 = 0, stride2 = 0;
  int wino_m = 0;        // Winograd output tile, decided once (0: not a Winograd conv)
  WinoPlan wino;
  // part_out: a split-K conv that leaves its partials unreduced in PART for the next step's input transform;
  // part_in: that next step (a Winograd conv), in_nsplit / in_spec / in_relu its producer's
  bool part_out = false, part_in = false;
  int in_nsplit = 0, in_spec = -1, in_relu = 0;
  // XS_BN_TRAIN: y (+ y_elems floats) fp32, M rows of Co channels at stride y_ld; res / res_ld / relu above
  long y_elems = 0, rows_per_image = 0;
  bool dropout = false;  // the bottleneck's Dropout2d
  bool few_cells = false;  // XS_PPM_CONV / XS_PPM_FOLD: the few-row form (launch_ppm_gemm)
  int mid_slot = -1;       // XS_MID_COPY: the block's bit of the request mask (extract_block_bit)
};

struct ExtractSizes {  // floats
  long A = 0, T1 = 0, T2 = 0, D = 0, COL = 0, POOL = 0, PPM = 0, Q = 0, R = 0, F = 0, PARTS = 0;
  size_t PART = 0, bn_part = 0, wino_V = 0, wino_M = 0;
};

constexpr int kKcPpm = 32, kKcQ = 64;  // K chunk of the two small-M GEMMs

struct ExtractPlan {
  const char* error = nullptr;  // the pass cannot run (CWT_ESTATE)
  ExtractMode mode = EM_X6;
  ExtractModeTraits traits = extract_mode_traits(EM_X6);
  int N = 0, S = 0, Hs = 0, H1 = 0, h = 0;
  ExtractRec whole;             // the whole-pass record: brackets steps [0, pass_steps)
  std::vector<ExtractStep> steps;
  size_t pass_steps = 0;
  ExtractSizes ws;
};

// ---- the planner, in four parts: buffer sizes, the conv list, the convs' forms, their records ----

// The buffers whose sizes follow from the batch and the image alone
inline ExtractSizes extract_buffer_sizes(int N, int Hs, int H1, int h) {
  ExtractSizes z;
  z.A = std::max({(long)N * Hs * Hs * 128, (long)N * H1 * H1 * 256, (long)N * h * h * 2048});
  z.T1 = std::max((long)N * H1 * H1 * 128, (long)N * h * h * 512);
  z.T2 = std::max((long)N * H1 * H1 * 64, (long)N * h * h * 512);
  z.D = std::max((long)N * H1 * H1 * 256, (long)N * h * h * 2048);
  z.COL = (long)N * h * 16 * 2048 + (long)N * 16 * 16 * 2048;  // PPM row-segment + block sums
  z.POOL = (long)N * 50 * 2048;
  z.PPM = (long)N * 50 * 512;
  z.Q = (long)N * 50 * 4608;
  z.R = (long)N * 12 * h * 3 * 512;
  z.F = (long)N * h * h * 512;
  z.PARTS = std::max((long)(2048 / kKcPpm) * N * 50 * 512, (long)(512 / kKcQ) * N * 50 * 4608);
  return z;
}

// The pass's convs in order: stem conv2 / conv3 (conv1 and the max pool are kernels of their own), the
// blocks, the bottleneck -- geometry and buffers, no tile plan or record yet
struct ExtractConvs {
  std::vector<ExtractStep> convs;
  size_t n_stem = 0, n_backbone = 0;         // convs [0, n_stem) the stem's, [n_stem, n_backbone) the blocks'
  std::vector<long> block_end;               // per block of layers 2-4, in order: the conv index of its last conv
  ExtractBuf L4 = XB_NONE;                   // layer4 output [N][h][h][2048]
  int ppm0 = 0, bott = 0;                    // specs of the first PPM conv and of the bottleneck conv
};

inline ExtractConvs extract_conv_list(const std::vector<ConvSpec>& arch, int N, int Hs, int H1, int h, bool dma,
                                      bool fuse_down) {
  ExtractConvs L;
  std::vector<ExtractStep>& convs = L.convs;
  auto cc = [&](int spec, int stage, int Ci, ExtractBuf x, int H, ExtractBuf y, ExtractBuf res, int res_ld, int relu) {
    const ConvSpec& s = arch[spec];
    ExtractStep c;
    c.kind = dma ? XS_CONV_DMA : XS_CONV_DIRECT;
    c.spec = spec, c.stage = stage;
    c.N = N, c.Hi = c.Wi = H, c.Ci = Ci, c.Co = s.Co, c.k = s.k, c.stride = s.stride, c.pad = s.pad, c.dil = s.dil;
    c.Ho = c.Wo = conv_out_size(H, s.k, s.stride, s.pad, s.dil);
    c.M = N * c.Ho * c.Wo;
    c.K = s.k * s.k * Ci;
    c.x = x, c.x_ld = Ci, c.y = y, c.y_ld = s.Co, c.y_off = 0, c.res = res, c.res_ld = res_ld, c.relu = relu;
    c.out_f32 = stage == 6;
    convs.push_back(c);
  };
  cc(1, 0, arch[1].Ci, XB_A, Hs, XB_B, XB_NONE, 0, 1);
  cc(2, 0, arch[2].Ci, XB_B, Hs, XB_A, XB_NONE, 0, 1);
  L.n_stem = convs.size();
  ExtractBuf cur = XB_B, other = XB_A;  // cur: the max pool's output
  int H = H1;
  size_t ai = 3;
  while (ai < arch.size() && is_block_role(arch[ai].role)) {
    const int c1 = (int)ai, c2 = c1 + 1, c3 = c1 + 2;
    const bool has_down = ai + 3 < arch.size() && arch[ai + 3].role == ROLE_DOWN;
    const int down = has_down ? c1 + 3 : -1, li = arch[c1].li, stage = li + 1, Cin = arch[c1].Ci;
    ai += has_down ? 4 : 3;
    const int Ho = arch[c2].stride == 2 ? down2(H) : H;
    cc(c1, stage, Cin, cur, H, XB_T1, XB_NONE, 0, 1);
    cc(c2, stage, arch[c2].Ci, XB_T1, H, XB_T2, XB_NONE, 0, 1);
    if (has_down && fuse_down) {  // conv3 + downsample conv as one two-source GEMM (fold_down)
      cc(c3, stage, arch[c3].Ci, XB_T2, Ho, other, XB_NONE, 0, 1);
      ExtractStep& c = convs.back();
      c.kind = XS_CONV_DUAL;
      c.x2 = cur, c.Hi2 = c.Wi2 = H, c.Ci2 = Cin, c.stride2 = arch[down].stride;
      c.K += Cin;
    } else {
      ExtractBuf res = cur;
      int res_ld = Cin;
      if (has_down) {
        cc(down, stage, Cin, cur, H, XB_D, XB_NONE, 0, 0);
        res = XB_D, res_ld = arch[down].Co;
      }
      cc(c3, stage, arch[c3].Ci, XB_T2, Ho, other, res, res_ld, 1);
    }
    if (li >= 1) L.block_end.push_back((long)convs.size() - 1);
    std::swap(cur, other);
    H = Ho;
  }
  L.n_backbone = convs.size();
  L.L4 = cur;
  L.ppm0 = (int)ai, L.bott = L.ppm0 + 4;
  // the bottleneck conv over the layer4 channels; the folded PPM field FB enters as residual
  cc(L.bott, 6, extractor_ci(arch[L.bott]), L.L4, h, XB_FEAT, XB_FB, 512, 1);
  return L;
}

// Each conv's tile plan, Winograd tile and split-K hand-over; returns the split-K scratch PART in floats
inline size_t plan_conv_forms(ExtractConvs& L, const std::vector<ConvForms>& forms, ExtractMode mode,
                              const ExtractKnobs& kn) {
  const ExtractModeTraits tr = extract_mode_traits(mode);
  const bool x6 = mode == EM_X6;
  size_t part = 0;
  for (ExtractStep& c : L.convs) {
    c.plan = c.kind == XS_CONV_DUAL ? plan_conv_dual(c.M, c.Co, c.K)
             : tr.dma               ? plan_conv_s(tr.prec, c.M, c.Co, c.K)
                                    : plan_conv(c.M, c.Co, c.K);
    if (c.plan.nsplit > 1) part = std::max(part, (size_t)c.plan.nsplit * c.M * c.Co);
  }
  // The Winograd form (x6): stride-1 3x3 layers whose transformed weights were built at load, on images
  // of a pixel stride equal to their channels.  The default tile: F(2x2,3x3) for Ci >= 256 (at Ci = 128
  // the direct conv measured faster).  F(4x4,3x3) only on request (CWT_WINO=4): its rounding error is
  // ~20x F(2x2)'s (4e-6 .. 1.2e-5 of max |y| per conv against 2-6e-7; the fp32 GEMM's accumulation
  // error, amplified by the transforms), for +8 % pipelined throughput (profiles/r5/wino4/)
  for (ExtractStep& c : L.convs) {
    const ConvForms& f = forms[c.spec];
    const bool eligible = c.kind == XS_CONV_DMA && (f.wino2 || f.wino4) && c.k == 3 && c.stride == 1 &&
                          c.pad == c.dil && c.x_ld == c.Ci;
    int wm = x6 && kn.wino != 0 && eligible ? (kn.wino == 2 || kn.wino == 4 ? kn.wino : c.Ci >= 256 ? 2 : 0) : 0;
    if (wm && !(wm == 4 ? f.wino4 : f.wino2)) wm = 0;  // form not built for this layer
    c.wino_m = wm;
    if (wm) c.kind = XS_CONV_WINO;
  }
  // conv i leaves its split-K partials unreduced for conv i + 1's input transform: a split-K conv
  // into T1 (a block's conv1: read by its conv2 alone, never a mid feature) in front of a Winograd conv
  for (size_t i = 0; x6 && kn.fuse_splitk_wino && i + 1 < L.n_backbone; ++i) {
    ExtractStep &c = L.convs[i], &nx = L.convs[i + 1];
    if (c.plan.nsplit > 1 && c.y == XB_T1 && c.res == XB_NONE && c.y_off == 0 && c.y_ld == c.Co && nx.x == XB_T1 &&
        !c.wino_m && nx.wino_m) {
      c.part_out = nx.part_in = true;
      nx.in_nsplit = c.plan.nsplit, nx.in_spec = c.spec, nx.in_relu = c.relu;
    }
  }
  return part;
}

// A planned conv's record, and a Winograd conv's plan with its sub-records.  Algorithmic bytes: every
// operand once, the mode's element size (the bf16 stack's fp32 bottleneck output: 4 B).  The Winograd
// form's record names its batched GEMM's plan; its FLOPs stay the direct conv's (algorithmic: the roofline
// prices the conv, not the form that computes it).  train_bn: the conv runs raw, only the bottleneck's
// residual stays with it
inline void plan_conv_record(ExtractStep& c, const ExtractModeTraits& tr, bool train_bn, bool names) {
  if (c.wino_m)
    c.wino = wino_plan(c.N, c.Hi, c.Wi, c.Ci, c.Co, c.dil, c.wino_m, c.stage, c.in_nsplit, c.res != XB_NONE, names);
  const bool conv_res = c.res != XB_NONE && (!train_bn || c.stage == 6);
  const double eb = tr.elem_bytes, ob = c.out_f32 ? 4.0 : eb;
  c.rec.level = c.stage == 6 ? 1 : 2;
  c.rec.flops = 2.0 * c.M * c.Co * c.K;
  c.rec.bytes = eb * ((double)c.N * c.Hi * c.Wi * c.Ci + (double)c.N * c.Hi2 * c.Wi2 * c.Ci2 + (double)c.Co * c.K) +
                ob * ((double)c.M * c.Co + (conv_res ? (double)c.M * c.Co : 0.0));
  if (!names) return;
  const ConvPlan& pl = c.wino_m ? c.wino.gemm : c.plan;
  c.rec.name = std::string(tr.kernel) + (c.wino_m == 4 ? "w4<" : c.wino_m ? "w<" : "<") + std::to_string(pl.bm) + "," +
               std::to_string(pl.bn) + "," + std::to_string(c.stage) + ">" +
               (pl.nsplit > 1 ? "+splitk" + std::to_string(pl.nsplit) : std::string()) + " " + std::to_string(c.Ci) +
               (c.x2 != XB_NONE ? "+" + std::to_string(c.Ci2) : std::string()) + "x" + std::to_string(c.Co) + "k" +
               std::to_string(c.k) + "s" + std::to_string(c.stride) + "d" + std::to_string(c.dil) + "@" +
               std::to_string(c.Ho);
}

// The per-block request of mid features: one bit per bottleneck of layers 2-4 in network order (13 bits for
// 50 layers, 30 for 101).  The bit of block bi of layer li (1 .. 3), or -1 if the architecture has no such block
inline int extract_block_bit(const std::vector<ConvSpec>& arch, int li, int bi) {
  int bit = 0;
  for (const ConvSpec& s : arch) {
    if (s.role != ROLE_C1 || s.li < 1) continue;
    if (s.li == li && s.bi == bi) return bit;
    ++bit;
  }
  return -1;
}
// The request of cwt_extract_features_mid: the last block of every layer (2 + i) whose bit i of want_mid is set
inline uint64_t extract_last_blocks(const std::vector<ConvSpec>& arch, int want_mid) {
  uint64_t m = 0;
  int bit = 0, last[4] = {-1, -1, -1, -1};
  for (const ConvSpec& s : arch)
    if (s.role == ROLE_C1 && s.li >= 1) last[s.li] = bit++;
  for (int li = 1; li < 4; ++li)
    if (((want_mid >> (li - 1)) & 1) && last[li] >= 0) m |= uint64_t(1) << last[li];
  return m;
}

// arch / forms: backbone_arch(layers) and, per spec, the forms its loader built.  want_blocks: bit set = a copy
// of that block's output (extract_block_bit); 0: none, the plan of cwt_extract_features.  names: build the records' name strings (off when the profiler is: no record is
// taken then).
inline ExtractPlan extract_plan(const std::vector<ConvSpec>& arch, const std::vector<ConvForms>& forms, int N, int S,
                                ExtractMode mode, const ExtractKnobs& kn, uint64_t want_blocks, bool train_bn,
                                bool names = true) {
  ExtractPlan P;
  P.mode = mode;
  const ExtractModeTraits tr = P.traits = extract_mode_traits(mode);
  const int Hs = down2(S), H1 = down2(Hs), h = down2(H1);
  P.N = N, P.S = S, P.Hs = Hs, P.H1 = H1, P.h = h;
  ExtractSizes& z = P.ws = extract_buffer_sizes(N, Hs, H1, h);
  ExtractConvs L = extract_conv_list(arch, N, Hs, H1, h, tr.dma, mode == EM_X6 && kn.fuse_down);
  std::vector<ExtractStep>& convs = L.convs;
  z.PART = plan_conv_forms(L, forms, mode, kn);
  if (train_bn) z.bn_part = bn_train_part_floats((long)N * Hs * Hs, 64);
  // ---- records and the sizes that follow from the convs ----
  const long cells = (long)N * 50;
  const double ppm_flops = 2.0 * cells * 512 * 2048 + 2.0 * cells * 4608 * 512 +
                           2.0 * N * 12 * h * 3 * 512 * 3 * 6 + 2.0 * N * h * h * 512 * 36;
  P.whole.level = 1;
  P.whole.flops = 2.0 * N * Hs * Hs * 64 * 27 + ppm_flops;
  if (names) P.whole.name = "extract_features N=" + std::to_string(N) + " S=" + std::to_string(S);
  for (ExtractStep& c : convs) {
    if (mode == EM_B16 && !forms[c.spec].w_b) P.error = "bf16 conv weights missing (Ci % 64 != 0)";
    P.whole.flops += 2.0 * c.M * c.Co * c.K;
    P.whole.bytes += 4.0 * ((double)c.N * c.Hi * c.Wi * c.Ci + (double)c.Co * c.K + (double)c.M * c.Co);
    plan_conv_record(c, tr, train_bn, names);
    if (train_bn) z.bn_part = std::max(z.bn_part, bn_train_part_floats(c.M, c.Co));
    if (c.wino_m) {
      z.wino_V = std::max(z.wino_V, (size_t)c.wino.g.P * c.wino.g.T * c.Ci);
      z.wino_M = std::max(z.wino_M, (size_t)c.wino.g.P * c.wino.g.T * c.Co);
    }
  }

  // ---- the ordered steps ----
  std::vector<ExtractStep>& st = P.steps;
  st.reserve(2 * convs.size() + 16);
  auto add = [&](ExtractStepKind kind, int level, const char* name, double flops, double bytes) -> ExtractStep& {
    ExtractStep s;
    s.kind = kind;
    s.rec.level = level;
    if (names && name) s.rec.name = name;
    s.rec.flops = flops, s.rec.bytes = bytes;
    st.push_back(s);
    return st.back();
  };
  // the training-mode BN of a raw output y (fp32: such a pass runs in EM_F32)
  auto add_bn = [&](int spec, ExtractBuf y, long y_elems, int y_ld, long M, int C, ExtractBuf res, int res_ld, int relu,
                    bool dropout, long rows_per_image) {
    ExtractStep& s = add(XS_BN_TRAIN, 0, nullptr, 0.0, 0.0);
    s.spec = spec, s.y = y, s.y_elems = y_elems, s.y_ld = y_ld, s.M = (int)M, s.Co = C, s.res = res, s.res_ld = res_ld;
    s.relu = relu, s.dropout = dropout, s.rows_per_image = rows_per_image;
  };
  // training-mode BN: the conv runs raw (the bottleneck keeps its residual, the raw PPM half of the same
  // conv); every other residual / ReLU moves after the BN
  auto add_conv = [&](size_t i) {
    const ExtractStep& o = convs[i];
    st.push_back(o);
    if (!train_bn) return;
    const bool keep_res = o.stage == 6;
    ExtractStep& c = st.back();
    c.raw = true, c.relu = 0;
    if (!keep_res) c.res = XB_NONE;
    add_bn(o.spec, o.y, 0, o.y_ld, o.M, o.Co, keep_res ? XB_NONE : o.res, o.res_ld, o.relu, keep_res, (long)o.Ho * o.Wo);
  };
  {
    ExtractStep& s = add(XS_STEM1, 2, "stem_conv1 3x64k3s2", 2.0 * N * Hs * Hs * 64 * 27,
                         4.0 * ((double)N * 3 * S * S + (double)N * Hs * Hs * 64));
    s.spec = 0, s.raw = train_bn, s.relu = train_bn ? 0 : 1;
    if (train_bn) add_bn(0, XB_A, 0, 64, (long)N * Hs * Hs, 64, XB_NONE, 0, 1, false, (long)Hs * Hs);
  }
  for (size_t i = 0; i < L.n_stem; ++i) add_conv(i);
  add(XS_MAXPOOL, 2, "maxpool3s2", 0.0, 4.0 * ((double)N * Hs * Hs * 128 + (double)N * H1 * H1 * 128));
  size_t blk = 0;  // the next block of layers 2-4 to end
  for (size_t i = L.n_stem; i < L.n_backbone; ++i) {
    add_conv(i);
    if (blk >= L.block_end.size() || (long)i != L.block_end[blk]) continue;
    // a requested block's output (after the residual and ReLU), before its buffer is reused
    if ((want_blocks >> blk) & 1) {
      ExtractStep& s = add(XS_MID_COPY, 0, nullptr, 0.0, 0.0);
      s.x = convs[i].y, s.mid_slot = (int)blk, s.M = convs[i].M, s.Co = convs[i].Co;
    }
    ++blk;
  }
  add(XS_PPM_POOL, 2, "ppm_pool", 0.0, 4.0 * ((double)N * h * h * 2048 + (double)N * 50 * 2048)).x = L.L4;
  const bool few_cells = cells <= kPpmGemmMaxRows && !kn.ppm_splitk;
  {
    ExtractStep& s = add(XS_PPM_CONV, 2, "ppm_conv smallm 2048x512", 2.0 * cells * 512 * 2048,
                         4.0 * (4.0 * 2048 * 512 + cells * 2560.0));
    s.raw = train_bn, s.few_cells = few_cells;
  }
  if (train_bn) {  // the PPM BNs on the batch statistics of their pooled cells
    long row0 = 0;
    for (int i = 0; i < 4; ++i) {
      const long Mb = (long)N * kBins[i] * kBins[i];
      add_bn(L.ppm0 + i, XB_PPM, row0 * 512, 512, Mb, 512, XB_NONE, 0, 1, false, (long)kBins[i] * kBins[i]);
      row0 += Mb;
    }
  }
  {
    ExtractStep& s = add(XS_PPM_FOLD, 2, "ppm_fold_q smallm 512x4608", 2.0 * cells * 4608 * 512,
                         4.0 * (4.0 * 512 * 4608 + cells * 5120.0));
    s.raw = train_bn, s.few_cells = few_cells;
  }
  add(XS_PPM_FIELD, 2, "ppm_field", 2.0 * N * 12 * h * 3 * 512 * 3 * 6 + 2.0 * N * h * h * 512 * 36,
      4.0 * ((double)cells * 4608 + 2.0 * z.R + z.F));
  add_conv(L.n_backbone);
  P.pass_steps = st.size();
  if (train_bn) {
    add(XS_REFOLD_PPM, 0, nullptr, 0.0, 0.0).spec = L.bott;
    add(XS_REFOLD_DOWN, 0, nullptr, 0.0, 0.0);
  }
  return P;
}

// Every record of the plan in the order a pass at profile level 3 takes them: the whole-pass record, then
// each step's, a Winograd conv's three sub-records after its own
template <typename F>
inline void for_each_record(const ExtractPlan& p, F f) {
  f(p.whole);
  for (const ExtractStep& s : p.steps) {
    if (s.rec.level > 0) f(s.rec);
    if (s.kind == XS_CONV_WINO) f(s.wino.in), f(s.wino.mm), f(s.wino.out);
  }
}

}  // namespace cwt
