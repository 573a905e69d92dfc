// The frozen extractor of libcwt.so: backbone weight loading, the conv call list of run_extract
// (with its Winograd form) and the cwt_backbone_* / cwt_extract_features* / cwt_preprocess_* entry
// points (include/cwt.h).
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "conv_forms.h"
#include "ctx.h"

namespace cwt {

struct Block {
  ConvLayer c1, c2, c3, down;
  bool has_down = false;
  // has_down, x6: conv3 + BN and the downsample conv + BN as ONE 1x1 GEMM over the concatenated K
  // (fold_down): w / w_s / w_l the folded rows [s3 W3 | sd Wd], Ci = c3.Ci (the first source's),
  // unit scale, shift b3 + bd
  ConvLayer fused;
};

struct Backbone {  // the opaque cwt_backbone of the C ABI
  int layers = 0;
  int device = 0;
  int precision = CWT_CONV_FP32;  // cwt_backbone_set_precision
  ConvLayer stem[3];
  std::vector<Block> blocks[4];
  ConvLayer ppm[4];     // PPM 1x1 convs (scale/shift used; weights below)
  float* ppm_wt[4] = {};  // their weights K-major [2048][512] for the small-M GEMM
  ConvLayer bott;       // bottleneck conv over the 2048 layer4 channels only
  float* ppm_q[4] = {};   // bottleneck weights of PPM bin b, K-major [512][9 * 512], BN scale folded in
  float* ppm_q_raw[4] = {};  // the same without the BN scale (training-mode BN; ppm_q is refolded)
  float* ones = nullptr;     // [2048] scale / shift of a raw conv (training-mode BN)
  float* zeros = nullptr;
  float eps = 1e-5f;
  std::map<std::string, std::pair<float*, int>> bn_by_name;  // BN prefix -> (device [4][C], C)
  std::vector<void*> allocs;
};

struct HostParams {
  std::map<std::string, std::pair<const float*, int64_t>> m;
  const float* get(const std::string& k, int64_t numel, std::string* err) const {
    auto it = m.find(k);
    if (it == m.end() || it->second.first == nullptr) {
      *err = "missing tensor '" + k + "'";
      return nullptr;
    }
    if (it->second.second != numel) {
      *err = "tensor '" + k + "' has " + std::to_string(it->second.second) + " elements, expected " +
             std::to_string(numel);
      return nullptr;
    }
    return it->second.first;
  }
};

static int upload(Backbone* bb, const std::vector<float>& v, float** out) {
  void* p = nullptr;
  CWT_HIP(hipMalloc(&p, v.size() * sizeof(float)));
  CWT_HIP(hipMemcpy(p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
  bb->allocs.push_back(p);
  *out = (float*)p;
  return 0;
}

static uint16_t bf16_rne(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7F800000u) == 0x7F800000u) return (uint16_t)(u >> 16);  // inf / nan pass through
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

static float bf16_to_float(uint16_t h) {
  uint32_t u = (uint32_t)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

static int upload_u16(Backbone* bb, const std::vector<uint16_t>& v, __bf16** out) {
  void* p = nullptr;
  CWT_HIP(hipMalloc(&p, v.size() * sizeof(uint16_t)));
  CWT_HIP(hipMemcpy(p, v.data(), v.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
  bb->allocs.push_back(p);
  *out = (__bf16*)p;
  return 0;
}

// BN eval folding as PyTorch's CPU inference kernel: alpha = w / sqrt(var + eps), beta = b - mean * alpha.
// ci_total / ci_off: the stored weight has ci_total input channels; this layer takes
// [ci_off, ci_off + Ci) of them (the bottleneck's layer4 half).
static int load_conv(Backbone* bb, const HostParams& hp, const std::string& wname, const std::string& bnp, int Ci,
                     int Co, int k, int stride, int pad, int dil, float eps, bool stem1, ConvLayer* L,
                     int ci_total = -1, int ci_off = 0) {
  if (ci_total < 0) ci_total = Ci;
  std::string err;
  const float* w = hp.get(wname, (int64_t)Co * ci_total * k * k, &err);
  if (!w) return fail(CWT_EARG, err);
  const float* g = hp.get(bnp + ".weight", Co, &err);
  const float* b = g ? hp.get(bnp + ".bias", Co, &err) : nullptr;
  const float* rm = b ? hp.get(bnp + ".running_mean", Co, &err) : nullptr;
  const float* rv = rm ? hp.get(bnp + ".running_var", Co, &err) : nullptr;
  if (!rv) return fail(CWT_EARG, err);
  L->Ci = Ci;
  L->Co = Co;
  L->k = k;
  L->stride = stride;
  L->pad = pad;
  L->dil = dil;
  const int K = k * k * Ci;
  std::vector<float> packed((size_t)Co * K);
  for (int co = 0; co < Co; ++co)
    for (int ci = 0; ci < Ci; ++ci)
      for (int ky = 0; ky < k; ++ky)
        for (int kx = 0; kx < k; ++kx) {
          const float v = w[(((size_t)co * ci_total + ci_off + ci) * k + ky) * k + kx];
          if (stem1)
            packed[((size_t)(ci * 9 + ky * 3 + kx)) * Co + co] = v;
          else
            packed[(size_t)co * K + packed_k(ci, ky * k + kx, k * k)] = v;
        }
  std::vector<float> sc(Co), sh(Co);
  for (int c = 0; c < Co; ++c) {
    const float invstd = 1.0f / std::sqrt(rv[c] + eps);
    sc[c] = g[c] * invstd;
    sh[c] = b[c] - rm[c] * sc[c];
  }
  int rc;
  if ((rc = upload(bb, packed, &L->w))) return rc;
  if (!stem1) {  // bf16x3 operands: hi = bf16_rne(w), lo = bf16_rne(w - hi)
    std::vector<uint16_t> hi(packed.size()), lo(packed.size()), lo3(packed.size());
    for (size_t i = 0; i < packed.size(); ++i) {
      const float v = packed[i];
      hi[i] = bf16_rne(v);
      const float r = v - bf16_to_float(hi[i]);
      lo[i] = bf16_rne(r);
      lo3[i] = bf16_rne(r - bf16_to_float(lo[i]));  // exact: at most 8 significant bits remain
    }
    std::vector<uint16_t> sl(2 * packed.size());
    for (size_t r = 0; r < (size_t)Co; ++r)
      for (int kb = 0; kb < K / 32; ++kb)
        for (int i = 0; i < 32; ++i) {
          const size_t src = r * K + kb * 32 + i, dst = (r * (K / 32) + kb) * 64 + i;
          sl[dst] = hi[src];
          sl[dst + 32] = lo[src];
        }
    if ((rc = upload_u16(bb, sl, &L->w_s))) return rc;
    if (K % 32 == 0 && (rc = upload_u16(bb, lo3, &L->w_l))) return rc;  // [Co][K] = [Co][K/32][32]
    // the Winograd form's transformed weights: stride-1 3x3 layers with Ci >= 256 (at Ci = 128 the
    // 16 thin GEMMs and the transforms measured slower than the direct conv: 35.9 vs 29.1 us,
    // profiles/r5/sweeps)
    // F(4x4,3x3) only on request (CWT_WINO=4 at load): faster in the pipeline but ~20x the
    // rounding error of F(2x2) / the fp32 conv (DESIGN.md §3 "Measured and not kept")
    static const bool wino4 = getenv("CWT_WINO") && getenv("CWT_WINO")[0] == '4';
    if (k == 3 && stride == 1 && Ci >= 128 && Ci % 32 == 0) {
      for (const int m : {2, 4}) {
        if ((m == 2 && Ci < 256) || (m == 4 && !wino4)) continue;
        const int P = (m + 2) * (m + 2);
        const size_t n = (size_t)P * Co * Ci;
        void *U = nullptr, *us = nullptr, *ul = nullptr;
        CWT_HIP(hipMalloc(&us, n * 4));
        bb->allocs.push_back(us);
        CWT_HIP(hipMalloc(&ul, n * 2));
        bb->allocs.push_back(ul);
        CWT_HIP(hipMalloc(&U, n * 4));
        rc = launch_wino_weights(L->w, Co, Ci, (float*)U, nullptr, m);
        if (!rc) rc = launch_split_w3((const float*)U, (long)P * Co, Ci, (__bf16*)us, (__bf16*)ul, nullptr);
        const hipError_t e = hipDeviceSynchronize();
        (void)hipFree(U);
        if (rc) return rc;
        if (e != hipSuccess) return fail((int)e, "winograd weight transform");
        (m == 2 ? L->wino_s : L->wino4_s) = (__bf16*)us;
        (m == 2 ? L->wino_l : L->wino4_l) = (__bf16*)ul;
      }
    }
    if (Ci % 64 == 0) {  // plain bf16 operand of the bf16 conv stack, K in packed_k64 order
      std::vector<uint16_t> b16(packed.size());
      for (int co = 0; co < Co; ++co)
        for (int ci = 0; ci < Ci; ++ci)
          for (int tap = 0; tap < k * k; ++tap)
            b16[(size_t)co * K + packed_k64(ci, tap, k * k)] = hi[(size_t)co * K + packed_k(ci, tap, k * k)];
      if ((rc = upload_u16(bb, b16, &L->w_b))) return rc;
    }
  }
  if ((rc = upload(bb, sc, &L->scale))) return rc;
  if ((rc = upload(bb, sh, &L->shift))) return rc;
  std::vector<float> bnp4((size_t)4 * Co);
  for (int c = 0; c < Co; ++c) {
    bnp4[c] = g[c];
    bnp4[Co + c] = b[c];
    bnp4[2 * Co + c] = rm[c];
    bnp4[3 * Co + c] = rv[c];
  }
  if ((rc = upload(bb, bnp4, &L->bn))) return rc;
  bb->bn_by_name[bnp] = {L->bn, Co};
  return 0;
}

// Weights of the folded PPM branch (backbone.hip, PPM section): the PPM 1x1 conv weights
// transposed to [2048][512], and per bin b the bottleneck taps over that bin's 512 concat
// channels as Wq_b[ci][tap * 512 + co] = W[co][2048 + 512 b + ci][tap] * bn_scale[co].
static int load_ppm_fold(Backbone* bb, const HostParams& hp, float eps) {
  std::string err;
  for (int b = 0; b < 4; ++b) {
    const float* w = hp.get("ppm.features." + std::to_string(b) + ".1.weight", (int64_t)512 * 2048, &err);
    if (!w) return fail(CWT_EARG, err);
    std::vector<float> t((size_t)2048 * 512);
    for (int co = 0; co < 512; ++co)
      for (int ci = 0; ci < 2048; ++ci) t[(size_t)ci * 512 + co] = w[(size_t)co * 2048 + ci];
    int rc;
    if ((rc = upload(bb, t, &bb->ppm_wt[b]))) return rc;
  }
  const float* w = hp.get("bottleneck.0.weight", (int64_t)512 * 4096 * 9, &err);
  const float* g = w ? hp.get("bottleneck.1.weight", 512, &err) : nullptr;
  const float* rv = g ? hp.get("bottleneck.1.running_var", 512, &err) : nullptr;
  if (!rv) return fail(CWT_EARG, err);
  for (int b = 0; b < 4; ++b) {
    std::vector<float> q((size_t)512 * 4608), qr((size_t)512 * 4608);
    for (int co = 0; co < 512; ++co) {
      const float sc = g[co] * (1.0f / std::sqrt(rv[co] + eps));  // as load_conv's BN fold
      for (int ci = 0; ci < 512; ++ci)
        for (int tap = 0; tap < 9; ++tap) {
          const float v = w[((size_t)co * 4096 + 2048 + 512 * b + ci) * 9 + tap];
          qr[(size_t)ci * 4608 + tap * 512 + co] = v;
          q[(size_t)ci * 4608 + tap * 512 + co] = v * sc;
        }
    }
    int rc;
    if ((rc = upload(bb, q, &bb->ppm_q[b])) || (rc = upload(bb, qr, &bb->ppm_q_raw[b]))) return rc;
  }
  return 0;
}

// The declared exact shortcut of a block with a downsample branch: both branches are
// 1x1 convs onto the same M x Co output, each followed by an eval-mode BN (a per-channel affine), so
//   relu(bn3(conv3(t)) + bnd(convd(x))) = relu([t | x] . [s3 W3 ; sd Wd]^T + (b3 + bd)).
// (Re)builds b.fused's rows from the two layers' current eval folds, then the x6 split; the folds
// change with the BN running statistics, so a training-mode BN pass calls this again.
static int fold_down(const Block& b, hipStream_t st) {
  const int K1 = b.c3.Ci, K2 = b.down.Ci, Co = b.c3.Co;
  int rc = launch_fold_dual(b.c3.w, b.c3.scale, b.c3.shift, K1, b.down.w, b.down.scale, b.down.shift, K2, Co,
                            b.fused.w, b.fused.shift, st);
  if (!rc) rc = launch_split_w3(b.fused.w, Co, K1 + K2, b.fused.w_s, b.fused.w_l, st);
  return rc;
}

static int alloc_fused(Backbone* bb, Block* b) {
  const size_t n = (size_t)b->c3.Co * (b->c3.Ci + b->down.Ci);
  void *w = nullptr, *s = nullptr, *l = nullptr, *sh = nullptr;
  CWT_HIP(hipMalloc(&w, n * 4));
  bb->allocs.push_back(w);
  CWT_HIP(hipMalloc(&s, n * 4));
  bb->allocs.push_back(s);
  CWT_HIP(hipMalloc(&l, n * 2));
  bb->allocs.push_back(l);
  CWT_HIP(hipMalloc(&sh, (size_t)b->c3.Co * 4));
  bb->allocs.push_back(sh);
  ConvLayer& F = b->fused;
  F.Ci = b->c3.Ci;
  F.Co = b->c3.Co;
  F.w = (float*)w;
  F.w_s = (__bf16*)s;
  F.w_l = (__bf16*)l;
  F.scale = bb->ones;
  F.shift = (float*)sh;
  const int rc = fold_down(*b, nullptr);
  if (rc) return rc;
  CWT_HIP(hipDeviceSynchronize());
  return 0;
}

static int load_backbone(int layers, const HostParams& hp, float eps, Backbone** out) {
  if (layers != 50 && layers != 101) return fail(CWT_EARG, "layers must be 50 or 101");
  Backbone* bb = new Backbone();
  bb->layers = layers;
  bb->eps = eps;
  int rc = 0;
  auto cleanup = [&]() {
    for (void* p : bb->allocs) (void)hipFree(p);
    delete bb;
  };
  // layer0: deep-base stem (resnet.py:110-118)
  if ((rc = load_conv(bb, hp, "layer0.0.weight", "layer0.1", 3, 64, 3, 2, 1, 1, eps, true, &bb->stem[0])) ||
      (rc = load_conv(bb, hp, "layer0.3.weight", "layer0.4", 64, 64, 3, 1, 1, 1, eps, false, &bb->stem[1])) ||
      (rc = load_conv(bb, hp, "layer0.6.weight", "layer0.7", 64, 128, 3, 1, 1, 1, eps, false, &bb->stem[2]))) {
    cleanup();
    return rc;
  }
  const int* nb = (layers == 50) ? kBlocks50 : kBlocks101;
  int inplanes = 128;
  const int planes_of[4] = {64, 128, 256, 512};
  for (int li = 0; li < 4; ++li) {
    const int planes = planes_of[li];
    for (int bi = 0; bi < nb[li]; ++bi) {
      Block B;
      // dilation surgery (pspnet.py:103-112): layer3 conv2 d2 s1, layer4 conv2 d4 s1, downsample s1
      int s2 = 1, d2 = 1, sd = 1;
      if (li == 1 && bi == 0) {
        s2 = 2;
        sd = 2;
      }
      if (li == 2) d2 = 2;
      if (li == 3) d2 = 4;
      const std::string p = "layer" + std::to_string(li + 1) + "." + std::to_string(bi);
      if ((rc = load_conv(bb, hp, p + ".conv1.weight", p + ".bn1", inplanes, planes, 1, 1, 0, 1, eps, false, &B.c1)) ||
          (rc = load_conv(bb, hp, p + ".conv2.weight", p + ".bn2", planes, planes, 3, s2, d2, d2, eps, false, &B.c2)) ||
          (rc = load_conv(bb, hp, p + ".conv3.weight", p + ".bn3", planes, planes * 4, 1, 1, 0, 1, eps, false,
                          &B.c3))) {
        cleanup();
        return rc;
      }
      if (bi == 0) {
        B.has_down = true;
        if ((rc = load_conv(bb, hp, p + ".downsample.0.weight", p + ".downsample.1", inplanes, planes * 4, 1, sd, 0, 1,
                            eps, false, &B.down))) {
          cleanup();
          return rc;
        }
      }
      inplanes = planes * 4;
      bb->blocks[li].push_back(B);
    }
  }
  for (int i = 0; i < 4; ++i) {
    const std::string p = "ppm.features." + std::to_string(i);
    if ((rc = load_conv(bb, hp, p + ".1.weight", p + ".2", 2048, 512, 1, 1, 0, 1, eps, false, &bb->ppm[i]))) {
      cleanup();
      return rc;
    }
  }
  if ((rc = load_conv(bb, hp, "bottleneck.0.weight", "bottleneck.1", 2048, 512, 3, 1, 1, 1, eps, false, &bb->bott,
                      4096, 0)) ||
      (rc = load_ppm_fold(bb, hp, eps)) || (rc = upload(bb, std::vector<float>(2048, 1.0f), &bb->ones)) ||
      (rc = upload(bb, std::vector<float>(2048, 0.0f), &bb->zeros))) {
    cleanup();
    return rc;
  }
  for (int li = 0; li < 4; ++li)
    for (Block& b : bb->blocks[li])
      if (b.has_down && (rc = alloc_fused(bb, &b))) {
        cleanup();
        return rc;
      }
  *out = bb;
  return 0;
}

ConvArgs make_args(const ConvCall& c) {
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  const ConvLayer& L = *c.L;
  a.x = c.x;
  a.w = L.w;
  a.scale = L.scale;
  a.shift = L.shift;
  a.res = c.res;
  a.y = c.y;
  a.N = c.N;
  a.Hi = c.Hi;
  a.Wi = c.Wi;
  a.Ci = L.Ci;
  a.x_ld = c.x_ld;
  a.Ho = conv_out_size(c.Hi, L.k, L.stride, L.pad, L.dil);
  a.Wo = conv_out_size(c.Wi, L.k, L.stride, L.pad, L.dil);
  a.Co = L.Co;
  a.kh = a.kw = L.k;
  a.stride = L.stride;
  a.pad = L.pad;
  a.dil = L.dil;
  a.M = c.N * a.Ho * a.Wo;
  a.K = L.k * L.k * L.Ci;
  a.y_ld = c.y_ld;
  a.y_off = c.y_off;
  a.res_ld = c.res_ld;
  a.relu = c.relu;
  return a;
}

// The Winograd output tile the x6 stack takes for a stride-1 3x3 conv by default (0 = the direct
// conv): F(2x2,3x3) for Ci >= 256 (at Ci = 128 the direct conv measured faster).  F(4x4,3x3)
// only on request (CWT_WINO=4): its rounding error is ~20x F(2x2)'s (4e-6 .. 1.2e-5 of max |y|
// per conv against 2-6e-7; the fp32 GEMM's accumulation error, amplified by the transforms), for
// +8 % pipelined throughput (profiles/r5/wino4/)
static int wino_tile_default(int Ci, int Co, int d, int Ho) {
  (void)Co;
  (void)d;
  (void)Ho;
  return Ci >= 256 ? 2 : 0;
}

// The debug entry points' forced form: bm = 1000 * variant + rows (cwt_debug.h) and bn must name a
// row of the family's form table (conv_forms.h); a timing-study form's fixed tile replaces the one
// named beside it (the grid must be the kernel's).
int force_conv_form(int prec, int bm, int bn, int Co, ConvPlan* p) {
  const int var = bm / 1000;
  bm %= 1000;
  CWT_CHECK(find_conv_form(prec, bm, bn, 0),
            "tile must be one of 256x256, 256x128, 128x256, 128x128, 128x64, 64x128, 64x64");
  const ConvForm* f = fixed_tile_form(prec, var);
  if (!f) f = find_conv_form(prec, bm, bn, var);
  CWT_CHECK(f, "no such conv form: the variant does not exist on this tile (conv_forms.h)");
  CWT_CHECK(Co % f->bn == 0, "Co % bn");
  p->bm = f->bm;
  p->bn = f->bn;
  p->var = var;
  return 0;
}

// One stride-1 3x3 conv (dilation d = padding) in the Winograd form F(m x m, 3x3) on the x6
// matrix-core arithmetic (wino.hip): input transform -> P = (m+2)^2 batched GEMMs
// (conv_igemm_x6, batch P) -> output transform with the conv's BN / residual / ReLU.  us / ul: the
// layer's wino_s / wino_l (m = 2) or wino4_s / wino4_l (m = 4); bm > 0 overrides the GEMMs' tile
// (bm = 1000 * variant + rows, as cwt_debug_conv_s).  sk: x holds the split-K partial planes of the
// 1x1 conv that produces this conv's input, reduced inside the input transform (ctx.h).
int run_wino_conv(cwt_ctx* ctx, const float* x, int N, int H, int W, int Ci, int Co, int d, int m,
                         const __bf16* us, const __bf16* ul, const float* scale, const float* shift, const float* res,
                         int res_ld, int relu, float* y, int y_ld, int y_off, int stage, hipStream_t st, int bm,
                         int bn, const WinoSplitKSrc* sk) {
  if (m != 2 && m != 4) return fail(CWT_EARG, "winograd: output tile must be 2 or 4");
  const WinoGeom g = wino_geom(N, H, W, d, m);
  if (g.T * Ci * 4 >= (1L << 31) || g.T * Co * 4 >= (1L << 31)) return fail(CWT_EARG, "winograd: plane too large");
  float *V, *Mb;
  const __bf16* zero = nullptr;
  int rc;
  ConvPlan p = plan_conv_s(6, (int)g.T, Co, Ci, g.P);
  if (bm > 0 && (rc = force_conv_form(6, bm, bn, Co, &p))) return rc;
  if ((rc = ws(ctx, "wino.V", (size_t)g.P * g.T * Ci, &V)) || (rc = ws(ctx, "wino.M", (size_t)g.P * g.T * Co, &Mb)) ||
      (rc = zero_line(ctx, &zero)))
    return rc;
  // sub-records (the executed work of the form): the transforms' algorithmic bytes
  // and the batched GEMMs' executed FLOPs, at profile level 3 only (their event pairs would add
  // ~10 us of gaps to each Winograd conv's own bracket at levels 1 and 2)
  const int plev = 3;
  (void)stage;
  const double vb = 4.0 * g.P * g.T * Ci, mb = 4.0 * g.P * g.T * Co;
  Prof pin(ctx, st, "wino_in " + std::to_string(Ci) + "@" + std::to_string(H), 0.0,
           4.0 * N * H * W * Ci * (sk ? sk->nsplit : 1) + vb, plev);
  rc = sk ? launch_wino_in_splitk(x, sk->nsplit, sk->scale, sk->shift, sk->relu, g, Ci, V, st)
          : launch_wino_in(x, g, Ci, V, st);
  pin.end();
  if (rc) return rc;
  ConvSArgs a = conv_s_geom(1, (int)g.T, 1, Ci, Co, 1, 1, 0, 1);  // each GEMM: a 1x1 conv over the T tiles
  a.xs = (const __bf16*)V;
  a.ws = us;
  a.ws_lo = ul;
  a.zero = zero;
  a.scale = scale;
  a.shift = shift;
  a.part = Mb;
  a.batch = g.P;
  a.xs_bstride = g.T * Ci * 4;
  a.ws_bstride = (long)Co * Ci * 2;
  a.wl_bstride = (long)Co * Ci;
  // the batched GEMMs are the stage-7 (F(2x2)) / stage-8 (F(4x4)) instantiations, the
  // bottleneck's (stage 6) its own: their own rocprofv3 statistics
  Prof pg(ctx, st, "wino_gemm " + std::to_string(Ci) + "x" + std::to_string(Co) + "@" + std::to_string(H),
          2.0 * g.P * g.T * Ci * Co, vb + 6.0 * g.P * Co * Ci + mb, plev);
  rc = launch_conv_x3s(a, p, m == 4 ? 8 : stage == 6 ? 6 : 7, nullptr, 0, st, 6);
  pg.end();
  if (rc) return rc;
  const double ob = 4.0 * N * H * W * Co * (res ? 2.0 : 1.0);
  Prof pout(ctx, st, "wino_out " + std::to_string(Co) + "@" + std::to_string(H), 0.0, mb + ob, plev);
  rc = launch_wino_out(Mb, g, Co, scale, shift, res, res_ld, relu, y, y_ld, y_off, st);
  pout.end();
  return rc;
}

// Training-mode BN of one extraction (cwt_extract_features_train_bn; bn_train.hip)
struct TrainBn {
  float momentum, drop_p;
  unsigned long long seed;
};

// The whole extractor as a list of conv calls + byte kernels.  dry_run sizes the split-K workspace.
// tb != null: every BN on batch statistics with running-statistic update, Dropout2d on the
// bottleneck output (train.py:184 model.train() before the first support extraction).
// mid (optional, eval mode only): fp32 NHWC copies of the outputs of layer2, layer3 and layer4
// ([N][h][h][512 / 1024 / 2048]; get_feat_list's per-layer features, pspnet.py:272-287)
static int run_extract(cwt_ctx* ctx, const Backbone* bb, const float* img, int N, int S, float* feat,
                       hipStream_t st, const TrainBn* tb = nullptr, float* const* mid = nullptr) {
  // conv arithmetic / activation storage: plain bf16 (cwt_backbone_set_precision), else the
  // context's fp32-accurate mode (S-layout bf16x3 by default)
  // the training-mode BN pass (once per epoch) amplifies conv rounding ~100x through its
  // batch statistics: it runs the exact-fp32 conv path in either precision (a
  // bf16 backbone too: the CPU emulation of its roundings, tests/bf16_ref.py, is 0.6 off the
  // exact features at R50 S = 65)
  const bool b16 = bb->precision == CWT_CONV_BF16 && !tb;
  const bool conv_split = ctx->conv_arith == CWT_CONV_ARITH_BF16X3 && !tb;
  const bool s_path = b16 || conv_split;  // S-layout / bf16 activations
  const int layout = b16 ? ACT_BF16 : conv_split ? ACT_SPLIT : ACT_F32;
  // the exact-fp32 path (eval mode) runs on the same LDS-DMA conv body (conv_igemm_f32d: fp32
  // NHWC activations, f32 MFMA); CWT_CONV_F32D=0 selects the register-staged conv_igemm_f32
  static const bool f32d_env = !(getenv("CWT_CONV_F32D") && getenv("CWT_CONV_F32D")[0] == '0');
  // fp32 width on the bf16 matrix cores (conv_igemm_x6): f32d's operands, split in registers
  const bool x6 = !s_path && !tb && ctx->conv_arith == CWT_CONV_ARITH_BF16X6;
  const bool f32d = !s_path && !tb && !x6 && f32d_env;
  const bool f32ops = f32d || x6;  // fp32 NHWC operands on the LDS-DMA body
  const bool dma = s_path || f32ops;  // conv_x3s.hip kernels
  const int prec = b16 ? 1 : conv_split ? 3 : x6 ? 6 : 0;
  // x6 (eval mode) only, A/B knobs read per call: CWT_FUSE_DOWN=0 restores the downsample conv as a
  // launch of its own (through D), CWT_FUSE_SPLITK_WINO=0 the split-K epilogue launch in front of a
  // Winograd conv
  const auto knob_on = [](const char* name) {
    const char* v = getenv(name);
    return !(v && v[0] == '0');
  };
  const bool fuse_down = x6 && knob_on("CWT_FUSE_DOWN");
  const bool fuse_splitk = x6 && knob_on("CWT_FUSE_SPLITK_WINO");
  const int Hs = down2(S), H1 = down2(Hs), h = down2(H1);
  const long sA = std::max({(long)N * Hs * Hs * 128, (long)N * H1 * H1 * 256, (long)N * h * h * 2048});
  const long sT1 = std::max((long)N * H1 * H1 * 128, (long)N * h * h * 512);
  const long sT2 = std::max((long)N * H1 * H1 * 64, (long)N * h * h * 512);
  const long sD = std::max((long)N * H1 * H1 * 256, (long)N * h * h * 2048);
  const long sCol = (long)N * h * 16 * 2048 + (long)N * 16 * 16 * 2048;  // PPM row-segment + block sums
  const long sPool = (long)N * 50 * 2048;
  const long sPpm = (long)N * 50 * 512;
  const long sQ = (long)N * 50 * 4608;
  const long sR = (long)N * 12 * h * 3 * 512;
  const long sF = (long)N * h * h * 512;
  constexpr int kKcPpm = 32, kKcQ = 64;  // K chunk of the two small-M GEMMs
  const long sPartS = std::max((long)(2048 / kKcPpm) * N * 50 * 512, (long)(512 / kKcQ) * N * 50 * 4608);

  // collect every conv call first (to size split-K scratch), then run
  float *A, *B, *T1, *T2, *D, *COL, *POOL, *PPM, *QB, *RB, *FB, *PARTS;
  int rc;
  if ((rc = ws(ctx, "bb.A", sA, &A)) || (rc = ws(ctx, "bb.B", sA, &B)) || (rc = ws(ctx, "bb.T1", sT1, &T1)) ||
      (rc = ws(ctx, "bb.T2", sT2, &T2)) || (rc = ws(ctx, "bb.D", sD, &D)) || (rc = ws(ctx, "bb.COL", sCol, &COL)) ||
      (rc = ws(ctx, "bb.POOL", sPool, &POOL)) || (rc = ws(ctx, "bb.PPM", sPpm, &PPM)) ||
      (rc = ws(ctx, "bb.Q", sQ, &QB)) || (rc = ws(ctx, "bb.R", sR, &RB)) || (rc = ws(ctx, "bb.F", sF, &FB)) ||
      (rc = ws(ctx, "bb.PARTS", sPartS, &PARTS)))
    return rc;

  std::vector<ConvCall> calls;
  std::vector<ConvArgs> args;  // make_args(calls[i]), computed once; plans[i] below
  int stage = 0;
  auto cc = [&](const ConvLayer* L, const float* x, int n, int Hi, int Wi, int x_ld, float* y, int y_ld, int y_off,
                const float* res, int res_ld, int relu) {
    ConvCall c{stage, L, x, n, Hi, Wi, x_ld, y, y_ld, y_off, res, res_ld, relu, stage == 6};
    calls.push_back(c);
    args.push_back(make_args(c));
  };
  // stem conv2/conv3 (conv1 and maxpool are separate kernels, ordered below by index)
  cc(&bb->stem[1], A, N, Hs, Hs, 64, B, 64, 0, nullptr, 0, 1);
  cc(&bb->stem[2], B, N, Hs, Hs, 64, A, 128, 0, nullptr, 0, 1);
  const size_t n_stem_calls = calls.size();
  size_t last_of_layer[4] = {0, 0, 0, 0};  // call index of each layer's last block (mid features)
  float* cur = B;  // maxpool output
  float* other = A;
  int H = H1;
  for (int li = 0; li < 4; ++li) {
    stage = li + 1;
    const int nbk = (int)bb->blocks[li].size();
    for (int bi = 0; bi < nbk; ++bi) {
      const Block& blk = bb->blocks[li][bi];
      const int Cin = blk.c1.Ci;
      const int Ho = (blk.c2.stride == 2) ? down2(H) : H;
      cc(&blk.c1, cur, N, H, H, Cin, T1, blk.c1.Co, 0, nullptr, 0, 1);
      cc(&blk.c2, T1, N, H, H, blk.c2.Ci, T2, blk.c2.Co, 0, nullptr, 0, 1);
      const float* res = cur;
      int res_ld = Cin;
      if (blk.has_down && fuse_down) {  // conv3 + downsample conv as one two-source GEMM (fold_down)
        cc(&blk.fused, T2, N, Ho, Ho, blk.c3.Ci, other, blk.c3.Co, 0, nullptr, 0, 1);
        ConvCall& c = calls.back();
        c.x2 = cur;
        c.Hi2 = c.Wi2 = H;
        c.Ci2 = Cin;
        c.stride2 = blk.down.stride;
        args.back().K += Cin;
      } else {
        if (blk.has_down) {
          cc(&blk.down, cur, N, H, H, Cin, D, blk.down.Co, 0, nullptr, 0, 0);
          res = D;
          res_ld = blk.down.Co;
        }
        cc(&blk.c3, T2, N, Ho, Ho, blk.c3.Ci, other, blk.c3.Co, 0, res, res_ld, 1);
      }
      if (bi == nbk - 1) last_of_layer[li] = calls.size() - 1;
      std::swap(cur, other);
      H = Ho;
    }
  }
  const size_t n_backbone_calls = calls.size();
  const float* L4 = cur;  // layer4 output [N][h][h][2048]
  // the bottleneck conv over the layer4 channels; the folded PPM field FB enters as residual
  stage = 6;
  cc(&bb->bott, L4, N, h, h, 2048, feat, 512, 0, FB, 512, 1);

  // split-K scratch
  size_t part_floats = 0;
  std::vector<ConvPlan> plans;
  for (size_t i = 0; i < calls.size(); ++i) {
    const ConvArgs& a = args[i];
    if (b16 && !calls[i].L->w_b) return fail(CWT_ESTATE, "bf16 conv weights missing (Ci % 64 != 0)");
    ConvPlan pl = calls[i].x2 ? plan_conv_dual(a.M, a.Co, a.K)
                  : dma       ? plan_conv_s(prec, a.M, a.Co, a.K)
                              : plan_conv(a.M, a.Co, a.K);
    plans.push_back(pl);
    if (pl.nsplit > 1) part_floats = std::max(part_floats, (size_t)pl.nsplit * a.M * a.Co);
  }
  const __bf16* zero = nullptr;
  if (dma && (rc = zero_line(ctx, &zero))) return rc;
  float *BNPART = nullptr, *BNSC = nullptr;
  size_t bn_part_floats = 0;
  if (tb) {
    bn_part_floats = bn_train_part_floats((long)N * Hs * Hs, 64);
    for (auto& a : args) bn_part_floats = std::max(bn_part_floats, bn_train_part_floats(a.M, a.Co));
    if ((rc = ws(ctx, "bn.part", bn_part_floats, &BNPART)) || (rc = ws(ctx, "bn.bsc", 2 * 2048, &BNSC))) return rc;
  }
  // training-mode BN of a raw conv output y (layout / row stride), residual and ReLU after it
  auto bn_train = [&](const ConvLayer* L, void* y, int lay, int ld, long M, const void* res, int res_ld, int relu,
                      float drop_p, long rows_per_image) -> int {
    BnTrainArgs b;
    memset(&b, 0, sizeof(b));
    b.y = y;
    b.layout = lay;
    b.ld = ld;
    b.M = M;
    b.C = L->Co;
    b.res = res;
    b.res_ld = res_ld;
    b.relu = relu;
    b.bn = L->bn;
    b.scale = L->scale;
    b.shift = L->shift;
    b.eps = bb->eps;
    b.momentum = tb->momentum;
    b.drop_p = drop_p;
    b.seed = tb->seed;
    b.rows_per_image = rows_per_image;
    return launch_bn_train(b, BNPART, bn_part_floats, BNSC, st);
  };
  float* PART = nullptr;
  if (part_floats && (rc = ws(ctx, "bb.PART", part_floats, &PART))) return rc;
  // the Winograd form: stride-1 3x3 layers whose transformed weights were built at load, on
  // images of a pixel stride equal to their channels
  auto c_wino = [&](const ConvCall& c) {
    return (c.L->wino_s || c.L->wino4_s) && c.L->k == 3 && c.L->stride == 1 && c.L->pad == c.L->dil &&
           c.x_ld == c.L->Ci;
  };
  // the Winograd output tile call i takes (0: the direct conv)
  // A/B: CWT_WINO=0 every conv direct, 2 / 4 every Winograd-eligible conv in F(2x2) / F(4x4)
  static const int wino_env = getenv("CWT_WINO") && getenv("CWT_WINO")[0] ? atoi(getenv("CWT_WINO")) : -1;
  auto wino_tile = [&](size_t i) {
    const ConvArgs& a = args[i];
    int wm = x6 && wino_env != 0 && c_wino(calls[i])
                 ? (wino_env == 2 || wino_env == 4 ? wino_env : wino_tile_default(a.Ci, a.Co, a.dil, a.Ho))
                 : 0;
    if (wm && !(wm == 4 ? calls[i].L->wino4_s : calls[i].L->wino_s)) wm = 0;  // form not built for this layer
    return wm;
  };
  // call i leaves its split-K partials unreduced for call i + 1's input transform: a split-K conv
  // into T1 (a block's conv1: read by its conv2 alone, never a mid feature) in front of a Winograd conv
  auto partials_to_wino = [&](size_t i) {
    return fuse_splitk && i + 1 < n_backbone_calls && plans[i].nsplit > 1 && calls[i].y == T1 && !calls[i].res &&
           calls[i].y_off == 0 && calls[i].y_ld == args[i].Co && calls[i + 1].x == T1 && !wino_tile(i) &&
           wino_tile(i + 1) != 0;
  };
  auto run_call = [&](size_t i) -> int {
    ConvArgs a = args[i];  // a copy: the training-mode BN override below
    // training-mode BN: raw conv (scale 1, shift 0); the bottleneck keeps its residual (the
    // raw PPM half of the same conv), every other residual / ReLU moves after the BN
    const bool keep_res = calls[i].stage == 6;
    if (tb) {
      a.scale = bb->ones;
      a.shift = bb->zeros;
      a.relu = 0;
      if (!keep_res) a.res = nullptr;
    }
    const int wm = wino_tile(i);
    const bool wino = wm != 0;
    const bool part_out = partials_to_wino(i), part_in = i > 0 && partials_to_wino(i - 1);
    // the Winograd form's record names its batched GEMM's plan; its FLOPs stay the direct conv's
    // (algorithmic: the roofline prices the conv, not the form that computes it)
    const WinoGeom wg = wino_geom(a.N, a.Hi, a.Wi, a.dil, wm ? wm : 2);
    const ConvPlan pl = wino ? plan_conv_s(6, (int)wg.T, a.Co, a.Ci, wg.P) : plans[i];
    const double flops = 2.0 * a.M * a.Co * a.K;
    // algorithmic bytes: every operand once; 4 B per element (fp32 or the bf16x3 S-layout),
    // 2 B for the bf16 stack's activations and weights (its fp32 bottleneck output: 4 B)
    const double eb = b16 ? 2.0 : 4.0, ob = calls[i].out_f32 ? 4.0 : eb;
    const ConvCall& cl = calls[i];
    const double bytes = eb * ((double)a.N * a.Hi * a.Wi * a.Ci + (double)a.N * cl.Hi2 * cl.Wi2 * cl.Ci2 +
                               (double)a.Co * a.K) +
                         ob * ((double)a.M * a.Co + (a.res ? (double)a.M * a.Co : 0.0));
    Prof p(ctx, st,
           std::string(b16 ? "conv_igemm_b16<" : conv_split ? "conv_igemm_x3s<" : wino ? (wm == 4 ? "conv_igemm_x6w4<" : "conv_igemm_x6w<")
                       : x6 ? "conv_igemm_x6<" : f32d ? "conv_igemm_f32d<" : "conv_igemm_f32<") +
               std::to_string(pl.bm) + "," +
               std::to_string(pl.bn) + "," +
               std::to_string(calls[i].stage) + ">" +
               (pl.nsplit > 1 ? "+splitk" + std::to_string(pl.nsplit) : std::string()) + " " +
               std::to_string(a.Ci) + (cl.x2 ? "+" + std::to_string(cl.Ci2) : std::string()) + "x" +
               std::to_string(a.Co) + "k" + std::to_string(a.kh) + "s" +
               std::to_string(a.stride) + "d" + std::to_string(a.dil) + "@" + std::to_string(a.Ho),
           flops, bytes, calls[i].stage == 6 ? 1 : 2);
    int r;
    if (wino) {
      const ConvCall& c = calls[i];
      // its input still in the previous call's split-K partials: reduced by the input transform
      const WinoSplitKSrc sk{part_in ? plans[i - 1].nsplit : 0, part_in ? calls[i - 1].L->scale : nullptr,
                             part_in ? calls[i - 1].L->shift : nullptr, part_in ? calls[i - 1].relu : 0};
      r = run_wino_conv(ctx, part_in ? PART : c.x, a.N, a.Hi, a.Wi, a.Ci, a.Co, a.dil, wm,
                        wm == 4 ? c.L->wino4_s : c.L->wino_s, wm == 4 ? c.L->wino4_l : c.L->wino_l, a.scale, a.shift,
                        a.res, c.res_ld, a.relu, c.y, c.y_ld, c.y_off, c.stage, st, 0, 0, part_in ? &sk : nullptr);
    } else if (dma) {
      ConvSArgs sa = conv_s_geom(a.N, a.Hi, a.Wi, a.Ci, a.Co, a.kh, a.stride, a.pad, a.dil);
      const ConvCall& c = calls[i];
      sa.xs = (const __bf16*)c.x;  // (f32d: the fp32 NHWC map, the same 128-B line geometry)
      sa.ws = b16 ? c.L->w_b : f32d ? (const __bf16*)c.L->w : c.L->w_s;  // x6: hi | mid (+ ws_lo)
      sa.ws_lo = x6 ? c.L->w_l : nullptr;
      sa.zero = zero;
      sa.scale = a.scale;
      sa.shift = a.shift;
      if (c.out_f32 || f32ops) {
        sa.y = c.y;
        sa.y_ld = c.y_ld;
        sa.y_off = c.y_off;
        sa.res = a.res;
        sa.res_ld = c.res_ld;
      } else {
        sa.ys = (__bf16*)c.y;
        sa.res_s = (const __bf16*)a.res;
      }
      sa.relu = a.relu;
      if (c.x2) {
        sa.xs2 = (const __bf16*)c.x2;
        sa.Hi2 = c.Hi2;
        sa.Wi2 = c.Wi2;
        sa.Ci2 = c.Ci2;
        sa.stride2 = c.stride2;
        sa.kt_switch = a.Ci / 32;
        sa.K = a.K;
      }
      r = part_out ? launch_conv_x3s_partials(sa, pl, c.stage, PART, part_floats, st, prec)
                   : launch_conv_x3s(sa, pl, c.stage, PART, part_floats, st, prec);
    } else {
      r = launch_conv(a, pl, calls[i].stage, PART, part_floats, st);
    }
    p.end();
    if (r || !tb) return r;
    const ConvCall& c = calls[i];
    const bool f32 = c.out_f32 || !s_path;
    return bn_train(c.L, c.y, f32 ? ACT_F32 : layout, f32 ? c.y_ld : c.L->Co, a.M, keep_res ? nullptr : c.res,
                    f32 ? c.res_ld : c.L->Co, c.relu, c.stage == 6 ? tb->drop_p : 0.f, (long)a.Ho * a.Wo);
  };

  const long cells = (long)N * 50;
  const double ppm_flops = 2.0 * cells * 512 * 2048 + 2.0 * cells * 4608 * 512 +
                           2.0 * N * 12 * h * 3 * 512 * 3 * 6 + 2.0 * N * h * h * 512 * 36;
  double all_flops = 2.0 * N * Hs * Hs * 64 * 27 + ppm_flops, all_bytes = 0.0;
  for (auto& a : args) {
    all_flops += 2.0 * a.M * a.Co * a.K;
    all_bytes += 4.0 * ((double)a.N * a.Hi * a.Wi * a.Ci + (double)a.Co * a.K + (double)a.M * a.Co);
  }
  Prof whole(ctx, st, "extract_features N=" + std::to_string(N) + " S=" + std::to_string(S), all_flops, all_bytes, 1);
  {
    Prof p(ctx, st, "stem_conv1 3x64k3s2", 2.0 * N * Hs * Hs * 64 * 27, 4.0 * ((double)N * 3 * S * S + (double)N * Hs * Hs * 64));
    if ((rc = launch_stem_conv1(img, N, S, bb->stem[0].w, tb ? bb->ones : bb->stem[0].scale,
                                tb ? bb->zeros : bb->stem[0].shift, A, Hs, st, layout, tb ? 0 : 1)))
      return rc;
    p.end();
    if (tb && (rc = bn_train(&bb->stem[0], A, layout, 64, (long)N * Hs * Hs, nullptr, 0, 1, 0.f, (long)Hs * Hs)))
      return rc;
  }
  for (size_t i = 0; i < n_stem_calls; ++i)
    if ((rc = run_call(i))) return rc;
  {
    Prof p(ctx, st, "maxpool3s2", 0.0, 4.0 * ((double)N * Hs * Hs * 128 + (double)N * H1 * H1 * 128));
    if ((rc = layout == ACT_BF16    ? launch_maxpool3s2_b16((const __bf16*)A, N, Hs, Hs, 128, (__bf16*)B, H1, H1, st)
              : layout == ACT_SPLIT ? launch_maxpool3s2_s((const __bf16*)A, N, Hs, Hs, 128, (__bf16*)B, H1, H1, st)
                                    : launch_maxpool3s2(A, N, Hs, Hs, 128, B, H1, H1, st)))
      return rc;
    p.end();
  }
  for (size_t i = n_stem_calls; i < n_backbone_calls; ++i) {
    if ((rc = run_call(i))) return rc;
    for (int li = 1; li < 4 && mid; ++li) {  // layer2 .. layer4 outputs, before the buffer is reused
      if (i != last_of_layer[li] || !mid[li - 1]) continue;
      const ConvCall& c = calls[i];
      const ConvArgs& a = args[i];
      const long P = (long)a.M;
      if (layout == ACT_SPLIT)
        rc = launch_unsplit_act((const __bf16*)c.y, P, a.Co, mid[li - 1], a.Co, st);
      else if (layout == ACT_BF16)
        rc = launch_widen_bf16((const __bf16*)c.y, P * a.Co, mid[li - 1], st);
      else {
        const hipError_t e = hipMemcpyAsync(mid[li - 1], c.y, (size_t)P * a.Co * 4, hipMemcpyDeviceToDevice, st);
        rc = e == hipSuccess ? 0 : fail((int)e, "mid feature copy");
      }
      if (rc) return rc;
    }
  }
  {
    Prof p(ctx, st, "ppm_pool", 0.0, 4.0 * ((double)N * h * h * 2048 + (double)N * 50 * 2048));
    if ((rc = launch_ppm(L4, N, h, h, 2048, kBins, 4, COL, POOL, st, layout))) return rc;
    p.end();
  }
  int Mb[4];
  const float *Wp[4], *Wq[4], *Sc[4], *Sh[4];
  static const bool ppm_splitk = getenv("CWT_PPM_SPLITK") != nullptr;  // A/B: the split-K form
  const bool few_cells = cells <= kPpmGemmMaxRows && !ppm_splitk;
  for (int i = 0; i < 4; ++i) {
    Mb[i] = N * kBins[i] * kBins[i];
    Wp[i] = bb->ppm_wt[i];
    Wq[i] = tb ? bb->ppm_q_raw[i] : bb->ppm_q[i];
    Sc[i] = bb->ppm[i].scale;
    Sh[i] = bb->ppm[i].shift;
  }
  {  // PPM 1x1 conv + BN + ReLU over the pooled cells (pspnet.py:27-29)
    Prof p(ctx, st, "ppm_conv smallm 2048x512", 2.0 * cells * 512 * 2048, 4.0 * (4.0 * 2048 * 512 + cells * 2560.0));
    if ((rc = few_cells ? launch_ppm_gemm(POOL, 2048, Wp, Mb, 4, 512, 2048, tb ? nullptr : Sc, tb ? nullptr : Sh, PARTS,
                                          (size_t)sPartS, PPM, st)
                        : launch_smallm_gemm(POOL, 2048, Wp, Mb, 4, 512, 2048, kKcPpm, PARTS, (size_t)sPartS,
                                             tb ? nullptr : Sc, tb ? nullptr : Sh, PPM, st)))
      return rc;
    p.end();
  }
  if (tb) {  // the PPM BNs on the batch statistics of their pooled cells
    long row0 = 0;
    for (int i = 0; i < 4; ++i) {
      if ((rc = bn_train(&bb->ppm[i], PPM + row0 * 512, ACT_F32, 512, Mb[i], nullptr, 0, 1, 0.f,
                         (long)kBins[i] * kBins[i])))
        return rc;
      row0 += Mb[i];
    }
  }
  {  // per-tap products of the bottleneck's PPM channels with the cells
    Prof p(ctx, st, "ppm_fold_q smallm 512x4608", 2.0 * cells * 4608 * 512, 4.0 * (4.0 * 512 * 4608 + cells * 5120.0));
    if ((rc = few_cells ? launch_ppm_gemm(PPM, 512, Wq, Mb, 4, 4608, 512, nullptr, nullptr, PARTS, (size_t)sPartS, QB, st)
                        : launch_smallm_gemm(PPM, 512, Wq, Mb, 4, 4608, 512, kKcQ, PARTS, (size_t)sPartS, nullptr,
                                             nullptr, QB, st)))
      return rc;
    p.end();
  }
  {  // separable interpolation of the per-tap products: the PPM half of the bottleneck conv
    Prof p(ctx, st, "ppm_field", 2.0 * N * 12 * h * 3 * 512 * 3 * 6 + 2.0 * N * h * h * 512 * 36,
           4.0 * ((double)cells * 4608 + 2.0 * sR + sF));
    if ((rc = launch_ppm_field(QB, N, h, h, kBins, RB, FB, st))) return rc;
    p.end();
  }
  rc = run_call(n_backbone_calls);
  whole.end();
  if (!rc && tb)  // refold the bottleneck's new eval BN scale into the PPM-branch weights
    for (int i = 0; i < 4 && !rc; ++i)
      rc = launch_scale_cols(bb->ppm_q_raw[i], bb->ppm_q[i], 512L * 4608, 512, bb->bott.scale, st);
  if (!rc && tb)  // ... and the new conv3 / downsample eval folds into the fused rows
    for (int li = 0; li < 4 && !rc; ++li)
      for (const Block& b : bb->blocks[li])
        if (b.has_down && !rc) rc = fold_down(b, st);
  return rc;
}

}  // namespace cwt

using namespace cwt;

extern "C" {

int cwt_backbone_load(cwt_ctx* ctx, int layers, int n_tensors, const char* const* names,
                      const float* const* host_data, const int64_t* numel, float bn_eps, cwt_backbone** out) {
  if (!ctx || !names || !host_data || !numel || n_tensors <= 0 || !out) return fail(CWT_EARG, "null argument");
  CWT_HIP(hipSetDevice(ctx->device));
  HostParams hp;
  for (int i = 0; i < n_tensors; ++i) hp.m[names[i]] = {host_data[i], numel[i]};
  Backbone* bb = nullptr;
  int rc = load_backbone(layers, hp, bn_eps, &bb);
  if (rc) return rc;
  bb->device = ctx->device;
  *out = reinterpret_cast<cwt_backbone*>(bb);
  return 0;
}

int cwt_backbone_destroy(cwt_backbone* handle) {
  Backbone* bb = reinterpret_cast<Backbone*>(handle);
  if (!bb) return 0;
  (void)hipSetDevice(bb->device);
  (void)hipDeviceSynchronize();
  for (void* p : bb->allocs) (void)hipFree(p);
  delete bb;
  return 0;
}

int cwt_backbone_set_precision(cwt_backbone* handle, int precision) {
  Backbone* bb = reinterpret_cast<Backbone*>(handle);
  if (!bb) return fail(CWT_EARG, "backbone is NULL");
  if (precision != CWT_CONV_FP32 && precision != CWT_CONV_BF16)
    return fail(CWT_EARG, "precision must be CWT_CONV_FP32 (0) or CWT_CONV_BF16 (1)");
  bb->precision = precision;
  return 0;
}

int cwt_extract_features(cwt_ctx* ctx, const cwt_backbone* handle, const float* img, int N, int S, float* feat,
                         void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  const Backbone* bb = reinterpret_cast<const Backbone*>(handle);
  if (!bb) return fail(CWT_ESTATE, "backbone is NULL (cwt_backbone_load)");
  if (bb->device != ctx->device) return fail(CWT_EARG, "backbone and context are on different devices");
  CWT_CHECK(img && feat, "null buffer");
  CWT_CHECK(N >= 1 && S >= 9 && (S - 1) % 8 == 0, "need N >= 1 and (S-1) % 8 == 0 (pspnet.py:150)");
  CWT_HIP(hipSetDevice(ctx->device));
  return run_extract(ctx, bb, img, N, S, feat, (hipStream_t)stream);
}

int cwt_extract_features_mid(cwt_ctx* ctx, const cwt_backbone* handle, const float* img, int N, int S, float* feat,
                             float* l2, float* l3, float* l4, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  const Backbone* bb = reinterpret_cast<const Backbone*>(handle);
  if (!bb) return fail(CWT_ESTATE, "backbone is NULL (cwt_backbone_load)");
  if (bb->device != ctx->device) return fail(CWT_EARG, "backbone and context are on different devices");
  CWT_CHECK(img && feat, "null buffer");
  CWT_CHECK(N >= 1 && S >= 9 && (S - 1) % 8 == 0, "need N >= 1 and (S-1) % 8 == 0 (pspnet.py:150)");
  CWT_HIP(hipSetDevice(ctx->device));
  float* const mid[3] = {l2, l3, l4};
  return run_extract(ctx, bb, img, N, S, feat, (hipStream_t)stream, nullptr, mid);
}

int cwt_extract_features_train_bn(cwt_ctx* ctx, cwt_backbone* handle, const float* img, int N, int S, float* feat,
                                  float momentum, float dropout_p, uint64_t seed, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  Backbone* bb = reinterpret_cast<Backbone*>(handle);
  if (!bb) return fail(CWT_ESTATE, "backbone is NULL (cwt_backbone_load)");
  if (bb->device != ctx->device) return fail(CWT_EARG, "backbone and context are on different devices");
  CWT_CHECK(img && feat, "null buffer");
  CWT_CHECK(N >= 1 && S >= 9 && (S - 1) % 8 == 0, "need N >= 1 and (S-1) % 8 == 0 (pspnet.py:150)");
  CWT_CHECK(N >= 2, "Expected more than 1 value per channel when training (the PPM bin-1 BatchNorm2d needs N >= 2)");
  CWT_CHECK(momentum >= 0.f && momentum <= 1.f && dropout_p >= 0.f && dropout_p < 1.f, "bad momentum / dropout_p");
  CWT_HIP(hipSetDevice(ctx->device));
  TrainBn tb{momentum, dropout_p, (unsigned long long)seed};
  return run_extract(ctx, bb, img, N, S, feat, (hipStream_t)stream, &tb);
}

int cwt_backbone_read_bn(const cwt_backbone* handle, const char* name, float* out, int C) {
  const Backbone* bb = reinterpret_cast<const Backbone*>(handle);
  if (!bb) return fail(CWT_ESTATE, "backbone is NULL (cwt_backbone_load)");
  CWT_CHECK(name && out, "null argument");
  auto it = bb->bn_by_name.find(name);
  if (it == bb->bn_by_name.end()) return fail(CWT_EARG, std::string("no BatchNorm2d named ") + name);
  CWT_CHECK(it->second.second == C, "C does not match the BatchNorm2d's channel count");
  CWT_HIP(hipSetDevice(bb->device));
  CWT_HIP(hipDeviceSynchronize());
  CWT_HIP(hipMemcpy(out, it->second.first, sizeof(float) * 4 * C, hipMemcpyDeviceToHost));
  return 0;
}

int cwt_preprocess_image(cwt_ctx* ctx, const void* src, int src_dtype, int H, int W, int S, const float* mean,
                         const float* std_, const float* pad, int flip_h, int flip_v, float* dst, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(src && dst && mean && std_, "null argument");
  CWT_CHECK(src_dtype == CWT_U8 || src_dtype == CWT_F32, "src_dtype must be CWT_U8 or CWT_F32");
  CWT_CHECK(H >= 1 && W >= 1 && S >= 8, "bad sizes");
  CWT_HIP(hipSetDevice(ctx->device));
  return launch_episode_image(src, src_dtype == CWT_F32, H, W, S, mean, std_, pad, flip_h, flip_v, dst,
                              (hipStream_t)stream);
}

int cwt_preprocess_label(cwt_ctx* ctx, const uint8_t* src, int H, int W, int S, int class_chosen, int flip_h,
                         int flip_v, int64_t* dst, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(src && dst, "null argument");
  CWT_CHECK(H >= 1 && W >= 1 && S >= 8, "bad sizes");
  CWT_HIP(hipSetDevice(ctx->device));
  return launch_episode_label(src, H, W, S, class_chosen, flip_h, flip_v, (long long*)dst, (hipStream_t)stream);
}

}  // extern "C"
