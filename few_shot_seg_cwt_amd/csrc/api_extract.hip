// The frozen extractor of libcwt.so: backbone weight loading (over the table of backbone_arch.h),
// run_extract -- the executor of an ExtractPlan (extract_plan.h: every decision of a pass is made
// there, once; this file resolves buffers and launches) -- with its Winograd conv, and the
// cwt_backbone_* / cwt_extract_features* / cwt_preprocess_* entry points (include/cwt.h).  No kernels.
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
  std::vector<ConvSpec> arch;    // backbone_arch(layers)
  std::vector<ConvForms> forms;  // per spec: the operand forms load_conv built (the planner's input)
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
// The layer takes the first Ci of the spec's input channels (all of them but for the bottleneck); builds
// the operand forms `forms` names (conv_forms_built); stem1: the stem's conv1, its own weight layout.
static int load_conv(Backbone* bb, const HostParams& hp, const ConvSpec& spec, int Ci, const ConvForms& forms, float eps,
                     bool stem1, ConvLayer* L) {
  const std::string &wname = spec.wname, &bnp = spec.bnp;
  const int Co = spec.Co, k = spec.k, stride = spec.stride, pad = spec.pad, dil = spec.dil, ci_total = spec.Ci;
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
          const float v = w[(((size_t)co * ci_total + ci) * k + ky) * k + kx];
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
    if (forms.w_l && (rc = upload_u16(bb, lo3, &L->w_l))) return rc;  // [Co][K] = [Co][K/32][32]
    {  // the Winograd forms' transformed weights
      for (const int m : {2, 4}) {
        if (!(m == 2 ? forms.wino2 : forms.wino4)) continue;
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
    if (forms.w_b) {  // plain bf16 operand of the bf16 conv stack, K in packed_k64 order
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

// The layer a spec of the architecture is loaded into
static ConvLayer* layer_of(Backbone* bb, const ConvSpec& s) {
  switch (s.role) {
    case ROLE_STEM: return &bb->stem[s.bi];
    case ROLE_PPM: return &bb->ppm[s.bi];
    case ROLE_BOTT: return &bb->bott;
    default: break;
  }
  Block& b = bb->blocks[s.li][s.bi];
  return s.role == ROLE_C1 ? &b.c1 : s.role == ROLE_C2 ? &b.c2 : s.role == ROLE_C3 ? &b.c3 : &b.down;
}
static const ConvLayer* layer_of(const Backbone* bb, const ConvSpec& s) {
  return layer_of(const_cast<Backbone*>(bb), s);
}

static int load_backbone(int layers, const HostParams& hp, float eps, Backbone** out) {
  if (layers != 50 && layers != 101) return fail(CWT_EARG, "layers must be 50 or 101");
  Backbone* bb = new Backbone();
  bb->layers = layers;
  bb->eps = eps;
  bb->arch = backbone_arch(layers);
  // F(4x4) Winograd weights only when CWT_WINO=4 at load
  bb->forms = extractor_forms(bb->arch, extract_knobs_from_env().wino4_at_load);
  int rc = 0;
  auto cleanup = [&]() {
    for (void* p : bb->allocs) (void)hipFree(p);
    delete bb;
  };
  for (const ConvSpec& s : bb->arch) {
    if (s.role == ROLE_C1) bb->blocks[s.li].emplace_back();
    if (s.role == ROLE_DOWN) bb->blocks[s.li][s.bi].has_down = true;
  }
  for (size_t i = 0; i < bb->arch.size(); ++i) {
    const ConvSpec& s = bb->arch[i];
    // extractor_ci: the bottleneck conv over the layer4 half of its input alone; its PPM half is folded into
    // the PPM branch (load_ppm_fold below, from the same tensor)
    const bool stem1 = s.role == ROLE_STEM && s.bi == 0;
    if ((rc = load_conv(bb, hp, s, extractor_ci(s), bb->forms[i], eps, stem1, layer_of(bb, s)))) {
      cleanup();
      return rc;
    }
  }
  if ((rc = load_ppm_fold(bb, hp, eps)) || (rc = upload(bb, std::vector<float>(2048, 1.0f), &bb->ones)) ||
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
// (conv_igemm_x6, batch P) -> output transform with the conv's BN / residual / ReLU, as wp plans it
// (wino_plan: geometry, the GEMMs' plan and stage tag, the three sub-records).  us / ul: the
// layer's wino_s / wino_l (m = 2) or wino4_s / wino4_l (m = 4).  sk: x holds the split-K partial planes
// of the 1x1 conv that produces this conv's input, reduced inside the input transform (ctx.h).
int run_wino_conv(cwt_ctx* ctx, const float* x, int Ci, int Co, const WinoPlan& wp, const __bf16* us, const __bf16* ul,
                  const float* scale, const float* shift, const float* res, int res_ld, int relu, float* y, int y_ld,
                  int y_off, hipStream_t st, const WinoSplitKSrc* sk) {
  const WinoGeom& g = wp.g;
  if (g.m != 2 && g.m != 4) return fail(CWT_EARG, "winograd: output tile must be 2 or 4");
  if (g.T * Ci * 4 >= (1L << 31) || g.T * Co * 4 >= (1L << 31)) return fail(CWT_EARG, "winograd: plane too large");
  float *V, *Mb;
  const __bf16* zero = nullptr;
  int rc;
  if ((rc = ws(ctx, "wino.V", (size_t)g.P * g.T * Ci, &V)) || (rc = ws(ctx, "wino.M", (size_t)g.P * g.T * Co, &Mb)) ||
      (rc = zero_line(ctx, &zero)))
    return rc;
  Prof pin = open_record(ctx, st, wp.in);
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
  Prof pg = open_record(ctx, st, wp.mm);
  rc = launch_conv_x3s(a, wp.gemm, wp.gemm_stage, nullptr, 0, st, 6);
  pg.end();
  if (rc) return rc;
  Prof pout = open_record(ctx, st, wp.out);
  rc = launch_wino_out(Mb, g, Co, scale, shift, res, res_ld, relu, y, y_ld, y_off, st);
  pout.end();
  return rc;
}

// Training-mode BN of one extraction (cwt_extract_features_train_bn; bn_train.hip)
struct TrainBn {
  float momentum, drop_p;
  unsigned long long seed;
};

// One pass in flight: the plan, its buffers resolved to pointers, and what the launches need beside it
struct ExtractRun {
  cwt_ctx* ctx;
  const Backbone* bb;
  const ExtractPlan& P;
  const TrainBn* tb;
  hipStream_t st;
  float* buf[XB_COUNT] = {};  // XB_NONE stays null
  float* mid[64] = {};        // the caller's buffer per requested block (ExtractStep::mid_slot)
  float *bn_part = nullptr, *bn_sc = nullptr;
  const __bf16* zero = nullptr;
  const ConvLayer* layer(int spec) const { return layer_of(bb, bb->arch[spec]); }
};

static int resolve_buffers(ExtractRun& r, const float* img, float* feat) {
  const ExtractSizes& z = r.P.ws;
  cwt_ctx* ctx = r.ctx;
  float** b = r.buf;
  float *V, *M;
  int rc;
  if ((rc = ws(ctx, "bb.A", z.A, &b[XB_A])) || (rc = ws(ctx, "bb.B", z.A, &b[XB_B])) ||
      (rc = ws(ctx, "bb.T1", z.T1, &b[XB_T1])) || (rc = ws(ctx, "bb.T2", z.T2, &b[XB_T2])) ||
      (rc = ws(ctx, "bb.D", z.D, &b[XB_D])) || (rc = ws(ctx, "bb.COL", z.COL, &b[XB_COL])) ||
      (rc = ws(ctx, "bb.POOL", z.POOL, &b[XB_POOL])) || (rc = ws(ctx, "bb.PPM", z.PPM, &b[XB_PPM])) ||
      (rc = ws(ctx, "bb.Q", z.Q, &b[XB_Q])) || (rc = ws(ctx, "bb.R", z.R, &b[XB_R])) ||
      (rc = ws(ctx, "bb.F", z.F, &b[XB_FB])) || (rc = ws(ctx, "bb.PARTS", z.PARTS, &b[XB_PARTS])))
    return rc;
  if (r.P.traits.dma && (rc = zero_line(ctx, &r.zero))) return rc;
  if (r.tb && ((rc = ws(ctx, "bn.part", z.bn_part, &r.bn_part)) || (rc = ws(ctx, "bn.bsc", 2 * 2048, &r.bn_sc))))
    return rc;
  if (z.PART && (rc = ws(ctx, "bb.PART", z.PART, &b[XB_PART]))) return rc;
  // the Winograd convs' V / M at their largest, so run_wino_conv never grows them mid-pass
  if (z.wino_V && ((rc = ws(ctx, "wino.V", z.wino_V, &V)) || (rc = ws(ctx, "wino.M", z.wino_M, &M)))) return rc;
  b[XB_IMG] = const_cast<float*>(img);
  b[XB_FEAT] = feat;
  return 0;
}

// A conv step of any kind, under its record
static int run_conv_step(const ExtractRun& r, const ExtractStep& s) {
  const Backbone* bb = r.bb;
  const ConvSpec& spec = bb->arch[s.spec];
  const ConvLayer& L = s.kind == XS_CONV_DUAL ? bb->blocks[spec.li][spec.bi].fused : *r.layer(s.spec);
  const float *scale = s.raw ? bb->ones : L.scale, *shift = s.raw ? bb->zeros : L.shift;
  const float *x = r.buf[s.x], *res = r.buf[s.res];
  float *y = r.buf[s.y], *part = r.buf[XB_PART];
  const size_t part_floats = r.P.ws.PART;
  Prof p = open_record(r.ctx, r.st, s.rec);
  int rc;
  if (s.kind == XS_CONV_WINO) {
    // its input still in the previous conv's split-K partials: reduced by the input transform
    const ConvLayer* prod = s.part_in ? r.layer(s.in_spec) : nullptr;
    const WinoSplitKSrc sk{s.in_nsplit, prod ? prod->scale : nullptr, prod ? prod->shift : nullptr, s.in_relu};
    const bool w4 = s.wino_m == 4;
    rc = run_wino_conv(r.ctx, s.part_in ? part : x, s.Ci, s.Co, s.wino, w4 ? L.wino4_s : L.wino_s,
                       w4 ? L.wino4_l : L.wino_l, scale, shift, res, s.res_ld, s.relu, y, s.y_ld, s.y_off, r.st,
                       s.part_in ? &sk : nullptr);
  } else if (s.kind == XS_CONV_DIRECT) {
    ConvArgs a = conv_geom<ConvArgs>(s.N, s.Hi, s.Wi, s.Ci, s.Co, s.k, s.stride, s.pad, s.dil);
    a.x = x;
    a.x_ld = s.x_ld;
    a.w = L.w;
    a.scale = scale;
    a.shift = shift;
    a.res = res;
    a.res_ld = s.res_ld;
    a.y = y;
    a.y_ld = s.y_ld;
    a.y_off = s.y_off;
    a.relu = s.relu;
    rc = launch_conv(a, s.plan, s.stage, part, part_floats, r.st);
  } else {
    const ExtractMode mode = r.P.mode;
    ConvSArgs sa = conv_s_geom(s.N, s.Hi, s.Wi, s.Ci, s.Co, s.k, s.stride, s.pad, s.dil);
    sa.xs = (const __bf16*)x;  // (f32d / x6: the fp32 NHWC map, the same 128-B line geometry)
    sa.ws = mode == EM_B16 ? L.w_b : mode == EM_F32D ? (const __bf16*)L.w : L.w_s;  // x6: hi | mid (+ ws_lo)
    sa.ws_lo = mode == EM_X6 ? L.w_l : nullptr;
    sa.zero = r.zero;
    sa.scale = scale;
    sa.shift = shift;
    if (s.out_f32 || r.P.traits.out_f32) {
      sa.y = y;
      sa.y_ld = s.y_ld;
      sa.y_off = s.y_off;
      sa.res = res;
      sa.res_ld = s.res_ld;
    } else {
      sa.ys = (__bf16*)y;
      sa.res_s = (const __bf16*)res;
    }
    sa.relu = s.relu;
    if (s.kind == XS_CONV_DUAL) {
      sa.xs2 = (const __bf16*)r.buf[s.x2];
      sa.Hi2 = s.Hi2;
      sa.Wi2 = s.Wi2;
      sa.Ci2 = s.Ci2;
      sa.stride2 = s.stride2;
      sa.kt_switch = s.Ci / 32;
      sa.K = s.K;
    }
    const int prec = r.P.traits.prec;
    rc = s.part_out ? launch_conv_x3s_partials(sa, s.plan, s.stage, part, part_floats, r.st, prec)
                    : launch_conv_x3s(sa, s.plan, s.stage, part, part_floats, r.st, prec);
  }
  p.end();
  return rc;
}

// Training-mode BN of the raw fp32 output the step names, its residual and ReLU after it
static int run_bn_step(const ExtractRun& r, const ExtractStep& s) {
  const ConvLayer* L = r.layer(s.spec);
  BnTrainArgs b;
  memset(&b, 0, sizeof(b));
  b.y = r.buf[s.y] + s.y_elems;
  b.layout = ACT_F32;
  b.ld = s.y_ld;
  b.M = s.M;
  b.C = s.Co;
  b.res = r.buf[s.res];
  b.res_ld = s.res_ld;
  b.relu = s.relu;
  b.bn = L->bn;
  b.scale = L->scale;
  b.shift = L->shift;
  b.eps = r.bb->eps;
  b.momentum = r.tb->momentum;
  b.drop_p = s.dropout ? r.tb->drop_p : 0.f;
  b.seed = r.tb->seed;
  b.rows_per_image = s.rows_per_image;
  return launch_bn_train(b, r.bn_part, r.P.ws.bn_part, r.bn_sc, r.st);
}

// The two small-M GEMMs of the PPM branch over the pooled cells of the four bins
static int run_ppm_gemm_step(const ExtractRun& r, const ExtractStep& s) {
  const Backbone* bb = r.bb;
  const bool conv = s.kind == XS_PPM_CONV;
  int Mb[4];
  const float *W[4], *Sc[4], *Sh[4];
  for (int i = 0; i < 4; ++i) {
    Mb[i] = r.P.N * kBins[i] * kBins[i];
    W[i] = conv ? bb->ppm_wt[i] : s.raw ? bb->ppm_q_raw[i] : bb->ppm_q[i];
    Sc[i] = bb->ppm[i].scale;
    Sh[i] = bb->ppm[i].shift;
  }
  const bool bn = conv && !s.raw;  // the eval BN + ReLU in the GEMM's epilogue
  const float* in = r.buf[conv ? XB_POOL : XB_PPM];
  float *out = r.buf[conv ? XB_PPM : XB_Q], *parts = r.buf[XB_PARTS];
  const int Nc = conv ? 512 : 4608, K = conv ? 2048 : 512;
  const size_t parts_floats = (size_t)r.P.ws.PARTS;
  return s.few_cells ? launch_ppm_gemm(in, K, W, Mb, 4, Nc, K, bn ? Sc : nullptr, bn ? Sh : nullptr, parts, parts_floats,
                                       out, r.st)
                     : launch_smallm_gemm(in, K, W, Mb, 4, Nc, K, conv ? kKcPpm : kKcQ, parts, parts_floats,
                                          bn ? Sc : nullptr, bn ? Sh : nullptr, out, r.st);
}

// The launches of one step, under the step's record
static int run_step(const ExtractRun& r, const ExtractStep& s) {
  if (s.kind == XS_CONV_DIRECT || s.kind == XS_CONV_DMA || s.kind == XS_CONV_DUAL || s.kind == XS_CONV_WINO)
    return run_conv_step(r, s);
  const ExtractPlan& P = r.P;
  const Backbone* bb = r.bb;
  const int N = P.N, layout = P.traits.layout;
  hipStream_t st = r.st;
  float* const* b = r.buf;
  Prof p = open_record(r.ctx, st, s.rec);
  int rc = 0;
  switch (s.kind) {
    case XS_STEM1:
      rc = launch_stem_conv1(b[XB_IMG], N, P.S, bb->stem[0].w, s.raw ? bb->ones : bb->stem[0].scale,
                             s.raw ? bb->zeros : bb->stem[0].shift, b[XB_A], P.Hs, st, layout, s.relu);
      break;
    case XS_MAXPOOL: {
      const int Hs = P.Hs, H1 = P.H1;
      const __bf16* in = (const __bf16*)b[XB_A];
      __bf16* out = (__bf16*)b[XB_B];
      rc = layout == ACT_BF16    ? launch_maxpool3s2_b16(in, N, Hs, Hs, 128, out, H1, H1, st)
           : layout == ACT_SPLIT ? launch_maxpool3s2_s(in, N, Hs, Hs, 128, out, H1, H1, st)
                                 : launch_maxpool3s2(b[XB_A], N, Hs, Hs, 128, b[XB_B], H1, H1, st);
      break;
    }
    case XS_MID_COPY: {
      float* out = s.mid_slot >= 0 && s.mid_slot < 64 ? r.mid[s.mid_slot] : nullptr;
      if (!out) return fail(CWT_ESTATE, "extract plan: a mid feature copy without its buffer");
      if (layout == ACT_SPLIT)
        rc = launch_unsplit_act((const __bf16*)b[s.x], s.M, s.Co, out, s.Co, st);
      else if (layout == ACT_BF16)
        rc = launch_widen_bf16((const __bf16*)b[s.x], (long)s.M * s.Co, out, st);
      else {
        const hipError_t e = hipMemcpyAsync(out, b[s.x], (size_t)s.M * s.Co * 4, hipMemcpyDeviceToDevice, st);
        rc = e == hipSuccess ? 0 : fail((int)e, "mid feature copy");
      }
      break;
    }
    case XS_PPM_POOL: rc = launch_ppm(b[s.x], N, P.h, P.h, 2048, kBins, 4, b[XB_COL], b[XB_POOL], st, layout); break;
    case XS_PPM_CONV:
    case XS_PPM_FOLD: rc = run_ppm_gemm_step(r, s); break;
    case XS_PPM_FIELD: rc = launch_ppm_field(b[XB_Q], N, P.h, P.h, kBins, b[XB_R], b[XB_FB], st); break;
    case XS_BN_TRAIN: rc = run_bn_step(r, s); break;
    case XS_REFOLD_PPM:
      for (int i = 0; i < 4 && !rc; ++i)
        rc = launch_scale_cols(bb->ppm_q_raw[i], bb->ppm_q[i], 512L * 4608, 512, bb->bott.scale, st);
      break;
    case XS_REFOLD_DOWN:
      for (int li = 0; li < 4 && !rc; ++li)
        for (const Block& blk : bb->blocks[li])
          if (blk.has_down && !rc) rc = fold_down(blk, st);
      break;
    default: return fail(CWT_ESTATE, "extract plan: unknown step");
  }
  p.end();
  return rc;
}

// The whole extractor: plans the pass (extract_plan.h), then executes the plan's steps in order.
// tb != null: every BN on batch statistics with running-statistic update, Dropout2d on the
// bottleneck output (train.py:184 model.train() before the first support extraction).
// want_blocks / mid (eval mode only): bit i set = an fp32 NHWC copy of block i's output (extract_block_bit)
// into mid[i] ([N][h][h][512 / 1024 / 2048]; get_feat_list's features, pspnet.py:272-287)
static int run_extract(cwt_ctx* ctx, const Backbone* bb, const float* img, int N, int S, float* feat,
                       hipStream_t st, const TrainBn* tb = nullptr, uint64_t want_blocks = 0,
                       float* const* mid = nullptr) {
  const ExtractKnobs kn = extract_knobs_from_env();
  const ExtractPlan P = extract_plan(bb->arch, bb->forms, N, S, extract_mode(bb->precision, ctx->conv_arith, tb, kn), kn,
                                     want_blocks, tb != nullptr, ctx->prof_level > 0);
  if (P.error) return fail(CWT_ESTATE, P.error);
  ExtractRun r{ctx, bb, P, tb, st};
  for (int i = 0; i < 64 && mid; ++i) r.mid[i] = (want_blocks >> i) & 1 ? mid[i] : nullptr;
  int rc;
  if ((rc = resolve_buffers(r, img, feat))) return rc;
  Prof whole = open_record(ctx, st, P.whole);
  for (size_t i = 0; i < P.steps.size(); ++i) {
    if (i == P.pass_steps) whole.end();  // the post-pass refolds lie outside the pass's record
    if ((rc = run_step(r, P.steps[i]))) return rc;
  }
  whole.end();
  return 0;
}

}  // namespace cwt

using namespace cwt;

// The argument checks the cwt_extract_features* entry points share; selects the context's device
static int check_extract_args(cwt_ctx* ctx, const Backbone* bb, const float* img, const float* feat, int N, int S) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  if (!bb) return fail(CWT_ESTATE, "backbone is NULL (cwt_backbone_load)");
  if (bb->device != ctx->device) return fail(CWT_EARG, "backbone and context are on different devices");
  CWT_CHECK(img && feat, "null buffer");
  CWT_CHECK(N >= 1 && S >= 9 && (S - 1) % 8 == 0, "need N >= 1 and (S-1) % 8 == 0 (pspnet.py:150)");
  CWT_HIP(hipSetDevice(ctx->device));
  return 0;
}

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
  const Backbone* bb = reinterpret_cast<const Backbone*>(handle);
  if (const int rc = check_extract_args(ctx, bb, img, feat, N, S)) return rc;
  return run_extract(ctx, bb, img, N, S, feat, (hipStream_t)stream);
}

int cwt_extract_features_mid(cwt_ctx* ctx, const cwt_backbone* handle, const float* img, int N, int S, float* feat,
                             float* l2, float* l3, float* l4, void* stream) {
  const Backbone* bb = reinterpret_cast<const Backbone*>(handle);
  if (const int rc = check_extract_args(ctx, bb, img, feat, N, S)) return rc;
  float* const lay[3] = {l2, l3, l4};
  const uint64_t want = extract_last_blocks(bb->arch, (l2 ? 1 : 0) | (l3 ? 2 : 0) | (l4 ? 4 : 0));
  float* mid[64] = {};
  for (int i = 0; i < 3; ++i)
    if (lay[i]) mid[extract_block_bit(bb->arch, i + 1, (int)bb->blocks[i + 1].size() - 1)] = lay[i];
  return run_extract(ctx, bb, img, N, S, feat, (hipStream_t)stream, nullptr, want, mid);
}

int cwt_extract_features_blocks(cwt_ctx* ctx, const cwt_backbone* handle, const float* img, int N, int S, float* feat,
                                int n_out, const int* layer, const int* block, float* const* out, void* stream) {
  const Backbone* bb = reinterpret_cast<const Backbone*>(handle);
  if (const int rc = check_extract_args(ctx, bb, img, feat, N, S)) return rc;
  CWT_CHECK(n_out >= 0 && n_out <= 64 && (n_out == 0 || (layer && block && out)), "bad block request");
  uint64_t want = 0;
  float* mid[64] = {};
  for (int i = 0; i < n_out; ++i) {
    CWT_CHECK(layer[i] >= 2 && layer[i] <= 4 && block[i] >= 0 && out[i], "block request: layer 2..4, block >= 0, a buffer");
    const int bit = extract_block_bit(bb->arch, layer[i] - 1, block[i]);
    CWT_CHECK(bit >= 0 && bit < 64, "block request: the layer has no such bottleneck");
    CWT_CHECK(!((want >> bit) & 1), "block request: a (layer, block) pair named twice");
    want |= uint64_t(1) << bit;
    mid[bit] = out[i];
  }
  return run_extract(ctx, bb, img, N, S, feat, (hipStream_t)stream, nullptr, want, mid);
}

int cwt_extract_features_train_bn(cwt_ctx* ctx, cwt_backbone* handle, const float* img, int N, int S, float* feat,
                                  float momentum, float dropout_p, uint64_t seed, void* stream) {
  const Backbone* bb = reinterpret_cast<const Backbone*>(handle);
  if (const int rc = check_extract_args(ctx, bb, img, feat, N, S)) return rc;
  CWT_CHECK(N >= 2, "Expected more than 1 value per channel when training (the PPM bin-1 BatchNorm2d needs N >= 2)");
  CWT_CHECK(momentum >= 0.f && momentum <= 1.f && dropout_p >= 0.f && dropout_p < 1.f, "bad momentum / dropout_p");
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
