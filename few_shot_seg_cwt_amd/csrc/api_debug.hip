// The cwt_debug_* hooks of libcwt.so (include/cwt_debug.h): single launches of the product path on
// caller buffers, for the tests and the timing tools.
#include <algorithm>
#include <cstdlib>

#include "../../include/cwt_debug.h"
#include "conv_forms.h"
#include "ctx.h"
#include "match_plan.h"

using namespace cwt;

namespace cwt {
// HW_REG_HW_ID (wave, SIMD, CU, SH, SE fields) and HW_REG_XCC_ID of each workgroup's first wave
__global__ void census_kernel(unsigned* out) {
  unsigned hw, xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  if (threadIdx.x == 0) {
    out[2 * blockIdx.x] = hw;
    out[2 * blockIdx.x + 1] = xcc;
  }
}
}  // namespace cwt

static int debug_conv_s(cwt_ctx* ctx, int prec, const void* xs, int N, int Hi, int Wi, int Ci, const void* ws,
                        const float* scale, const float* shift, int Co, int k, int stride, int pad, int dil,
                        const float* res, int res_ld, const void* res_s, int relu, float* y, int y_ld, int y_off,
                        void* ys, int bm, int bn, int nsplit, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(xs && ws && scale && shift && (y || ys), "null buffer");
  const int kb = prec == 1 ? 64 : 32;
  CWT_CHECK(Ci % kb == 0 && Co % 64 == 0, prec == 1 ? "need Ci%64==0, Co%64==0" : "need Ci%32==0, Co%64==0");
  CWT_CHECK(!y || (y_ld >= y_off + Co && y_ld % 4 == 0 && y_off % 4 == 0), "bad y stride");
  ConvSArgs a = conv_s_geom(N, Hi, Wi, Ci, Co, k, stride, pad, dil);
  int rc;
  ConvPlan p = plan_conv_s(prec, a.M, a.Co, a.K);
  if (bm > 0 && (rc = force_conv_form(prec, bm, bn, Co, &p))) return rc;  // before any device call
  CWT_HIP(hipSetDevice(ctx->device));
  if ((rc = zero_line(ctx, &a.zero))) return rc;
  a.xs = (const __bf16*)xs;
  a.ws = (const __bf16*)ws;
  a.scale = scale;
  a.shift = shift;
  a.res = res;
  a.res_ld = res_ld;
  a.res_s = (const __bf16*)res_s;
  a.relu = relu;
  a.y = y;
  a.y_ld = y_ld;
  a.y_off = y_off;
  a.ys = (__bf16*)ys;
  if (nsplit > 0) {
    const int kt = a.K / kb;
    p.kt_per_split = cdiv(kt, nsplit);
    p.nsplit = cdiv(kt, p.kt_per_split);
  }
  if (prec == 6) {  // the fp32 packed weights -> the x6 kernel's hi | mid line and lo plane
    __bf16 *w3s, *w3l;  // hi | mid lines (2 per weight) and the lo plane
    if ((rc = cwt::ws(ctx, "dbg.w3s", (size_t)Co * a.K * 2, &w3s)) ||  // (cwt::ws: the parameter ws hides it)
        (rc = cwt::ws(ctx, "dbg.w3l", (size_t)Co * a.K, &w3l)))
      return rc;
    // CWT_DBG_W3_CACHE=1 (timing tools that call the same conv repeatedly): split the weights only when
    // the source buffer or its shape changes, so the timed calls are the conv alone
    static const bool w3_cache = getenv("CWT_DBG_W3_CACHE") && getenv("CWT_DBG_W3_CACHE")[0] == '1';
    static const void* w3_src = nullptr;
    static long w3_n = 0;
    static void* w3_dst = nullptr;
    if (!(w3_cache && w3_src == ws && w3_n == (long)Co * a.K && w3_dst == w3s)) {
      if ((rc = launch_split_w3((const float*)ws, Co, a.K, w3s, w3l, (hipStream_t)stream))) return rc;
      w3_src = ws;
      w3_n = (long)Co * a.K;
      w3_dst = w3s;
    }
    a.ws = w3s;
    a.ws_lo = w3l;
  }
  float* part = nullptr;
  const size_t pf = (size_t)p.nsplit * a.M * a.Co;
  if (p.nsplit > 1 && (rc = cwt::ws(ctx, "dbg.PART", pf, &part))) return rc;
  return launch_conv_x3s(a, p, 0, part, pf, (hipStream_t)stream, prec);
}

// A text export into the caller's buffer (NUL-terminated)
static int copy_text(const std::string& text, char* buf, int64_t cap) {
  CWT_CHECK(buf && (int64_t)text.size() + 1 <= cap, "text buffer too small");
  memcpy(buf, text.c_str(), text.size() + 1);
  return 0;
}

extern "C" {

int cwt_debug_conv(cwt_ctx* ctx, const float* x, int N, int Hi, int Wi, int Ci, int x_ld, const float* w_packed,
                   const float* scale, const float* shift, int Co, int k, int stride, int pad, int dil,
                   const float* res, int res_ld, int relu, float* y, int y_ld, int y_off, int bm, int bn,
                   int nsplit, int precision, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(x && w_packed && scale && shift && y, "null buffer");
  CWT_CHECK(Ci % 32 == 0 && Co % 64 == 0 && x_ld >= Ci && y_ld >= y_off + Co, "need Ci%32==0, Co%64==0");
  CWT_HIP(hipSetDevice(ctx->device));
  int rc;
  if (k > 1) {  // caller layout [Co][k][k][Ci] -> packed_k order
    float* wp;
    if ((rc = ws(ctx, "dbg.wpack", (size_t)Co * k * k * Ci, &wp))) return rc;
    if ((rc = launch_repack_cblock(w_packed, wp, Co, k * k, Ci, (hipStream_t)stream))) return rc;
    w_packed = wp;
  }
  ConvArgs a = conv_geom<ConvArgs>(N, Hi, Wi, Ci, Co, k, stride, pad, dil);
  a.x = x;
  a.x_ld = x_ld;
  a.w = w_packed;
  a.scale = scale;
  a.shift = shift;
  a.res = res;
  a.res_ld = res_ld;
  a.y = y;
  a.y_ld = y_ld;
  a.y_off = y_off;
  a.relu = relu;
  CWT_CHECK(precision == 0, "cwt_debug_conv runs the exact-fp32 conv only (bf16x3 plans: cwt_debug_conv_s)");
  ConvPlan p = plan_conv(a.M, a.Co, a.K);
  if (bm > 0) {
    CWT_CHECK((bm == 128 && (bn == 128 || bn == 64)) || (bm == 64 && bn == 64), "tile must be 128x128, 128x64 or 64x64");
    CWT_CHECK(Co % bn == 0, "Co % bn");
    p.bm = bm;
    p.bn = bn;
  }
  if (nsplit > 0) {
    const int kt = a.K / 32;
    p.kt_per_split = cdiv(kt, nsplit);
    p.nsplit = cdiv(kt, p.kt_per_split);
  }
  float* part = nullptr;
  size_t pf = (size_t)p.nsplit * a.M * a.Co;
  if (p.nsplit > 1 && (rc = ws(ctx, "dbg.PART", pf, &part))) return rc;
  return launch_conv(a, p, 0, part, pf, (hipStream_t)stream);
}

int cwt_debug_census(cwt_ctx* ctx, int nblocks, unsigned* out, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(out && nblocks > 0, "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(census_kernel, dim3(nblocks), dim3(64), 0, (hipStream_t)stream, out);
  CWT_LAUNCH_CHECK();
  return 0;
}

int cwt_debug_split_act(cwt_ctx* ctx, const float* x, int64_t P, int C, int ld, void* out, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(x && out && P >= 0 && C % 32 == 0 && ld >= C && ld % 4 == 0, "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  return launch_split_act(x, P, C, ld, (__bf16*)out, (hipStream_t)stream);
}

int cwt_debug_unsplit_act(cwt_ctx* ctx, const void* s, int64_t P, int C, float* out, int ld, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(s && out && P >= 0 && C % 32 == 0 && ld >= C && ld % 4 == 0, "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  return launch_unsplit_act((const __bf16*)s, P, C, out, ld, (hipStream_t)stream);
}

int cwt_debug_pack_wsplit(cwt_ctx* ctx, const float* w, int Co, int k, int Ci, void* out, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(w && out && Co > 0 && Ci % 32 == 0 && (k == 1 || k == 3), "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  float* wp;
  int rc;
  const long K = (long)k * k * Ci;
  if ((rc = ws(ctx, "dbg.wpack", (size_t)Co * K, &wp))) return rc;
  if ((rc = launch_repack_cblock(w, wp, Co, k * k, Ci, (hipStream_t)stream))) return rc;
  return launch_split_act(wp, Co, (int)K, (int)K, (__bf16*)out, (hipStream_t)stream);
}

// Single kernels of run_extract's glue on caller buffers (include/cwt_debug.h has the argument
// layouts): the launchers of the product path, their workspaces from the context.
int cwt_debug_backbone_op(cwt_ctx* ctx, int op, void* const* b, const int64_t* ia, const float* fa, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(b && ia, "null argument");
  CWT_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  auto lay_ok = [](int64_t l) { return l == ACT_F32 || l == ACT_SPLIT || l == ACT_BF16; };
  float* p;
  int rc;
  if (op == 0) {  // stem conv1: b = img w scale shift out; ia = N S layout relu
    const int N = (int)ia[0], S = (int)ia[1];
    CWT_CHECK(b[0] && b[1] && b[2] && b[3] && b[4] && N > 0 && S > 0 && lay_ok(ia[2]), "stem conv1");
    return launch_stem_conv1((const float*)b[0], N, S, (const float*)b[1], (const float*)b[2], (const float*)b[3],
                             (float*)b[4], down2(S), st, (int)ia[2], (int)ia[3]);
  }
  if (op == 1) {  // max pool: b = in out; ia = N H W C layout
    const int N = (int)ia[0], H = (int)ia[1], W = (int)ia[2], C = (int)ia[3], lay = (int)ia[4];
    CWT_CHECK(b[0] && b[1] && N > 0 && H > 0 && W > 0 && C > 0 && lay_ok(ia[4]), "maxpool");
    const int Ho = down2(H), Wo = down2(W);
    if (lay == ACT_BF16) return launch_maxpool3s2_b16((const __bf16*)b[0], N, H, W, C, (__bf16*)b[1], Ho, Wo, st);
    if (lay == ACT_SPLIT) return launch_maxpool3s2_s((const __bf16*)b[0], N, H, W, C, (__bf16*)b[1], Ho, Wo, st);
    CWT_CHECK(C % 4 == 0, "maxpool: C % 4");
    return launch_maxpool3s2((const float*)b[0], N, H, W, C, (float*)b[1], Ho, Wo, st);
  }
  if (op == 2) {  // PPM pooling: b = x pooled; ia = N h w ld layout
    const int N = (int)ia[0], h = (int)ia[1], w = (int)ia[2], ld = (int)ia[3];
    CWT_CHECK(b[0] && b[1] && N > 0 && h > 0 && w > 0 && ld >= 2048 && lay_ok(ia[4]), "ppm");
    // rowseg [N][h][nseg_x <= 16][2048] + blk [N][nseg_y <= 16][nseg_x <= 16][2048]
    if ((rc = ws(ctx, "dbg.ppm", ((size_t)N * h * 16 + (size_t)N * 256) * 2048, &p))) return rc;
    return launch_ppm((const float*)b[0], N, h, w, ld, kBins, 4, p, (float*)b[1], st, (int)ia[4]);
  }
  if (op == 3) {  // PPM GEMM: b = A Bt0..3 scale0..3 shift0..3 out; ia = M0..3 N K kchunk form
    int M[4];
    const float *Bt[4], *sc[4], *sh[4];
    long Mtot = 0;
    int nbn = 0;
    for (int q = 0; q < 4; ++q) {
      CWT_CHECK(ia[q] > 0 && ia[q] <= 4096 && b[1 + q], "ppm gemm: problem");
      M[q] = (int)ia[q];
      Mtot += M[q];
      Bt[q] = (const float*)b[1 + q];
      sc[q] = (const float*)b[5 + q];
      sh[q] = (const float*)b[9 + q];
      CWT_CHECK(!sc[q] == !sh[q], "ppm gemm: scale without shift");
      nbn += sc[q] != nullptr;
    }
    const int N = (int)ia[4], K = (int)ia[5], kc = (int)ia[6];
    int form = (int)ia[7];
    CWT_CHECK(b[0] && b[13] && N > 0 && K > 0 && (nbn == 0 || nbn == 4) && form <= 1, "ppm gemm");
    if (form < 0) form = Mtot <= kPpmGemmMaxRows ? 0 : 1;  // run_extract's rule
    CWT_CHECK(form == 0 || kc == 32 || kc == 64, "ppm gemm: K chunk");
    const size_t part_floats = (size_t)(form == 0 ? 8 : K / kc) * Mtot * N;
    if ((rc = ws(ctx, "dbg.parts", part_floats, &p))) return rc;
    return form == 0 ? launch_ppm_gemm((const float*)b[0], K, Bt, M, 4, N, K, nbn ? sc : nullptr, nbn ? sh : nullptr,
                                       p, part_floats, (float*)b[13], st)
                     : launch_smallm_gemm((const float*)b[0], K, Bt, M, 4, N, K, kc, p, part_floats,
                                          nbn ? sc : nullptr, nbn ? sh : nullptr, (float*)b[13], st);
  }
  if (op == 4) {  // training-mode BN: b = y res bn scale shift; ia = M C layout ld res_ld relu rows_per_image seed
    CWT_CHECK(fa && b[0] && b[2] && b[3] && b[4] && ia[0] > 0 && ia[1] > 0 && ia[1] <= 2048 && lay_ok(ia[2]) &&
                  ia[6] > 0,
              "bn_train");
    BnTrainArgs a;
    memset(&a, 0, sizeof(a));
    a.y = b[0];
    a.M = (long)ia[0];
    a.C = (int)ia[1];
    a.layout = (int)ia[2];
    a.ld = (int)ia[3];
    a.res = b[1];
    a.res_ld = (int)ia[4];
    a.relu = (int)ia[5];
    a.rows_per_image = (long)ia[6];
    a.seed = (unsigned long long)ia[7];
    a.bn = (float*)b[2];
    a.scale = (float*)b[3];
    a.shift = (float*)b[4];
    a.eps = fa[0];
    a.momentum = fa[1];
    a.drop_p = fa[2];
    CWT_CHECK(a.layout != ACT_F32 || a.ld >= a.C, "bn_train: ld < C");
    const size_t pf = bn_train_part_floats(a.M, a.C);
    float* bsc;
    if ((rc = ws(ctx, "dbg.bn.part", pf, &p)) || (rc = ws(ctx, "dbg.bn.bsc", 2 * 2048, &bsc))) return rc;
    return launch_bn_train(a, p, pf, bsc, st);
  }
  if (op == 5) {  // widen: b = in out; ia = count
    CWT_CHECK(b[0] && b[1] && ia[0] > 0, "widen");
    return launch_widen_bf16((const __bf16*)b[0], (long)ia[0], (float*)b[1], st);
  }
  return fail(CWT_EARG, "cwt_debug_backbone_op: unknown op");
}

int cwt_debug_conv_s(cwt_ctx* ctx, const void* xs, int N, int Hi, int Wi, int Ci, const void* ws, const float* scale,
                     const float* shift, int Co, int k, int stride, int pad, int dil, const float* res, int res_ld,
                     const void* res_s, int relu, float* y, int y_ld, int y_off, void* ys, int bm, int bn, int nsplit,
                     void* stream) {
  return debug_conv_s(ctx, 3, xs, N, Hi, Wi, Ci, ws, scale, shift, Co, k, stride, pad, dil, res, res_ld, res_s, relu, y,
                      y_ld, y_off, ys, bm, bn, nsplit, stream);
}

int cwt_debug_conv_f32d(cwt_ctx* ctx, const float* x, int N, int Hi, int Wi, int Ci, const float* w_packed,
                        const float* scale, const float* shift, int Co, int k, int stride, int pad, int dil,
                        const float* res, int res_ld, int relu, float* y, int y_ld, int y_off, int bm, int bn,
                        int nsplit, void* stream) {
  return debug_conv_s(ctx, 0, x, N, Hi, Wi, Ci, w_packed, scale, shift, Co, k, stride, pad, dil, res, res_ld, nullptr,
                      relu, y, y_ld, y_off, nullptr, bm, bn, nsplit, stream);
}

int cwt_debug_conv_x6(cwt_ctx* ctx, const float* x, int N, int Hi, int Wi, int Ci, const float* w_packed,
                      const float* scale, const float* shift, int Co, int k, int stride, int pad, int dil,
                      const float* res, int res_ld, int relu, float* y, int y_ld, int y_off, int bm, int bn,
                      int nsplit, void* stream) {
  return debug_conv_s(ctx, 6, x, N, Hi, Wi, Ci, w_packed, scale, shift, Co, k, stride, pad, dil, res, res_ld, nullptr,
                      relu, y, y_ld, y_off, nullptr, bm, bn, nsplit, stream);
}

int cwt_debug_conv_x6_dual(cwt_ctx* ctx, const float* t, int N, int Ho, int Wo, int K1, const float* x, int Hi2,
                           int Wi2, int K2, int stride2, const float* w3, const float* s3, const float* b3,
                           const float* wd, const float* sd, const float* bd, int Co, int relu, float* y, int bm,
                           int bn, int nsplit, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(t && x && w3 && s3 && b3 && wd && sd && bd && y, "null buffer");
  CWT_CHECK(N >= 1 && Ho >= 1 && Wo >= 1 && K1 > 0 && K2 > 0 && K1 % 32 == 0 && K2 % 32 == 0 && Co % 64 == 0,
            "need K1 % 32 == 0, K2 % 32 == 0, Co % 64 == 0");
  CWT_CHECK(stride2 >= 1 && (Ho - 1) * stride2 < Hi2 && (Wo - 1) * stride2 < Wi2, "second source too small");
  const int K = K1 + K2;
  ConvSArgs a = conv_s_geom(N, Ho, Wo, K1, Co, 1, 1, 0, 1);
  int rc;
  ConvPlan p = plan_conv_dual(a.M, Co, K);
  if (bm > 0 && (rc = force_conv_form(6, bm, bn, Co, &p))) return rc;  // before any device call
  if (nsplit > 0) {
    p.kt_per_split = cdiv(K / 32, nsplit);
    p.nsplit = cdiv(K / 32, p.kt_per_split);
  }
  CWT_HIP(hipSetDevice(ctx->device));
  const hipStream_t st = (hipStream_t)stream;
  float *wf, *shf, *ones, *part = nullptr;
  __bf16 *w3s, *w3l;
  if ((rc = zero_line(ctx, &a.zero)) || (rc = ws(ctx, "dbg.dual.w", (size_t)Co * K, &wf)) ||
      (rc = ws(ctx, "dbg.dual.sh", (size_t)Co, &shf)) || (rc = ws(ctx, "dbg.dual.ones", (size_t)Co, &ones)) ||
      (rc = ws(ctx, "dbg.dual.w3s", (size_t)Co * K * 2, &w3s)) || (rc = ws(ctx, "dbg.dual.w3l", (size_t)Co * K, &w3l)))
    return rc;
  // CWT_DBG_W3_CACHE=1 (timing tools): fold and split the weights only when their source or shape changes
  static const bool w3_cache = getenv("CWT_DBG_W3_CACHE") && getenv("CWT_DBG_W3_CACHE")[0] == '1';
  static const void* f_src = nullptr;
  static long f_n = 0;
  static void* f_dst = nullptr;
  if (!(w3_cache && f_src == w3 && f_n == (long)Co * K && f_dst == w3s)) {
    const std::vector<float> one(Co, 1.0f);
    CWT_HIP(hipMemcpyAsync(ones, one.data(), sizeof(float) * Co, hipMemcpyHostToDevice, st));
    CWT_HIP(hipStreamSynchronize(st));
    if ((rc = launch_fold_dual(w3, s3, b3, K1, wd, sd, bd, K2, Co, wf, shf, st)) ||
        (rc = launch_split_w3(wf, Co, K, w3s, w3l, st)))
      return rc;
    f_src = w3;
    f_n = (long)Co * K;
    f_dst = w3s;
  }
  a.K = K;
  a.xs = (const __bf16*)t;
  a.xs2 = (const __bf16*)x;
  a.Hi2 = Hi2;
  a.Wi2 = Wi2;
  a.Ci2 = K2;
  a.stride2 = stride2;
  a.kt_switch = K1 / 32;
  a.ws = w3s;
  a.ws_lo = w3l;
  a.scale = ones;
  a.shift = shf;
  a.relu = relu;
  a.y = y;
  a.y_ld = Co;
  const size_t pf = (size_t)p.nsplit * a.M * Co;
  if (p.nsplit > 1 && (rc = ws(ctx, "dbg.PART", pf, &part))) return rc;
  return launch_conv_x3s(a, p, 0, part, pf, st, 6);
}

int cwt_debug_wino_in(cwt_ctx* ctx, const float* x, int nsplit, const float* scale, const float* shift, int relu,
                      int N, int H, int W, int C, int d, int m, float* V, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(x && V && N >= 1 && H >= 1 && W >= 1 && C >= 4 && C % 4 == 0 && d >= 1 && (m == 2 || m == 4), "wino_in");
  CWT_CHECK(nsplit == 0 || (scale && shift && nsplit <= 64), "wino_in: split-K partials need scale and shift");
  CWT_HIP(hipSetDevice(ctx->device));
  const WinoGeom g = wino_geom(N, H, W, d, m);
  return nsplit > 0 ? launch_wino_in_splitk(x, nsplit, scale, shift, relu, g, C, V, (hipStream_t)stream)
                    : launch_wino_in(x, g, C, V, (hipStream_t)stream);
}

int cwt_debug_splitk_epilogue(cwt_ctx* ctx, const float* part, int nsplit, int M, int Co, const float* scale,
                              const float* shift, int relu, float* y, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_HIP(hipSetDevice(ctx->device));
  return launch_splitk_reduce_f32(part, nsplit, M, Co, scale, shift, relu, y, (hipStream_t)stream);
}

int cwt_debug_conv_form(int prec, int bm, int bn, int var, int* out4) {
  CWT_CHECK(out4, "out4 is NULL");
  const ConvForm* f = find_conv_form(prec, bm, bn, var);
  if (!f) return fail(CWT_EARG, "no such conv form (conv_forms.h)");
  out4[0] = f->waves_m;
  out4[1] = f->waves_n;
  out4[2] = f->nstg;
  out4[3] = f->pf;
  return 0;
}

int cwt_debug_conv_plan(int prec, int M, int Co, int K, int batch, int* out5) {
  CWT_CHECK(out5 && M > 0 && Co > 0 && K > 0 && batch >= 0, "bad arguments");
  CWT_CHECK(prec == 0 || prec == 1 || prec == 3 || prec == 6, "prec must be 0, 1, 3 or 6");
  const ConvPlan p = plan_conv_s(prec, M, Co, K, batch);
  const int v[5] = {p.bm, p.bn, p.var, p.nsplit, p.kt_per_split};
  std::copy(v, v + 5, out5);
  if (!find_conv_form(prec, p.bm, p.bn, p.var)) return fail(CWT_EARG, "the plan's form is no such conv form");
  return 0;
}

int cwt_debug_adapt_plan(int E, int n, int h, int w, int iters, int upw, int cu_count, int* out8) {
  CWT_CHECK(out8 && E >= 1 && n >= 1 && h >= 2 && w >= 2 && upw >= 0, "bad arguments");
  const AdaptPlan p = adapt_plan(E, n, h, w, iters, upw, cu_count, adapt_knobs_from_env());
  const int v[8] = {p.persist ? 1 : 0, p.form, p.G, p.units, p.ncb, p.uc, (int)p.k, (int)p.span};
  std::copy(v, v + 8, out8);
  return 0;
}

int cwt_debug_extract_plan(int layers, int N, int S, int precision, int conv_arith, int train_bn, int want_mid, char* buf,
                           int64_t cap) {
  CWT_CHECK(layers == 50 || layers == 101, "layers must be 50 or 101");
  CWT_CHECK(N >= 1 && S >= 9 && (S - 1) % 8 == 0, "need N >= 1 and (S-1) % 8 == 0");
  const ExtractKnobs kn = extract_knobs_from_env();
  const std::vector<ConvSpec> arch = backbone_arch(layers);
  const ExtractPlan p = extract_plan(arch, extractor_forms(arch, kn.wino4_at_load), N, S,
                                     extract_mode(precision, conv_arith, train_bn != 0, kn), kn,
                                     extract_last_blocks(arch, want_mid ? 7 : 0),
                                     train_bn != 0);
  if (p.error) return fail(CWT_ESTATE, p.error);
  std::string out;
  char num[64];
  for_each_record(p, [&](const ExtractRec& r) {
    snprintf(num, sizeof(num), "\t%.17g\t%.17g\n", r.flops, r.bytes);
    out += std::to_string(r.level) + "\t" + r.name + num;
  });
  const ExtractSizes& z = p.ws;
  const std::pair<const char*, size_t> sizes[] = {
      {"bb.A", z.A}, {"bb.B", z.A}, {"bb.T1", z.T1}, {"bb.T2", z.T2}, {"bb.D", z.D}, {"bb.COL", z.COL},
      {"bb.POOL", z.POOL}, {"bb.PPM", z.PPM}, {"bb.Q", z.Q}, {"bb.R", z.R}, {"bb.F", z.F}, {"bb.PARTS", z.PARTS},
      {"bb.PART", z.PART}, {"bn.part", z.bn_part}, {"wino.V", z.wino_V}, {"wino.M", z.wino_M}};
  for (const auto& s : sizes) out += std::string("ws\t") + s.first + "\t" + std::to_string(s.second) + "\n";
  for (const ExtractStep& s : p.steps)  // the one choice of form no record names
    if (s.kind == XS_PPM_CONV) out += std::string("form\tppm_gemm\t") + (s.few_cells ? "few_rows" : "splitk") + "\n";
  return copy_text(out, buf, cap);
}

int cwt_debug_extract_mode(int mode, int* out5) {
  CWT_CHECK(out5, "out5 is NULL");
  if (mode < 0 || mode >= EM_NMODES) return fail(CWT_EARG, "no such extractor mode (extract_plan.h)");
  const ExtractModeTraits t = extract_mode_traits(mode);
  const int v[5] = {t.layout, t.prec, t.dma, t.out_f32, (int)t.elem_bytes};
  std::copy(v, v + 5, out5);
  return 0;
}

int cwt_debug_backbone_arch(int layers, char* buf, int64_t cap) {
  CWT_CHECK(layers == 50 || layers == 101, "layers must be 50 or 101");
  std::string out;
  for (const ConvSpec& s : backbone_arch(layers))
    out += s.wname + "\t" + s.bnp + "\t" + std::to_string(s.Ci) + "\t" + std::to_string(s.Co) + "\t" +
           std::to_string(s.k) + "\t" + std::to_string(s.stride) + "\t" + std::to_string(s.pad) + "\t" +
           std::to_string(s.dil) + "\n";
  return copy_text(out, buf, cap);
}

int cwt_debug_adapt_form(int form, int* out6) {
  CWT_CHECK(out6, "out6 is NULL");
  if (form < 0 || form >= PA_NFORMS) return fail(CWT_EARG, "no such inner-loop form (adapt_plan.h)");
  const PaFormTraits t = pa_form_traits(form);
  const int v[6] = {t.nu, t.ewk, t.lock, t.breg, t.stream, t.res1};
  std::copy(v, v + 6, out6);
  return 0;
}

int cwt_debug_cp4d_plan(int dir, int B, int hA, int wA, int hB, int wB, int cin, int cout, int variant, int cu, int occ,
                        int* out16) {
  CWT_CHECK(out16 && dir >= 0 && dir <= 2 && B >= 1 && hA >= 1 && wA >= 1 && hB >= 1 && wB >= 1, "bad arguments");
  const auto plan = dir == 0 ? cp4d_plan_fwd : dir == 1 ? cp4d_plan_dgrad : cp4d_plan_wgrad;
  const Cp4dPlan p = plan(B, hA, wA, hB, wB, cin, cout, variant, cp4d_env(), cu, occ);
  const int v[16] = {p.rc, p.form, p.cin, p.cout, p.mode, p.pf, p.gx,    p.gy,
                     p.gz, p.wc,   p.nsa, p.ntiles, p.order, p.dbg, p.G, p.n};
  std::copy(v, v + 16, out16);
  return p.rc ? fail(p.rc, p.msg) : 0;
}

int cwt_debug_cp4d_form(int form, char* buf, int64_t cap) {
  const Cp4dFormInfo f = cp4d_form_info(form);
  if (!f.name) return fail(CWT_EARG, "no such consensus-layer form (cp4d_plan.h)");
  return copy_text(std::string(f.name) + "\t" + f.kernel + "\t" + f.targs, buf, cap);
}

int cwt_debug_cp4d_wgrad_part_floats(void) { return cp4d_wgrad_part_floats(); }

int cwt_debug_match_plan(int dir, int B, int L, int h, int w, int symmetric, int cv4, int train, int readout,
                         int want_d_corr, int want_d_v, char* buf, int64_t cap) {
  CWT_CHECK(dir == 0 || dir == 1, "dir must be 0 (forward) or 1 (backward)");
  const auto S = [](long v) { return std::to_string(v); };
  std::string out;
  const auto params = [&](const MatchParams& T, bool cv, int branches) {
    static const char* const names[2][4] = {{"conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias"},
                                            {"weight", "bias", "", ""}};
    for (int l = 0; l < 3; ++l)
      for (int s = 0; s < (cv ? 1 : 2); ++s) {
        out += "param\t" + S(l) + "\t" + names[cv][2 * s] + "\t" + S(T.W[l][s]) + "\t" + S(T.nW[l]) + "\n";
        out += "param\t" + S(l) + "\t" + names[cv][2 * s + 1] + "\t" + S(T.b[l][s]) + "\t" + S(T.nb[l]) + "\n";
      }
    out += "param\ttotal\t" + S(T.total) + "\n";
    for (int br = 0; br < (cv ? 0 : branches); ++br)
      for (int l = 0; l < 3; ++l)
        out += "role\t" + S(br) + "\t" + S(l) + "\t" + S(T.Wa(l, br)) + "\t" + S(T.ba(l, br)) + "\t" + S(T.Wb(l, br)) +
               "\t" + S(T.bb(l, br)) + "\n";
  };
  const auto one = [&](const std::string& name, const MatchBuf& b) {
    if (b.floats)
      out += "buf\t" + name + "\t" + (b.ws ? b.ws : "saved") + "\t" + S(b.off) + "\t" + S(b.floats) + "\t" +
             (b.per_cv ? "Cv" : "1") + "\n";
  };
  if (dir == 0) {
    const MatchPlan p = match_plan(B, L, h, w, symmetric != 0, cv4 != 0, train != 0, readout != 0, match_env());
    CWT_CHECK(!p.rc, p.msg);
    static const char* const mm1[] = {"direct", "planar2", "clast"};
    static const char* const mm2[] = {"plain", "add", "sum"};
    out += std::string("plan\tfwd\tmm1=") + mm1[p.mm1] + "\tlayers=" + (p.cv4 ? "cv4d" : "cp4d") + "\tbranches=" +
           S(p.branches) + "\tfork=" + S(p.fork) + "\tmm2=" + mm2[p.mm2] + "\treadout=" + S(p.readout) + "\ttrain=" +
           S(p.train) + "\n";
    params(p.params, p.cv4, p.branches);
    one("x0", p.x0);
    for (int br = 0; br < 2; ++br)
      for (int l = 0; l < 3; ++l) one("o" + S(br) + S(l), p.o[br][l]);
    one("y", p.y), one("attn", p.attn), one("vt", p.vt);
    if (p.train)
      out += "saved\ttotal\t" + S(match_saved_layout(B, L, (long)h * w, symmetric != 0, readout != 0).total) + "\n";
  } else {
    const MatchBwdPlan p = match_bwd_plan(B, L, h, w, symmetric != 0, want_d_corr != 0, want_d_v != 0, readout != 0);
    CWT_CHECK(!p.rc, p.msg);
    out += "plan\tbwd\tbranches=" + S(p.branches) + "\td_corr=" + S(p.d_corr) + "\td_v=" + S(p.d_v) + "\treadout=" +
           S(p.readout) + "\tclast=" + S(p.clast) + "\n";
    params(p.params, false, p.branches);
    const long E = (long)B * h * w * h * w;
    const MatchSavedLayout& s = p.saved;
    one("x0", match_in_saved(s.x0, E * L));
    for (int br = 0; br < p.branches; ++br)
      for (int l = 0; l < 3; ++l) one("o" + S(br) + S(l), match_in_saved(s.o[br][l], E * match_ch(L, l + 1)));
    one("y", match_in_saved(s.y, E));
    if (s.attn >= 0) one("attn", match_in_saved(s.attn, s.total - s.attn));
    one("g2d", p.g2d), one("dy", p.dy), one("gA", p.gA), one("gm", p.gm), one("dx0", p.dx0), one("part", p.part);
    one("xcl", p.xcl), one("dxcl", p.dxcl);
    out += "saved\ttotal\t" + S(s.total) + "\n";
  }
  return copy_text(out, buf, cap);
}

int cwt_debug_conv_x6w(cwt_ctx* ctx, const float* x, int N, int Hi, int Wi, int Ci, const float* w_packed,
                       const float* scale, const float* shift, int Co, int k, int stride, int pad, int dil,
                       const float* res, int res_ld, int relu, float* y, int y_ld, int y_off, int bm, int bn,
                       int nsplit, void* stream) {
  const int m = nsplit == 4 ? 4 : 2;  // nsplit selects the output tile: 4 = F(4x4,3x3), else F(2x2,3x3)
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(x && w_packed && scale && shift && y, "null buffer");
  CWT_CHECK(nsplit == 0 || nsplit == 1 || nsplit == 2 || nsplit == 4, "nsplit (the Winograd tile) must be 0, 2 or 4");
  CWT_CHECK(k == 3 && stride == 1 && pad == dil && dil >= 1, "winograd form: 3x3, stride 1, padding = dilation");
  CWT_CHECK(Ci % 32 == 0 && Co % 64 == 0 && N >= 1 && Hi >= 1 && Wi >= 1, "need Ci % 32 == 0, Co % 64 == 0");
  CWT_CHECK(y_ld >= y_off + Co && y_ld % 4 == 0 && y_off % 4 == 0 && (!res || res_ld % 4 == 0), "bad strides");
  int rc;
  // the form's plan, its GEMMs' tile forced where one is named: refused here, before any device call
  WinoPlan wp = wino_plan(N, Hi, Wi, Ci, Co, dil, m, 0, 0, res != nullptr, ctx->prof_level > 0);
  if (bm > 0 && (rc = force_conv_form(6, bm, bn, Co, &wp.gemm))) return rc;
  CWT_HIP(hipSetDevice(ctx->device));
  const hipStream_t st = (hipStream_t)stream;
  const int P = (m + 2) * (m + 2);
  const size_t n = (size_t)P * Co * Ci;
  float* U;
  __bf16 *us, *ul;  // split like ConvLayer's wino_s / wino_l
  if ((rc = ws(ctx, "dbg.wU", n, &U)) || (rc = ws(ctx, "dbg.wUs", n * 2, &us)) || (rc = ws(ctx, "dbg.wUl", n, &ul)))
    return rc;
  // CWT_DBG_W3_CACHE=1: transform and split the weights only when their source or shape changes
  static const bool w3_cache = getenv("CWT_DBG_W3_CACHE") && getenv("CWT_DBG_W3_CACHE")[0] == '1';
  static const void* u_src = nullptr;
  static long u_n = 0;
  static void* u_dst = nullptr;
  if (!(w3_cache && u_src == w_packed && u_n == (long)n * m && u_dst == us)) {
    if ((rc = launch_wino_weights(w_packed, Co, Ci, U, st, m)) ||
        (rc = launch_split_w3(U, (long)P * Co, Ci, us, ul, st)))
      return rc;
    u_src = w_packed;
    u_n = (long)n * m;
    u_dst = us;
  }
  return run_wino_conv(ctx, x, Ci, Co, wp, us, ul, scale, shift, res, res_ld, relu, y, y_ld, y_off, st);
}

int cwt_debug_conv_b16(cwt_ctx* ctx, const void* xs, int N, int Hi, int Wi, int Ci, const void* ws, const float* scale,
                       const float* shift, int Co, int k, int stride, int pad, int dil, const float* res, int res_ld,
                       const void* res_s, int relu, float* y, int y_ld, int y_off, void* ys, int bm, int bn,
                       int nsplit, void* stream) {
  return debug_conv_s(ctx, 1, xs, N, Hi, Wi, Ci, ws, scale, shift, Co, k, stride, pad, dil, res, res_ld, res_s, relu, y,
                      y_ld, y_off, ys, bm, bn, nsplit, stream);
}

// one CenterPivotConv4d layer (+ ReLU) on [B][NA][NB][cin] -> [B][NA][NB][cout] (launch_cp4d_layer);
// variant 0 the automatic kernel choice, 1 never the rolling-window form, 2 only it, 3 the
// channel-chunked form (cout 10)
int cwt_debug_cp4d_layer(cwt_ctx* ctx, const float* x, int B, int hA, int wA, int hB, int wB, int cin, int cout,
                         const float* Wa, const float* ba, const float* Wb, const float* bb, float* y, int variant,
                         void* stream) {
  if (!ctx || !x || !Wa || !ba || !Wb || !bb || !y) return fail(CWT_EARG, "null argument");
  if (B < 1 || hA < 1 || wA < 1 || hB < 1 || wB < 1) return fail(CWT_EARG, "bad shape");
  return launch_cp4d_layer_variant(x, B, hA, wA, hB, wB, cin, cout, Wa, ba, Wb, bb, y, variant, (hipStream_t)stream);
}

// the layer's input gradient dx [B][NA][NB][gout] (+)= from g [B][NA][NB][gin] (launch_cp4d_dgrad); variant as above
int cwt_debug_cp4d_dgrad(cwt_ctx* ctx, const float* g, int B, int hA, int wA, int hB, int wB, int gin, int gout,
                         const float* Wa, const float* Wb, float* dx, int accum, int variant, void* stream) {
  if (!ctx || !g || !Wa || !Wb || !dx) return fail(CWT_EARG, "null argument");
  if (B < 1 || hA < 1 || wA < 1 || hB < 1 || wB < 1) return fail(CWT_EARG, "bad shape");
  return launch_cp4d_dgrad(g, B, hA, wA, hB, wB, gin, gout, Wa, Wb, dx, accum, (hipStream_t)stream, variant);
}

// the layer's weight and bias gradients, added into dWa / dWb [cout][cin][3][3] and db1 / db2 [cout]
// (launch_cp4d_wgrad: the form cp4d_plan_wgrad names under the environment at this call)
int cwt_debug_cp4d_wgrad(cwt_ctx* ctx, const float* x, const float* gm, int B, int hA, int wA, int hB, int wB, int cin,
                         int cout, float* dWa, float* dWb, float* db1, float* db2, void* stream) {
  if (!ctx || !x || !gm || !dWa || !dWb || !db1 || !db2) return fail(CWT_EARG, "null argument");
  if (B < 1 || hA < 1 || wA < 1 || hB < 1 || wB < 1) return fail(CWT_EARG, "bad shape");
  CWT_HIP(hipSetDevice(ctx->device));
  float* part;
  int rc;
  if ((rc = ws(ctx, "mb.part", (size_t)cp4d_wgrad_part_floats(), &part))) return rc;
  return launch_cp4d_wgrad(x, gm, B, hA, wA, hB, wB, cin, cout, part, (size_t)cp4d_wgrad_part_floats(), dWa, dWb, db1,
                           db2, (hipStream_t)stream);
}

// MutualMatching's backward alone: dx [B][NA][NB][C] from x and dy of that shape (launch_mutual_matching_bwd)
int cwt_debug_mutual_matching_bwd(cwt_ctx* ctx, const float* x, const float* dy, int B, int NA, int NB, int C,
                                  float* dx, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(x && dy && dx && B >= 1 && NA >= 1 && NB >= 1 && C >= 1 && C <= 64, "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  MmBwdWs mw;
  int rc;
  if ((rc = mm_bwd_ws(ctx, B, NA, NB, C, &mw))) return rc;
  return launch_mutual_matching_bwd(x, dy, B, NA, NB, C, dx, mw, (hipStream_t)stream);
}

int cwt_debug_occupy(cwt_ctx* ctx, int nwg, int us, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(nwg >= 1 && nwg <= 256 && us >= 1 && us <= 100000, "occupy: 1 <= nwg <= 256, 1 <= us <= 100000");
  CWT_HIP(hipSetDevice(ctx->device));
  return launch_occupy(nwg, us, (hipStream_t)stream);
}

int cwt_debug_tail_stamps(cwt_ctx* ctx, unsigned long long* host_out, int64_t max_count, int64_t* count) {
  if (!ctx || !count) return fail(CWT_EARG, "null argument");
  CWT_HIP(hipSetDevice(ctx->device));
  auto it = ctx->ws.find("tail.stamps");
  *count = (it == ctx->ws.end() || !ctx->tail_stamp_G) ? 0 : (int64_t)ctx->tail_stamp_G * 16;
  if (host_out && *count > 0 && max_count > 0) {
    CWT_HIP(hipDeviceSynchronize());
    CWT_HIP(hipMemcpy(host_out, it->second.p, (size_t)std::min<int64_t>(max_count, *count) * 8, hipMemcpyDeviceToHost));
  }
  return 0;
}

int cwt_debug_adapt_stamps(cwt_ctx* ctx, unsigned long long* host_out, int64_t max_count, int64_t* count) {
  if (!ctx || !count) return fail(CWT_EARG, "null argument");
  CWT_HIP(hipSetDevice(ctx->device));
  *count = g_adapt_stamps ? g_adapt_stamps_n : 0;
  if (host_out && g_adapt_stamps && max_count > 0) {
    CWT_HIP(hipDeviceSynchronize());
    CWT_HIP(hipMemcpy(host_out, g_adapt_stamps, (size_t)std::min<int64_t>(max_count, g_adapt_stamps_n) * 8,
                      hipMemcpyDeviceToHost));
  }
  return 0;
}

int cwt_debug_adapt_spin_limit(cwt_ctx* ctx, int64_t limit) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(limit >= 0, "limit must be >= 0");
  ctx->adapt_spin_limit = (long)limit;
  return 0;
}

}  // extern "C"
