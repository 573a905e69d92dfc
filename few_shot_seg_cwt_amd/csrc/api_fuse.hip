// The fusion trainer's entry points of libcwt.so (include/cwt.h): FuseNet1's 4-D stack, the support
// mask, the mask's fold into the attention net's bias, the softmax, the blend and the loss head
// (kernels: fuse.hip).  Every entry checks its arguments before it looks at the context, so a refusal needs
// no device.
#include "ctx.h"
#include "fuse.h"

using namespace cwt;

static int fuse_stack_args(const void* corr, int B, int hA, int wA, int hB, int wB, const float* const* w,
                           const void* X, int64_t ldx, int col) {
  CWT_CHECK(corr && X, "corr / X is NULL");
  for (int i = 0; i < 8; ++i) CWT_CHECK(w[i], "a FuseNet1 parameter is NULL");
  CWT_CHECK(B >= 1 && B <= 64, "B must lie in [1, 64]");
  CWT_CHECK(hA >= 2 && wA >= 2 && hB >= 2 && wB >= 2 && hA <= 512 && wA <= 512 && hB <= 512 && wB <= 512,
            "sides must lie in [2, 512]");
  const FuseGeom g = fuse_geom(B, hA, wA, hB, wB);
  CWT_CHECK(col >= 0 && ldx >= (int64_t)col + g.NB2(), "ldx too small for col + ceil(hB/2) ceil(wB/2) columns");
  CWT_CHECK(g.units() <= (1L << 30) && (long)B * g.NA() * ldx <= (1L << 40), "tensor too large");
  return 0;
}

extern "C" {

int64_t cwt_fuse_stack_saved_floats(int B, int hA, int wA, int hB, int wB) {
  if (B < 1 || hA < 2 || wA < 2 || hB < 2 || wB < 2) return 0;
  return (int64_t)fuse_geom(B, hA, wA, hB, wB).units() * FUSE_C;
}

int cwt_fuse_stack(cwt_ctx* ctx, const float* corr, int B, int hA, int wA, int hB, int wB, const float* w1a,
                   const float* b1a, const float* w1b, const float* b1b, const float* w2a, const float* b2a,
                   const float* w2b, const float* b2b, float* y1_saved, float* X, int64_t ldx, int col, void* stream) {
  const float* w[8] = {w1a, b1a, w1b, b1b, w2a, b2a, w2b, b2b};
  int rc;
  if ((rc = fuse_stack_args(corr, B, hA, wA, hB, wB, w, X, ldx, col))) return rc;
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const FuseGeom g = fuse_geom(B, hA, wA, hB, wB);
  const double u = (double)g.units();
  Prof p(ctx, st, y1_saved ? "fuse_stack_train" : "fuse_stack", 2.0 * u * (y1_saved ? 1 : 17) * FUSE_C * 18 + 2.0 * u * 18 * FUSE_C,
         4.0 * ((double)B * g.NA() * g.NB() + u * (y1_saved ? 2 * FUSE_C + 1 : 1)));
  rc = launch_fuse_stack(corr, g, FuseParams{w1a, b1a, w1b, b1b, w2a, b2a, w2b, b2b}, y1_saved, X, (long)ldx, col, st);
  p.end();
  return rc;
}

int cwt_fuse_stack_backward(cwt_ctx* ctx, const float* corr, int B, int hA, int wA, int hB, int wB, const float* w2a,
                            const float* w2b, const float* y1_saved, const float* X, const float* d_X, int64_t ldx,
                            int col, int accumulate, float* d_w1a, float* d_b1a, float* d_w1b, float* d_b1b,
                            float* d_w2a, float* d_b2a, float* d_w2b, float* d_b2b, void* stream) {
  const float* w[8] = {d_w1a, d_b1a, d_w1b, d_b1b, d_w2a, d_b2a, d_w2b, d_b2b};
  int rc;
  if ((rc = fuse_stack_args(corr, B, hA, wA, hB, wB, w, X, ldx, col))) return rc;
  CWT_CHECK(w2a && w2b && y1_saved && d_X, "w2a / w2b / y1_saved / d_X is NULL");
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const FuseGeom g = fuse_geom(B, hA, wA, hB, wB);
  double* part;
  if ((rc = ws(ctx, "fuse.part", fuse_bwd_part_doubles(g), &part))) return rc;
  const double u = (double)g.units();
  Prof p(ctx, st, "fuse_stack_backward", 2.0 * u * FUSE_C * 54, 4.0 * ((double)B * g.NA() * g.NB() + u * (FUSE_C + 2)));
  rc = launch_fuse_stack_bwd(corr, g, FuseParams{nullptr, nullptr, nullptr, nullptr, w2a, nullptr, w2b, nullptr},
                             y1_saved, X, d_X, (long)ldx, col, accumulate,
                             FuseGrads{d_w1a, d_b1a, d_w1b, d_b1b, d_w2a, d_b2a, d_w2b, d_b2b}, part, st);
  p.end();
  return rc;
}

int cwt_fuse_support_mask(cwt_ctx* ctx, const int64_t* label, int H, int W, int m, int align_corners, int pool,
                          float* s_mask, void* stream) {
  CWT_CHECK(label && s_mask, "label / s_mask is NULL");
  CWT_CHECK(H >= 2 && W >= 2 && H <= 16384 && W <= 16384 && m >= 1 && m <= 1024, "H, W in [2, 16384], m in [1, 1024]");
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_HIP(hipSetDevice(ctx->device));
  return launch_fuse_support_mask(label, H, W, m, align_corners != 0, pool != 0, s_mask, (hipStream_t)stream);
}

int cwt_fuse_mask_bias(cwt_ctx* ctx, const float* W, int64_t ldw, int col, const float* s_mask, int n, const float* b,
                       int mid, float* b_eff, void* stream) {
  CWT_CHECK(W && s_mask && b && b_eff, "W / s_mask / b / b_eff is NULL");
  CWT_CHECK(mid >= 1 && n >= 1 && col >= 0 && ldw >= (int64_t)col + n, "ldw too small for col + n columns");
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_HIP(hipSetDevice(ctx->device));
  return launch_fuse_mask_bias(W, (long)ldw, col, s_mask, n, b, mid, b_eff, (hipStream_t)stream);
}

int cwt_fuse_mask_bias_backward(cwt_ctx* ctx, const float* d_b, const float* s_mask, int mid, int n, float* d_W,
                                int64_t ldw, int col, void* stream) {
  CWT_CHECK(d_b && s_mask && d_W, "d_b / s_mask / d_W is NULL");
  CWT_CHECK(mid >= 1 && n >= 1 && col >= 0 && ldw >= (int64_t)col + n, "ldw too small for col + n columns");
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_HIP(hipSetDevice(ctx->device));
  return launch_fuse_mask_bias_bwd(d_b, s_mask, mid, n, d_W, (long)ldw, col, (hipStream_t)stream);
}

int cwt_fuse_softmax2(cwt_ctx* ctx, const float* z, int B, int64_t P, float* wt, void* stream) {
  CWT_CHECK(z && wt && B >= 1 && P >= 1 && (long)B * P <= (1L << 30), "bad arguments");
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_HIP(hipSetDevice(ctx->device));
  return launch_fuse_softmax2(z, B, (long)P, wt, (hipStream_t)stream);
}

int cwt_fuse_softmax2_backward(cwt_ctx* ctx, const float* wt, const float* d_wt, int B, int64_t P, float* d_z,
                               void* stream) {
  CWT_CHECK(wt && d_wt && d_z && B >= 1 && P >= 1 && (long)B * P <= (1L << 30), "bad arguments");
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_HIP(hipSetDevice(ctx->device));
  return launch_fuse_softmax2_bwd(wt, d_wt, B, (long)P, d_z, (hipStream_t)stream);
}

int cwt_fuse_blend(cwt_ctx* ctx, const float* wv, const float* f_q, const float* wt, int B, int64_t P, int C,
                   float* out, void* stream) {
  CWT_CHECK(wv && f_q && wt && out && B >= 1 && P >= 1 && C >= 1 && (long)B * P <= (1L << 30), "bad arguments");
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_HIP(hipSetDevice(ctx->device));
  return launch_fuse_blend(wv, f_q, wt, B, (long)P, C, out, (hipStream_t)stream);
}

int cwt_fuse_blend_backward(cwt_ctx* ctx, const float* wv, const float* f_q, const float* d_out, int B, int64_t P,
                            int C, float* d_wt, void* stream) {
  CWT_CHECK(wv && f_q && d_out && d_wt && B >= 1 && P >= 1 && C >= 1 && (long)B * P <= (1L << 30), "bad arguments");
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_HIP(hipSetDevice(ctx->device));
  return launch_fuse_blend_bwd(wv, f_q, d_out, B, (long)P, C, d_wt, (hipStream_t)stream);
}

int cwt_fuse_loss_head(cwt_ctx* ctx, const float* pd_q, const float* pd_q0, const float* pd_q1, int h, int w,
                       const int64_t* label, int S, float* loss_out, float* d_pd_q, float* iut_out,
                       float* disagree_out, void* stream) {
  CWT_CHECK(pd_q && pd_q0 && pd_q1 && label && loss_out && iut_out && disagree_out, "a pointer is NULL");
  CWT_CHECK(h >= 2 && w >= 2 && h <= 4096 && w <= 4096 && S >= 2 && S <= 16384, "h, w in [2, 4096], S in [2, 16384]");
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  double *part, *sc;
  unsigned* counts;
  int rc;
  if ((rc = ws(ctx, "fuse.loss.part", fuse_loss_part_doubles(), &part)) ||
      (rc = ws(ctx, "fuse.loss.counts", fuse_loss_count_words(), &counts)) || (rc = ws(ctx, "fuse.loss.sc", 2, &sc)))
    return rc;
  Prof p(ctx, st, "fuse_loss_head", 60.0 * S * S, 8.0 * S * S);
  rc = launch_fuse_loss_head(pd_q, pd_q0, pd_q1, h, w, label, S, loss_out, d_pd_q, iut_out, disagree_out, part, counts,
                             sc, st);
  p.end();
  return rc;
}

}  // extern "C"
