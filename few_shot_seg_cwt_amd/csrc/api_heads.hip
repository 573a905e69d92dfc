// WeightAverage, the MMN blend and DeTr entry points of libcwt.so (include/cwt.h), forward and
// backward (MatchNet's own entry points: api_match.hip).
#include "ctx.h"

using namespace cwt;

extern "C" {

static bool wa_channels_ok(int C) { return (C >= 64 && C <= 512 && C % 64 == 0) || C == 1024 || C == 2048; }

static int weight_average(cwt_ctx* ctx, const float* x, int N, int h, int w, int C, const float* w_tpg,
                          const float* b_theta, const float* b_phi, const float* b_g, const float* w_back,
                          const float* b_back, float* out, void* stream, float* tpg_keep, float* wavg_keep,
                          float p_att = 0.f, float p_proj = 0.f, unsigned long long seed = 0) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(x && w_tpg && b_theta && b_phi && b_g && w_back && b_back && out && N >= 1 && h >= 1 && w >= 1,
            "bad arguments");
  CWT_CHECK(wa_channels_ok(C), "WeightAverage: c_in a multiple of 64 up to 512, or 1024 or 2048");
  CWT_CHECK(p_att >= 0.f && p_att < 1.f && p_proj >= 0.f && p_proj < 1.f, "dropout probabilities must lie in [0, 1)");
  CWT_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const int co = C / 2;
  const long P = (long)N * h * w;
  float *tpg, *wavg, *back;
  int rc;
  if ((rc = ws(ctx, "wa.tpg", (size_t)P * 3 * co, &tpg)) || (rc = ws(ctx, "wa.avg", (size_t)P * co, &wavg)) ||
      (rc = ws(ctx, "wa.back", (size_t)P * C, &back)))
    return rc;
  if (tpg_keep) tpg = tpg_keep;
  if (wavg_keep) wavg = wavg_keep;
  Prof p(ctx, st, "weight_average c" + std::to_string(C), 2.0 * P * C * co * 4, 4.0 * P * (2.0 * C + 5.0 * co));
  // theta | phi | g of every pixel: one GEMM against the three stacked 1x1 weights [3co][C]
  const bool wa_f32d = gemm_f32d_mode() != 0;
  if (wa_f32d && gemm_f32d_ok((int)P, 3 * co, C, x, w_tpg, tpg, nullptr)) {
    if ((rc = gemm_f32d(ctx, x, w_tpg, (int)P, 3 * co, C, tpg, nullptr, nullptr, 0, st))) return rc;
  } else if ((rc = launch_gemm_abt(x, w_tpg, 1, (int)P, 3 * co, C, tpg, st))) {
    return rc;
  }
  if ((rc = launch_wa_attn(tpg, N, h, w, co, b_theta, b_phi, b_g, wavg, st, p_att, seed))) return rc;
  // conv_back + bias + residual in one epilogue (not under proj_drop: the mask goes between them)
  if (p_proj == 0.f && wa_f32d && gemm_f32d_ok((int)P, C, co, wavg, w_back, out, x)) {
    if ((rc = gemm_f32d(ctx, wavg, w_back, (int)P, C, co, out, b_back, x, C, st))) return rc;
  } else {
    if ((rc = launch_gemm_abt(wavg, w_back, 1, (int)P, C, co, back, st))) return rc;
    if ((rc = launch_wa_residual(x, back, b_back, P * C, C, out, st, p_proj, seed))) return rc;
  }
  p.end();
  return 0;
}

int cwt_weight_average(cwt_ctx* ctx, const float* x, int N, int h, int w, int C, const float* w_tpg,
                       const float* b_theta, const float* b_phi, const float* b_g, const float* w_back,
                       const float* b_back, float* out, void* stream) {
  return weight_average(ctx, x, N, h, w, C, w_tpg, b_theta, b_phi, b_g, w_back, b_back, out, stream, nullptr, nullptr);
}

int cwt_weight_average_train(cwt_ctx* ctx, const float* x, int N, int h, int w, int C, const float* w_tpg,
                             const float* b_theta, const float* b_phi, const float* b_g, const float* w_back,
                             const float* b_back, float* out, float* tpg, float* wavg, void* stream) {
  if (!tpg || !wavg) return fail(CWT_EARG, "tpg / wavg is NULL");
  return weight_average(ctx, x, N, h, w, C, w_tpg, b_theta, b_phi, b_g, w_back, b_back, out, stream, tpg, wavg);
}

int cwt_weight_average_train_drop(cwt_ctx* ctx, const float* x, int N, int h, int w, int C, const float* w_tpg,
                                  const float* b_theta, const float* b_phi, const float* b_g, const float* w_back,
                                  const float* b_back, float* out, float* tpg, float* wavg, float p_att,
                                  float p_proj, uint64_t seed, void* stream) {
  if (!tpg || !wavg) return fail(CWT_EARG, "tpg / wavg is NULL");
  return weight_average(ctx, x, N, h, w, C, w_tpg, b_theta, b_phi, b_g, w_back, b_back, out, stream, tpg, wavg, p_att,
                        p_proj, (unsigned long long)seed);
}

// d_res: the gradient at the output (the residual's share of d_x); d_out: the gradient at
// conv_back's output (d_res times the proj_drop mask, or d_res itself)
static int weight_average_backward(cwt_ctx* ctx, const float* x, int N, int h, int w, int C, const float* w_tpg,
                                   const float* b_theta, const float* b_phi, const float* b_g, const float* w_back,
                                   const float* tpg, const float* wavg, const float* d_res, float* d_x,
                                   float* d_w_tpg, float* d_b_theta, float* d_b_phi, float* d_b_g, float* d_w_back,
                                   float* d_b_back, float p_att, float p_proj, unsigned long long seed,
                                   void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(x && w_tpg && b_theta && b_phi && b_g && w_back && tpg && wavg && d_res && d_w_tpg && d_b_theta &&
                d_b_phi && d_b_g && d_w_back && d_b_back && N >= 1 && h >= 1 && w >= 1,
            "bad arguments");
  CWT_CHECK(wa_channels_ok(C), "WeightAverage: c_in a multiple of 64 up to 512, or 1024 or 2048");
  CWT_CHECK(p_att >= 0.f && p_att < 1.f && p_proj >= 0.f && p_proj < 1.f, "dropout probabilities must lie in [0, 1)");
  CWT_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const int co = C / 2;
  const long P = (long)N * h * w, ldP = ld32(P);
  const float* d_out = d_res;
  if (p_proj > 0.f) {
    float* dm;
    int rc0;
    if ((rc0 = ws(ctx, "wab.dmask", (size_t)P * C, &dm)) || (rc0 = launch_wa_proj_mask(d_res, P * C, p_proj, seed, dm, st)))
      return rc0;
    d_out = dm;
  }
  float *wbt, *dwavg, *coef, *dtpg, *dot, *wvt, *dtt, *xt;
  int rc;
  if ((rc = ws(ctx, "wab.wbT", (size_t)co * C, &wbt)) || (rc = ws(ctx, "wab.dwavg", (size_t)P * co, &dwavg)) ||
      (rc = ws(ctx, "wab.coef", (size_t)P * 27, &coef)) || (rc = ws(ctx, "wab.dtpg", (size_t)P * 3 * co, &dtpg)) ||
      (rc = ws(ctx, "wab.doT", (size_t)C * ldP, &dot)) || (rc = ws(ctx, "wab.wvT", (size_t)co * ldP, &wvt)) ||
      (rc = ws(ctx, "wab.dtT", (size_t)3 * co * ldP, &dtt)) || (rc = ws(ctx, "wab.xT", (size_t)C * ldP, &xt)))
    return rc;
  Prof p(ctx, st, "weight_average_backward c" + std::to_string(C), 2.0 * P * C * co * 8, 4.0 * P * (4.0 * C + 8.0 * co));
  // d wavg = d_out . w_back  (conv_back, msm_func.py:99)
  if ((rc = launch_match_vt(w_back, 1, C, co, C, wbt, st)) || (rc = gemm_nt(ctx, d_out, wbt, (int)P, co, C, dwavg, st)))
    return rc;
  // softmax-weighted neighbourhood and the cosine similarities (msm_func.py:66-97)
  if ((rc = launch_wa_bwd(tpg, N, h, w, co, b_theta, b_phi, b_g, dwavg, coef, dtpg, st, p_att, seed))) return rc;
  // biases: column sums in a fixed order
  float* csw;
  const size_t csn = colsum_ws_floats(P, C);
  if ((rc = ws(ctx, "colsum", csn, &csw))) return rc;
  if ((rc = launch_colsum(dtpg, P, co, 3L * co, 0, d_b_theta, csw, csn, st)) ||
      (rc = launch_colsum(dtpg + co, P, co, 3L * co, 0, d_b_phi, csw, csn, st)) ||
      (rc = launch_colsum(dtpg + 2 * co, P, co, 3L * co, 0, d_b_g, csw, csn, st)) ||
      (rc = launch_colsum(d_out, P, C, C, 0, d_b_back, csw, csn, st)))
    return rc;
  // d w_back = d_out^T . wavg, d w_tpg = d tpg^T . x (reductions over the pixels, zero-padded to 32)
  if ((rc = launch_match_vt(d_out, 1, (int)P, C, (int)ldP, dot, st)) ||
      (rc = launch_match_vt(wavg, 1, (int)P, co, (int)ldP, wvt, st)) ||
      (rc = gemm_nt(ctx, dot, wvt, C, co, (int)ldP, d_w_back, st)) ||
      (rc = launch_match_vt(dtpg, 1, (int)P, 3 * co, (int)ldP, dtt, st)) ||
      (rc = launch_match_vt(x, 1, (int)P, C, (int)ldP, xt, st)) ||
      (rc = gemm_nt(ctx, dtt, xt, 3 * co, C, (int)ldP, d_w_tpg, st)))
    return rc;
  if (d_x) {  // d x = d_out (the residual) + d tpg . w_tpg
    float* wtt;
    if ((rc = ws(ctx, "wab.wtT", (size_t)C * 3 * co, &wtt))) return rc;
    if ((rc = launch_match_vt(w_tpg, 1, 3 * co, C, 3 * co, wtt, st))) return rc;
    if (gemm_f32d_ok((int)P, C, 3 * co, dtpg, wtt, d_x, d_res)) {
      if ((rc = gemm_f32d(ctx, dtpg, wtt, (int)P, C, 3 * co, d_x, nullptr, d_res, C, st))) return rc;
    } else if ((rc = gemm_nt(ctx, dtpg, wtt, (int)P, C, 3 * co, d_x, st)) ||
               (rc = launch_add_inplace(d_x, d_res, P * C, st))) {
      return rc;
    }
  }
  p.end();
  return 0;
}

int cwt_weight_average_backward(cwt_ctx* ctx, const float* x, int N, int h, int w, int C, const float* w_tpg,
                                const float* b_theta, const float* b_phi, const float* b_g, const float* w_back,
                                const float* tpg, const float* wavg, const float* d_out, float* d_x,
                                float* d_w_tpg, float* d_b_theta, float* d_b_phi, float* d_b_g, float* d_w_back,
                                float* d_b_back, void* stream) {
  return weight_average_backward(ctx, x, N, h, w, C, w_tpg, b_theta, b_phi, b_g, w_back, tpg, wavg, d_out, d_x, d_w_tpg,
                                 d_b_theta, d_b_phi, d_b_g, d_w_back, d_b_back, 0.f, 0.f, 0, stream);
}

int cwt_weight_average_backward_drop(cwt_ctx* ctx, const float* x, int N, int h, int w, int C, const float* w_tpg,
                                     const float* b_theta, const float* b_phi, const float* b_g,
                                     const float* w_back, const float* tpg, const float* wavg, const float* d_out,
                                     float* d_x, float* d_w_tpg, float* d_b_theta, float* d_b_phi, float* d_b_g,
                                     float* d_w_back, float* d_b_back, float p_att, float p_proj, uint64_t seed,
                                     void* stream) {
  return weight_average_backward(ctx, x, N, h, w, C, w_tpg, b_theta, b_phi, b_g, w_back, tpg, wavg, d_out, d_x, d_w_tpg,
                                 d_b_theta, d_b_phi, d_b_g, d_w_back, d_b_back, p_att, p_proj, (unsigned long long)seed,
                                 stream);
}

int cwt_mmn_blend_backward(cwt_ctx* ctx, const float* d_fq, const float* d_att_mean, int B, int64_t n, float att_wt,
                           float* d_att, float* d_fq_in, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(d_att && B >= 1 && n >= 1, "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  return launch_mmn_blend_bwd(d_fq, d_att_mean, B, (long)n, att_wt, d_att, d_fq_in, (hipStream_t)stream);
}

int cwt_mmn_blend(cwt_ctx* ctx, const float* f_q, const float* att_fq, int B, int64_t n, float att_wt,
                  float* att_mean, float* fq_out, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(f_q && att_fq && att_mean && fq_out && B >= 1 && n >= 1, "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  return launch_mmn_blend(f_q, att_fq, B, (long)n, att_wt, att_mean, fq_out, (hipStream_t)stream);
}

int cwt_linear(cwt_ctx* ctx, const float* x, int64_t P, int K, const float* w, const float* bias, int N, int relu,
               int accumulate, float* out, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(x && w && out && P >= 1 && K >= 4 && K % 4 == 0 && N >= 1 && P <= (1L << 30), "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  float* tmp;
  int rc;
  if ((rc = ws(ctx, "linear.tmp", (size_t)P * N, &tmp))) return rc;
  Prof p(ctx, st, "linear " + std::to_string(K) + "x" + std::to_string(N), 2.0 * P * N * K,
         4.0 * ((double)P * K + (double)N * K + (double)P * N));
  if (!accumulate && gemm_f32d_ok((int)P, N, K, x, w, out, nullptr)) {  // (tmp + bias), relu: the epilogue's order
    if ((rc = gemm_f32d(ctx, x, w, (int)P, N, K, out, bias, nullptr, 0, st, relu))) return rc;
  } else {
    if (gemm_f32d_ok((int)P, N, K, x, w, tmp, nullptr)) {
      if ((rc = gemm_f32d(ctx, x, w, (int)P, N, K, tmp, nullptr, nullptr, 0, st))) return rc;
    } else if ((rc = launch_gemm_abt(x, w, 1, (int)P, N, K, tmp, st))) {
      return rc;
    }
    if ((rc = launch_linear_epilogue(tmp, bias, accumulate ? out : nullptr, (long)P, N, relu, out, st))) return rc;
  }
  p.end();
  return 0;
}

int cwt_sine_pos_add(cwt_ctx* ctx, const float* x, int B, int h, int w, int C, float temperature, int normalize,
                     float scale, float eps, float* out, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(x && out && B >= 1 && h >= 1 && w >= 1 && C >= 2 && C % 2 == 0 && temperature > 0.f, "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  return launch_sine_pos_add(x, B, h, w, C, temperature, normalize, scale, eps, out, (hipStream_t)stream);
}

int cwt_deform_attn(cwt_ctx* ctx, const float* value, const float* offsets, const float* logits, int B, int H, int W,
                    int n_heads, int n_points, int d_head, float* out, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(value && offsets && logits && out && B >= 1 && H >= 1 && W >= 1 && n_heads >= 1 && n_points >= 1 &&
                d_head >= 1,
            "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  Prof p(ctx, st, "deform_attn", 2.0 * B * H * W * n_heads * n_points * d_head * 5,
         4.0 * (double)B * H * W * n_heads * (d_head * 2 + n_points * 3));
  int rc = launch_deform_attn(value, offsets, logits, B, H, W, n_heads, n_points, d_head, out, st);
  p.end();
  return rc;
}

int cwt_norm_blend(cwt_ctx* ctx, const float* a, const float* b, int64_t T, int C, float wt, float* out,
                   void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(a && b && out && T >= 1 && C >= 1, "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  return launch_norm_blend(a, b, (long)T, C, wt, out, (hipStream_t)stream);
}

// ---- DeTr head backward (train_trans.py:100): linear / 1x1 conv, deformable attention, blend ----
int cwt_linear_backward(cwt_ctx* ctx, const float* x, int64_t P, int K, const float* w, int N, const float* out,
                        const float* d_out, float* d_x, float* d_w, int ldw, float* d_b, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(x && w && d_out && P >= 1 && K >= 1 && N >= 1 && P <= (1L << 30) && (!d_w || ldw >= K), "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const long ldN = ld32(N), ldP = ld32(P);
  float *gm, *wt, *gt, *xt;
  int rc;
  if ((rc = ws(ctx, "lb.gm", (size_t)P * ldN, &gm))) return rc;
  Prof p(ctx, st, "linear_backward " + std::to_string(K) + "x" + std::to_string(N), 4.0 * P * N * K,
         4.0 * ((double)P * K * 2 + (double)N * K * 2 + (double)P * N * 2));
  // the output gradient through the ReLU (out > 0) when out is given
  const float* g = d_out;
  if (out) {
    if ((rc = launch_relu_mask(d_out, out, P * N, gm, st))) return rc;
    g = gm;
  }
  if (d_b) {
    float* csw;
    const size_t csn = colsum_ws_floats(P, N);
    if ((rc = ws(ctx, "colsum", csn, &csw)) || (rc = launch_colsum(g, P, N, N, 0, d_b, csw, csn, st))) return rc;
  }
  if (d_x) {  // d x = g . w   (A = g [P][ldN], B^T = w^T [K][ldN])
    const float* gp = g;
    if (ldN != N) {
      float* gpad;
      if ((rc = ws(ctx, "lb.gpad", (size_t)P * ldN, &gpad)) || (rc = launch_copy_pad(g, P, N, (int)ldN, gpad, st)))
        return rc;
      gp = gpad;
    }
    if ((rc = ws(ctx, "lb.wT", (size_t)K * ldN, &wt)) || (rc = launch_match_vt(w, 1, N, K, (int)ldN, wt, st)) ||
        (rc = gemm_nt(ctx, gp, wt, (int)P, K, (int)ldN, d_x, st)))
      return rc;
  }
  if (d_w) {  // d w = g^T . x   (A = g^T [N][ldP], B^T = x^T [K][ldP])
    if ((rc = ws(ctx, "lb.gT", (size_t)N * ldP, &gt)) || (rc = ws(ctx, "lb.xT", (size_t)K * ldP, &xt)) ||
        (rc = launch_match_vt(g, 1, (int)P, N, (int)ldP, gt, st)) ||
        (rc = launch_match_vt(x, 1, (int)P, K, (int)ldP, xt, st)))
      return rc;
    float* dst = d_w;  // a dense [N][K] scratch when d_w's rows are strided
    if (ldw != K && (rc = ws(ctx, "lb.dw", (size_t)N * K, &dst))) return rc;
    if ((rc = gemm_nt(ctx, gt, xt, N, K, (int)ldP, dst, st))) return rc;
    if (ldw != K && (rc = launch_copy_2d(dst, N, K, K, d_w, ldw, st))) return rc;
  }
  p.end();
  return 0;
}

int cwt_deform_attn_backward(cwt_ctx* ctx, const float* value, const float* offsets, const float* logits, int B, int H,
                             int W, int n_heads, int n_points, int d_head, const float* d_out, float* d_value,
                             float* d_offsets, float* d_logits, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(value && offsets && logits && d_out && d_value && d_offsets && d_logits && B >= 1 && H >= 1 && W >= 1 &&
                n_heads >= 1 && n_points >= 1 && d_head >= 1,
            "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  Prof p(ctx, st, "deform_attn_backward", 2.0 * B * H * W * n_heads * n_points * d_head * 12,
         4.0 * (double)B * H * W * n_heads * (d_head * 7 + n_points * 6));
  void* ws;
  int rc;
  if ((rc = ensure_ws(ctx, "detr.dv64", deform_attn_bwd_ws_bytes(B, H, W, n_heads, d_head), &ws))) return rc;
  rc = launch_deform_attn_bwd(value, offsets, logits, B, H, W, n_heads, n_points, d_head, d_out, d_value, d_offsets,
                              d_logits, ws, st);
  p.end();
  return rc;
}

int cwt_norm_blend_backward(cwt_ctx* ctx, const float* a, const float* b, int64_t T, int C, float wt, const float* d_out,
                            float* d_a, float* d_b, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(a && b && d_out && T >= 1 && C >= 1, "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  return launch_norm_blend_bwd(a, b, d_out, (long)T, C, wt, d_a, d_b, (hipStream_t)stream);
}

}  // extern "C"
