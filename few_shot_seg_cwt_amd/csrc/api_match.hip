// MatchNet entry points of libcwt.so (include/cwt.h), forward and backward: the correlation,
// MutualMatching, the match pass and its backward -- the executors of match_plan.h's MatchPlan /
// MatchBwdPlan -- the support masks, the softmax readout, and the spatial context descriptor.
#include "ctx.h"
#include "match_plan.h"

using namespace cwt;

// ---- MatchNet (match.py:21-163, conv4d.py:11-62) ----
static int mm_ws(cwt_ctx* ctx, int B, int NA, int NB, int C, float** rowmax, float** colpart, float** colmax) {
  int rc;
  const long nrb = cdiv(NA, 8);  // row blocks of launch_mutual_matching (8 rows: vector forms; 16: scalar)
  if ((rc = ws(ctx, "match.rowmax", (size_t)B * C * NA, rowmax)) ||
      (rc = ws(ctx, "match.colpart", (size_t)B * C * nrb * NB, colpart)) ||
      (rc = ws(ctx, "match.colmax", (size_t)B * C * NB, colmax)))
    return rc;
  return 0;
}

int cwt::mm_bwd_ws(cwt_ctx* ctx, int B, int NA, int NB, int C, MmBwdWs* w) {
  const long nrb = cdiv(NA, 16), bc = (long)B * C;
  int rc;
  if ((rc = ws(ctx, "mb.rowmax", bc * NA, &w->rowmax)) || (rc = ws(ctx, "mb.rowarg", bc * NA, &w->rowarg)) ||
      (rc = ws(ctx, "mb.colpv", bc * nrb * NB, &w->colpv)) || (rc = ws(ctx, "mb.colpi", bc * nrb * NB, &w->colpi)) ||
      (rc = ws(ctx, "mb.colmax", bc * NB, &w->colmax)) || (rc = ws(ctx, "mb.colarg", bc * NB, &w->colarg)) ||
      (rc = ws(ctx, "mb.srow", bc * NA, &w->srow)) || (rc = ws(ctx, "mb.scol", bc * NB, &w->scol)))
    return rc;
  return 0;
}

// One entry of a plan's buffer table to its pointer (nullptr: the pass has no such tensor)
static int match_buf(cwt_ctx* ctx, const MatchBuf& b, float* saved, int Cv, float** p) {
  *p = nullptr;
  if (!b.floats) return 0;
  if (b.ws) return ws(ctx, b.ws, (size_t)b.floats * (b.per_cv ? Cv : 1), p);
  *p = saved + b.off;
  return 0;
}

// The readout: attn = softmax(temp * corr2d, dim=-1) [B][NA][ldp], zero-padded to ldp = ld32(NB);
// weighted_v = bmm(v, attn^T) (match.py:151-153), here as tokens [B][NA][Cv] = attn . v through
// vt [B][Cv][ldp]
static int match_readout_fwd(cwt_ctx* ctx, const float* corr2d, int B, int NA, int NB, float temp, const float* v,
                             int Cv, float* attn, float* vt, float* weighted_v, hipStream_t st) {
  const int ldp = (int)ld32(NB);
  int rc;
  if ((rc = launch_match_softmax(corr2d, B, NA, NB, temp, ldp, attn, st))) return rc;
  if ((rc = launch_match_vt(v, B, NB, Cv, ldp, vt, st))) return rc;
  return readout_gemm(ctx, attn, vt, B, NA, Cv, ldp, weighted_v, st);
}

// The readout's backward from attn (the forward's, kept or computed again):
// g2d += temp attn (dA - <attn, dA>) with dA = d_wv . v^T, the ig-masked columns of g2d zeroed (the
// reference overwrote them with a constant), d_v[b] = attn[b]^T . d_wv[b]
static int match_readout_bwd(cwt_ctx* ctx, const float* attn, int B, int NA, int NB, float temp, const float* v,
                             int Cv, const float* d_weighted_v, const uint8_t* ig_mask, float* g2d, float* d_v,
                             hipStream_t st) {
  const long ldp = ld32(NB);
  int rc;
  if (d_weighted_v) {
    float* dA;
    if ((rc = ws(ctx, "mb.dA", (size_t)B * NA * NB, &dA))) return rc;
    for (int b = 0; b < B; ++b)
      if ((rc = gemm_nt(ctx, d_weighted_v + (long)b * NA * Cv, v + (long)b * NB * Cv, NA, NB, Cv,
                        dA + (long)b * NA * NB, st)))
        return rc;
    if ((rc = launch_match_softmax_bwd(attn, (int)ldp, dA, B * NA, NB, temp, 1, g2d, st))) return rc;
  }
  if (ig_mask && (rc = launch_match_zero_ig_cols(g2d, ig_mask, B, NA, NB, st))) return rc;
  if (d_v) {
    const long lda = ld32(NA);
    float *pt, *dwt;
    if ((rc = ws(ctx, "mb.PT", (size_t)B * ldp * lda, &pt)) || (rc = ws(ctx, "mb.dwvT", (size_t)B * Cv * lda, &dwt)))
      return rc;
    if ((rc = launch_match_vt(attn, B, NA, (int)ldp, (int)lda, pt, st)) ||
        (rc = launch_match_vt(d_weighted_v, B, NA, Cv, (int)lda, dwt, st)))
      return rc;
    for (int b = 0; b < B; ++b)
      if ((rc = gemm_nt(ctx, pt + (long)b * ldp * lda, dwt + (long)b * Cv * lda, NB, Cv, (int)lda,
                        d_v + (long)b * NB * Cv, st)))
        return rc;
  }
  return 0;
}

// The executor of a MatchPlan: run_match_model (match.py:159-163) and the readout
static int match_corr_forward(cwt_ctx* ctx, const float* corr, int B, int L, int h, int w, const float* nc_params,
                              int symmetric, float temp, const float* v, int Cv, float* corr2d, float* weighted_v,
                              void* stream, bool cv4, float* saved = nullptr) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(corr && nc_params && corr2d, MATCH_MSG_ARGS);
  const MatchPlan P = match_plan(B, L, h, w, symmetric != 0, cv4, saved != nullptr, weighted_v != nullptr, match_env());
  CWT_CHECK(!P.rc, P.msg);
  CWT_CHECK(!weighted_v || (v && Cv >= 1), "weighted_v needs v");
  CWT_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const int NA = h * w;
  const long E = (long)B * NA * NA;
  const MatchParams& T = P.params;
  // the plan's buffer table to pointers, once
  float *x0, *o[2][3] = {}, *y, *attn, *vt, *rm, *cp, *cm;
  int rc;
  if ((rc = match_buf(ctx, P.x0, saved, Cv, &x0)) || (rc = match_buf(ctx, P.y, saved, Cv, &y)) ||
      (rc = match_buf(ctx, P.attn, saved, Cv, &attn)) || (rc = match_buf(ctx, P.vt, saved, Cv, &vt)) ||
      (rc = mm_ws(ctx, B, NA, NA, L, &rm, &cp, &cm)))
    return rc;
  for (int br = 0; br < P.branches; ++br)
    for (int l = 0; l < 3; ++l)
      if ((rc = match_buf(ctx, P.o[br][l], saved, Cv, &o[br][l]))) return rc;
  Prof p(ctx, st, "match_corr_forward", 2.0 * E * 2 * (18.0 * L * 10 + 18.0 * 100 + 18.0 * 10), 4.0 * E * (L + 1));
  if (P.mm1 == MM1_DIRECT) {
    if ((rc = launch_mutual_matching(corr, B, NA, NA, 1, x0, rm, cp, cm, st))) return rc;
  } else if (P.mm1 == MM1_PLANAR2) {
    if ((rc = launch_mutual_matching_planar2(corr, B, NA, NA, x0, rm, cp, cm, st))) return rc;
  } else {
    if ((rc = launch_to_channels_last(corr, B, L, (long)NA * NA, x0, st))) return rc;
    if ((rc = launch_mutual_matching(x0, B, NA, NA, L, x0, rm, cp, cm, st))) return rc;
  }
  if (P.fork) {
    if (!ctx->aux) CWT_HIP(hipStreamCreateWithFlags(&ctx->aux, hipStreamNonBlocking));
    if (!ctx->ev_fork) CWT_HIP(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    if (!ctx->ev_join) CWT_HIP(hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
    CWT_HIP(hipEventRecord(ctx->ev_fork, st));
    CWT_HIP(hipStreamWaitEvent(ctx->aux, ctx->ev_fork, 0));
  }
  for (int br = 0; br < P.branches; ++br) {
    const float* in = x0;
    const hipStream_t bst = (P.fork && br == 1) ? ctx->aux : st;
    for (int l = 0; l < 3; ++l) {
      const int cin = match_ch(L, l), cout = match_ch(L, l + 1);
      // Conv4d (conv4d.py:64-138): branch 1 is the same stack with each filter's position pairs
      // exchanged (cv4d_layer_kernel's swap); CenterPivotConv4d: with the a and b roles exchanged
      rc = P.cv4 ? launch_cv4d_layer(in, B, h, w, h, w, cin, cout, nc_params + T.W[l][0], nc_params + T.b[l][0], br,
                                     o[br][l], st)
                 : launch_cp4d_layer(in, B, h, w, h, w, cin, cout, nc_params + T.Wa(l, br), nc_params + T.ba(l, br),
                                     nc_params + T.Wb(l, br), nc_params + T.bb(l, br), o[br][l], bst);
      if (rc) return rc;
      in = o[br][l];
    }
  }
  if (P.fork) {
    CWT_HIP(hipEventRecord(ctx->ev_join, ctx->aux));
    CWT_HIP(hipStreamWaitEvent(st, ctx->ev_join, 0));
  }
  // training: y in its own slot, the ReLU outputs stay for the backward
  if (P.train) CWT_HIP(hipMemcpyAsync(y, o[0][2], (size_t)E * 4, hipMemcpyDeviceToDevice, st));
  if (P.mm2 == MM2_ADD && (rc = launch_add_inplace(y, (const float*)o[1][2], E, st))) return rc;
  if (P.mm2 == MM2_SUM) {  // MutualMatching of o[0][2] + o[1][2] (the sum folded into its two passes)
    if ((rc = launch_mutual_matching_sum(o[0][2], o[1][2], B, NA, NA, corr2d, rm, cp, cm, st))) return rc;
  } else if ((rc = launch_mutual_matching(y, B, NA, NA, 1, corr2d, rm, cp, cm, st))) {
    return rc;
  }
  if (P.readout && (rc = match_readout_fwd(ctx, corr2d, B, NA, NA, temp, v, Cv, attn, vt, weighted_v, st))) return rc;
  p.end();
  return 0;
}

extern "C" {

int cwt_corr(cwt_ctx* ctx, const float* q, const float* k, int B, int Pq, int Pk, int C, float* sim, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(q && k && sim && B >= 1 && Pq >= 1 && Pk >= 1 && C >= 4 && C % 4 == 0, "bad arguments (C % 4 == 0)");
  CWT_HIP(hipSetDevice(ctx->device));
  float *qn, *kn;
  int rc;
  if ((rc = ws(ctx, "corr.q", (size_t)B * Pq * C, &qn)) || (rc = ws(ctx, "corr.k", (size_t)B * Pk * C, &kn))) return rc;
  return launch_corr(q, k, B, Pq, Pk, C, qn, kn, sim, (hipStream_t)stream);
}

int cwt_mutual_matching(cwt_ctx* ctx, const float* x, int B, int NA, int NB, int C, float* y, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(x && y && B >= 1 && NA >= 1 && NB >= 1 && C >= 1 && C <= 64, "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  float *rm, *cp, *cm;
  int rc;
  if ((rc = mm_ws(ctx, B, NA, NB, C, &rm, &cp, &cm))) return rc;
  return launch_mutual_matching(x, B, NA, NB, C, y, rm, cp, cm, (hipStream_t)stream);
}

int cwt_match_corr_forward(cwt_ctx* ctx, const float* corr, int B, int L, int h, int w, const float* nc_params,
                           int symmetric, float temp, const float* v, int Cv, float* corr2d, float* weighted_v,
                           void* stream) {
  return match_corr_forward(ctx, corr, B, L, h, w, nc_params, symmetric, temp, v, Cv, corr2d, weighted_v, stream, false);
}

int cwt_match_corr_forward_cv4(cwt_ctx* ctx, const float* corr, int B, int L, int h, int w, const float* nc_params,
                               int symmetric, float temp, const float* v, int Cv, float* corr2d, float* weighted_v,
                               void* stream) {
  return match_corr_forward(ctx, corr, B, L, h, w, nc_params, symmetric, temp, v, Cv, corr2d, weighted_v, stream, true);
}

// ---- MatchNet / MMN backward (match_bwd.hip) ----
int cwt_match_corr_saved_floats(int B, int L, int h, int w, int symmetric, int readout, int64_t* n) {
  if (!n || B < 1 || L < 1 || L > CWT_MATCH_MAX_L || h < 1 || w < 1) return fail(CWT_EARG, MATCH_MSG_ARGS);
  *n = (int64_t)match_saved_layout(B, L, (long)h * w, symmetric != 0, readout != 0).total;
  return 0;
}

int cwt_match_corr_forward_train(cwt_ctx* ctx, const float* corr, int B, int L, int h, int w, const float* nc_params,
                                 int symmetric, float temp, const float* v, int Cv, float* corr2d, float* weighted_v,
                                 float* saved, void* stream) {
  if (!saved) return fail(CWT_EARG, "saved is NULL");
  return match_corr_forward(ctx, corr, B, L, h, w, nc_params, symmetric, temp, v, Cv, corr2d, weighted_v, stream, false,
                            saved);
}

// The executor of a MatchBwdPlan
int cwt_match_corr_backward(cwt_ctx* ctx, const float* corr, int B, int L, int h, int w, const float* nc_params,
                            int symmetric, float temp, const float* v, int Cv, const float* saved,
                            const float* d_corr2d, const float* d_weighted_v, float* d_corr, float* d_params,
                            float* d_v, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(corr && nc_params && saved && d_params, MATCH_MSG_ARGS);
  const MatchBwdPlan P =
      match_bwd_plan(B, L, h, w, symmetric != 0, d_corr != nullptr, d_v != nullptr, d_weighted_v != nullptr);
  CWT_CHECK(!P.rc, P.msg);
  CWT_CHECK(!d_weighted_v || (v && Cv >= 4 && Cv % 4 == 0), "d_weighted_v needs v and Cv % 4 == 0");
  CWT_CHECK(!d_v || d_weighted_v, "d_v needs d_weighted_v");
  CWT_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const int NA = h * w;
  const long E = (long)B * NA * NA;
  const MatchParams& T = P.params;
  const MatchSavedLayout& S = P.saved;
  float *g2d, *dy, *gA, *gm, *dx0, *part, *xcl, *dxcl;
  MmBwdWs mw;
  int rc;
  if ((rc = match_buf(ctx, P.g2d, nullptr, 0, &g2d)) || (rc = match_buf(ctx, P.dy, nullptr, 0, &dy)) ||
      (rc = match_buf(ctx, P.gA, nullptr, 0, &gA)) || (rc = match_buf(ctx, P.gm, nullptr, 0, &gm)) ||
      (rc = match_buf(ctx, P.dx0, nullptr, 0, &dx0)) || (rc = match_buf(ctx, P.part, nullptr, 0, &part)) ||
      (rc = match_buf(ctx, P.xcl, nullptr, 0, &xcl)) || (rc = match_buf(ctx, P.dxcl, nullptr, 0, &dxcl)) ||
      (rc = mm_bwd_ws(ctx, B, NA, NA, L, &mw)))
    return rc;
  Prof p(ctx, st, "match_corr_backward", 2.0 * 2.0 * E * 2 * (18.0 * L * 10 + 18.0 * 100 + 18.0 * 10),
         4.0 * E * (L + 44));
  CWT_HIP(hipMemsetAsync(d_params, 0, (size_t)T.total * 4, st));
  // the gradient at corr2d: the caller's, plus the softmax readout's (match.py:151-153)
  if (d_corr2d)
    CWT_HIP(hipMemcpyAsync(g2d, d_corr2d, (size_t)E * 4, hipMemcpyDeviceToDevice, st));
  else
    CWT_HIP(hipMemsetAsync(g2d, 0, (size_t)E * 4, st));
  if (P.readout &&
      (rc = match_readout_bwd(ctx, saved + S.attn, B, NA, NA, temp, v, Cv, d_weighted_v, nullptr, g2d, d_v, st)))
    return rc;
  // the second MutualMatching (match.py:162)
  if ((rc = launch_mutual_matching_bwd(saved + S.y, g2d, B, NA, NA, 1, dy, mw, st))) return rc;
  // NeighConsensus: both branches see the same output gradient (y = branch 0 + branch 1); branch 1
  // applied conv2's filter over the a plane and conv1's over the b plane (match.py:75-80).  The two
  // bias gradients are the same sum in either branch: their slots are not exchanged.
  for (int br = 0; br < P.branches; ++br) {
    const float* gcur = dy;
    for (int l = 2; l >= 0; --l) {
      const int cin = match_ch(L, l), cout = match_ch(L, l + 1);
      const float* in = l ? saved + S.o[br][l - 1] : saved + S.x0;
      const float *Wa = nc_params + T.Wa(l, br), *Wb = nc_params + T.Wb(l, br);
      if ((rc = launch_relu_mask(gcur, saved + S.o[br][l], E * cout, gm, st))) return rc;
      if ((rc = launch_cp4d_wgrad(in, gm, B, h, w, h, w, cin, cout, part, (size_t)P.part.floats, d_params + T.Wa(l, br),
                                  d_params + T.Wb(l, br), d_params + T.ba(l, 0), d_params + T.bb(l, 0), st)))
        return rc;
      if (l > 0) {
        if ((rc = launch_cp4d_dgrad(gm, B, h, w, h, w, cout, cin, Wa, Wb, gA, 0, st))) return rc;
        gcur = gA;
      } else if (P.d_corr) {
        if ((rc = launch_cp4d_dgrad(gm, B, h, w, h, w, cout, cin, Wa, Wb, dx0, br, st))) return rc;
      }
    }
  }
  // the first MutualMatching (match.py:160), back to the caller's channel-first layout
  if (P.d_corr && !P.clast) {
    if ((rc = launch_mutual_matching_bwd(corr, dx0, B, NA, NA, 1, d_corr, mw, st))) return rc;
  } else if (P.d_corr) {
    if ((rc = launch_to_channels_last(corr, B, L, (long)NA * NA, xcl, st)) ||
        (rc = launch_mutual_matching_bwd(xcl, dx0, B, NA, NA, L, dxcl, mw, st)) ||
        (rc = launch_to_channels_first(dxcl, B, L, (long)NA * NA, d_corr, st)))
      return rc;
  }
  p.end();
  return 0;
}

int cwt_corr_backward(cwt_ctx* ctx, const float* q, const float* k, int B, int Pq, int Pk, int C, const float* d_sim,
                      float* dq, float* dk, int accum_q, int accum_k, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(q && k && d_sim && B >= 1 && Pq >= 1 && Pk >= 1 && C >= 1, "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const float eps = 1e-12f;
  float *qn, *qr, *kn, *kr;
  int rc;
  if ((rc = ws(ctx, "cb.qn", (size_t)B * Pq * C, &qn)) || (rc = ws(ctx, "cb.qr", (size_t)B * Pq, &qr)) ||
      (rc = ws(ctx, "cb.kn", (size_t)B * Pk * C, &kn)) || (rc = ws(ctx, "cb.kr", (size_t)B * Pk, &kr)))
    return rc;
  Prof p(ctx, st, "corr_backward", 2.0 * 2.0 * B * (double)Pq * Pk * C, 4.0 * B * ((double)Pq * Pk + 2.0 * (Pq + Pk) * C));
  if ((rc = launch_token_norm(q, (long)B * Pq, C, eps, qn, qr, st)) ||
      (rc = launch_token_norm(k, (long)B * Pk, C, eps, kn, kr, st)))
    return rc;
  if (dq) {  // d qn = d_sim . kn
    const long ldk = ld32(Pk);
    float *dsp, *knt, *dqn;
    if ((rc = ws(ctx, "cb.dsp", (size_t)B * Pq * ldk, &dsp)) || (rc = ws(ctx, "cb.knT", (size_t)B * C * ldk, &knt)) ||
        (rc = ws(ctx, "cb.dqn", (size_t)B * Pq * C, &dqn)))
      return rc;
    if ((rc = launch_copy_pad(d_sim, (long)B * Pq, Pk, (int)ldk, dsp, st)) ||
        (rc = launch_match_vt(kn, B, Pk, C, (int)ldk, knt, st)))
      return rc;
    for (int b = 0; b < B; ++b)
      if ((rc = gemm_nt(ctx, dsp + (long)b * Pq * ldk, knt + (long)b * C * ldk, Pq, C, (int)ldk, dqn + (long)b * Pq * C,
                        st)))
        return rc;
    if ((rc = launch_token_norm_bwd(qn, qr, dqn, (long)B * Pq, C, C, eps, accum_q, dq, st))) return rc;
  }
  if (dk) {  // d kn = d_sim^T . qn
    const long ldq = ld32(Pq);
    float *dst, *qnt, *dkn;
    if ((rc = ws(ctx, "cb.dsT", (size_t)B * Pk * ldq, &dst)) || (rc = ws(ctx, "cb.qnT", (size_t)B * C * ldq, &qnt)) ||
        (rc = ws(ctx, "cb.dkn", (size_t)B * Pk * C, &dkn)))
      return rc;
    if ((rc = launch_match_vt(d_sim, B, Pq, Pk, (int)ldq, dst, st)) ||
        (rc = launch_match_vt(qn, B, Pq, C, (int)ldq, qnt, st)))
      return rc;
    for (int b = 0; b < B; ++b)
      if ((rc = gemm_nt(ctx, dst + (long)b * Pk * ldq, qnt + (long)b * C * ldq, Pk, C, (int)ldq, dkn + (long)b * Pk * C,
                        st)))
        return rc;
    if ((rc = launch_token_norm_bwd(kn, kr, dkn, (long)B * Pk, C, C, eps, accum_k, dk, st))) return rc;
  }
  p.end();
  return 0;
}

int cwt_sce_descriptor(cwt_ctx* ctx, const float* x, int B, int h, int w, int C, int k, int ldg, float* g,
                       void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(x && g && B >= 1 && h >= 1 && w >= 1 && C >= 1, "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  Prof p(ctx, st, "sce_descriptor", 2.0 * B * h * w * (double)k * k * C, 4.0 * B * h * w * ((double)C + ldg));
  int rc;
  if ((rc = launch_sce_descriptor(x, B, h, w, C, k, ldg, g, st))) return rc;
  p.end();
  return 0;
}

int cwt_channel_sum(cwt_ctx* ctx, const float* x, int B, int L, int64_t P, float* y, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(x && y && B >= 1 && L >= 1 && P >= 1, "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  Prof p(ctx, st, "channel_sum", (double)B * L * P, 4.0 * B * P * (L + 1));
  int rc;
  if ((rc = launch_channel_sum(x, B, L, (long)P, y, st))) return rc;
  p.end();
  return 0;
}

int cwt_match_masks(cwt_ctx* ctx, float* corr2d, int B, int NA, int NB, const uint8_t* ig_mask,
                    const int64_t* s_mask, float* inconsistent, void* stream) {
  return cwt_match_masks_train(ctx, corr2d, B, NA, NB, ig_mask, s_mask, inconsistent, 0.f, 0, stream);
}

int cwt_match_masks_train(cwt_ctx* ctx, float* corr2d, int B, int NA, int NB, const uint8_t* ig_mask,
                          const int64_t* s_mask, float* inconsistent, float drop_p, uint64_t seed, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(corr2d && B >= 1 && NA >= 1 && NB >= 1 && drop_p >= 0.f && drop_p < 1.f, "bad arguments");
  CWT_CHECK(!s_mask || inconsistent, "the cycle mask needs inconsistent");
  CWT_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  int *q2k = nullptr, *pi = nullptr;
  float* pv = nullptr;
  int rc;
  if (s_mask && ((rc = ws(ctx, "match.q2k", (size_t)B * NA, &q2k)) || (rc = ws(ctx, "match.colv", (size_t)B * 16 * NB, &pv)) ||
                 (rc = ws(ctx, "match.coli", (size_t)B * 16 * NB, &pi))))
    return rc;
  Prof p(ctx, st, "match_masks", 0.0, 4.0 * B * NA * NB * (s_mask ? 4 : 2));
  if ((rc = launch_match_masks(corr2d, B, NA, NB, ig_mask, s_mask, inconsistent, q2k, pv, pi, st, drop_p,
                               (unsigned long long)seed)))
    return rc;
  p.end();
  return 0;
}

int cwt_match_readout(cwt_ctx* ctx, const float* corr2d, int B, int NA, int NB, float temp, const float* v, int Cv,
                      float* weighted_v, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(corr2d && v && weighted_v && B >= 1 && NA >= 1 && NB >= 1 && Cv >= 1, "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const long ldp = ld32(NB);
  float *attn, *vt;
  int rc;
  if ((rc = ws(ctx, "match.attn", (size_t)B * NA * ldp, &attn)) || (rc = ws(ctx, "match.vt", (size_t)B * Cv * ldp, &vt)))
    return rc;
  Prof p(ctx, st, "match_readout", 2.0 * B * NA * (double)NB * Cv, 4.0 * B * ((double)NA * NB * 2 + (double)NB * Cv));
  if ((rc = match_readout_fwd(ctx, corr2d, B, NA, NB, temp, v, Cv, attn, vt, weighted_v, st))) return rc;
  p.end();
  return 0;
}

int cwt_match_readout_backward(cwt_ctx* ctx, const float* corr2d, int B, int NA, int NB, float temp, const float* v,
                               int Cv, const float* d_weighted_v, const uint8_t* ig_mask, float* d_corr2d, float* d_v,
                               void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(corr2d && d_corr2d && B >= 1 && NA >= 1 && NB >= 1, "bad arguments");
  CWT_CHECK(!d_weighted_v || (v && Cv >= 4 && Cv % 4 == 0), "d_weighted_v needs v and Cv % 4 == 0");
  CWT_CHECK(!d_v || d_weighted_v, "d_v needs d_weighted_v");
  CWT_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const long ldp = ld32(NB);
  float* attn;
  int rc;
  if ((rc = ws(ctx, "match.attn", (size_t)B * NA * ldp, &attn))) return rc;
  Prof p(ctx, st, "match_readout_backward", 2.0 * 2.0 * B * NA * (double)NB * Cv,
         4.0 * B * ((double)NA * NB * 4 + (double)(NA + NB) * Cv * 2));
  // attn = softmax(temp corr2d) again (the forward's masked corr2d); the gradient accumulates into the
  // caller's at corr2d
  if (d_weighted_v && (rc = launch_match_softmax(corr2d, B, NA, NB, temp, (int)ldp, attn, st))) return rc;
  if ((rc = match_readout_bwd(ctx, attn, B, NA, NB, temp, v, Cv, d_weighted_v, ig_mask, d_corr2d, d_v, st))) return rc;
  p.end();
  return 0;
}

}  // extern "C"
