// MatchNet, WeightAverage and DeTr entry points of libcwt.so (include/cwt.h), forward and backward.
#include <cstdlib>

#include "ctx.h"

using namespace cwt;

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

int cwt_mutual_matching(cwt_ctx* ctx, const float* x, int B, int NA, int NB, int C, float* y, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(x && y && B >= 1 && NA >= 1 && NB >= 1 && C >= 1 && C <= 64, "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  float *rm, *cp, *cm;
  int rc;
  if ((rc = mm_ws(ctx, B, NA, NB, C, &rm, &cp, &cm))) return rc;
  return launch_mutual_matching(x, B, NA, NB, C, y, rm, cp, cm, (hipStream_t)stream);
}

// the activations the corr_forward backward reads (cwt_match_corr_forward_train), carved from one
// caller buffer: x0 = MutualMatching(corr) channels-last [E][L], o[branch][layer] the ReLU outputs
// [E][10], [E][10], [E][1], y = o[0][2] + o[1][2] [E] (E = B NA NB), attn [B][NA][ld32(NB)]
struct MatchSaved {
  float* x0;
  float* o[2][3];
  float* y;
  float* attn;
};
static size_t match_saved_layout(float* base, int B, int L, long NA, int symmetric, int readout, MatchSaved* s) {
  const long E = (long)B * NA * NA, ldp = (NA + 31) & ~31L;
  size_t off = 0;
  auto take = [&](long n) {
    float* p = base ? base + off : nullptr;
    off += (size_t)n;
    return p;
  };
  MatchSaved d;
  d.x0 = take(E * L);
  for (int br = 0; br < 2; ++br)
    for (int l = 0; l < 3; ++l) d.o[br][l] = (br == 0 || symmetric) ? take(E * (l < 2 ? 10 : 1)) : nullptr;
  d.y = take(E);
  d.attn = readout ? take((long)B * NA * ldp) : nullptr;
  if (s) *s = d;
  return off;
}

// CWT_MM_FUSE=1: the 2-channel correlation's transposition folded into MutualMatching's passes
// and the symmetric branches' sum into the second MutualMatching (fewer passes over the 4-D map)
static bool mm_fuse() {
  static const bool on = getenv("CWT_MM_FUSE") && getenv("CWT_MM_FUSE")[0] == '1';
  return on;
}

static int match_corr_forward(cwt_ctx* ctx, const float* corr, int B, int L, int h, int w, const float* nc_params,
                              int symmetric, float temp, const float* v, int Cv, float* corr2d, float* weighted_v,
                              void* stream, bool cv4, float* saved = nullptr) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(corr && nc_params && corr2d && B >= 1 && 1 <= L && L <= CWT_MATCH_MAX_L && h >= 1 && w >= 1,
            "bad arguments (in_channel 1 .. CWT_MATCH_MAX_L = 32)");
  CWT_CHECK(!cv4 || L <= 2, "Conv4d ('cv4') layers take in_channel 1 or 2 only (CenterPivotConv4d: up to 32)");
  CWT_CHECK(!weighted_v || (v && Cv >= 1), "weighted_v needs v");
  CWT_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const long NA = (long)h * w, NB = NA, P = NA * NB;
  float *x0, *x1, *x2, *y1, *y2;
  int rc;
  if ((rc = ws(ctx, "match.x0", (size_t)B * P * L, &x0)) || (rc = ws(ctx, "match.x1", (size_t)B * P * 10, &x1)) ||
      (rc = ws(ctx, "match.x2", (size_t)B * P * 10, &x2)) || (rc = ws(ctx, "match.y1", (size_t)B * P, &y1)) ||
      (rc = ws(ctx, "match.y2", (size_t)B * P, &y2)))
    return rc;
  MatchSaved S;
  if (saved) {
    CWT_CHECK(!cv4, "the training forward keeps CenterPivotConv4d ('red') activations only");
    match_saved_layout(saved, B, L, NA, symmetric, weighted_v != nullptr, &S);
    x0 = S.x0;
  }
  float *rm, *cp, *cm;
  if ((rc = mm_ws(ctx, B, (int)NA, (int)NB, L, &rm, &cp, &cm))) return rc;
  Prof p(ctx, st, "match_corr_forward", 2.0 * B * P * 2 * (18.0 * L * 10 + 18.0 * 100 + 18.0 * 10), 4.0 * B * P * (L + 1));
  // run_match_model: MutualMatching -> NeighConsensus -> MutualMatching (match.py:159-163)
  if (L == 1) {
    if ((rc = launch_mutual_matching(corr, B, (int)NA, (int)NB, 1, x0, rm, cp, cm, st))) return rc;
  } else {
    if (mm_fuse() && L == 2) {
      if ((rc = launch_mutual_matching_planar2(corr, B, (int)NA, (int)NB, x0, rm, cp, cm, st))) return rc;
    } else {
      if ((rc = launch_to_channels_last(corr, B, L, P, x0, st))) return rc;
      if ((rc = launch_mutual_matching(x0, B, (int)NA, (int)NB, L, x0, rm, cp, cm, st))) return rc;
    }
  }
  const int ch[4] = {L, 10, 10, 1};
  if (cv4) {
    // Conv4d layers (conv4d.py:64-138): per layer weight [3][co][ci][3][3][3] (the reference's
    // pre-permuted filter), bias [co]; the symmetric branch is the same stack with each filter's
    // position pairs exchanged (cv4d_layer_kernel swap)
    const float* cw[3][2];
    const float* q = nc_params;
    for (int l = 0; l < 3; ++l) {
      cw[l][0] = q;
      q += 81 * ch[l] * ch[l + 1];
      cw[l][1] = q;
      q += ch[l + 1];
    }
    for (int br = 0; br < (symmetric ? 2 : 1); ++br) {
      const float* in = x0;
      float* outs[3] = {x1, x2, br ? y2 : y1};
      for (int l = 0; l < 3; ++l) {
        if ((rc = launch_cv4d_layer(in, B, h, w, h, w, ch[l], ch[l + 1], cw[l][0], cw[l][1], br, outs[l], st)))
          return rc;
        in = outs[l];
      }
    }
  } else {
  // parameters per layer: conv1.weight [co][ci][3][3], conv1.bias [co], conv2.weight, conv2.bias
  const float* lw[3][4];
  {
    const float* q = nc_params;
    for (int l = 0; l < 3; ++l) {
      const int n = ch[l + 1] * ch[l] * 9;
      lw[l][0] = q; q += n;
      lw[l][1] = q; q += ch[l + 1];
      lw[l][2] = q; q += n;
      lw[l][3] = q; q += ch[l + 1];
    }
  }
  // branch 0: conv(x) (conv1 over the query positions a, conv2 over the support positions b);
  // branch 1 (symmetric mode): conv(x^T)^T = the same stack with the two roles swapped.  The two
  // branches are independent until their sum: branch 1 runs on the context's second stream
  // (its own intermediate buffers), so one branch's store-bound layers overlap the other's
  // MFMA-bound ones (CWT_MATCH_BRANCH_STREAMS=0: one after the other on the caller's stream)
  static const bool two_streams = !(getenv("CWT_MATCH_BRANCH_STREAMS") && getenv("CWT_MATCH_BRANCH_STREAMS")[0] == '0');
  const bool fork = symmetric && two_streams;
  float *x1b = x1, *x2b = x2;
  if (fork) {
    if (!saved && ((rc = ws(ctx, "match.x1b", (size_t)B * P * 10, &x1b)) ||
                   (rc = ws(ctx, "match.x2b", (size_t)B * P * 10, &x2b))))
      return rc;
    if (!ctx->aux) CWT_HIP(hipStreamCreateWithFlags(&ctx->aux, hipStreamNonBlocking));
    if (!ctx->ev_fork) CWT_HIP(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    if (!ctx->ev_join) CWT_HIP(hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
    CWT_HIP(hipEventRecord(ctx->ev_fork, st));
    CWT_HIP(hipStreamWaitEvent(ctx->aux, ctx->ev_fork, 0));
  }
  for (int br = 0; br < (symmetric ? 2 : 1); ++br) {
    const float* in = x0;
    const hipStream_t bst = (fork && br == 1) ? ctx->aux : st;
    float* outs[3] = {br && fork ? x1b : x1, br && fork ? x2b : x2,
                      br ? y2 : y1};
    if (saved)
      for (int l = 0; l < 3; ++l) outs[l] = S.o[br][l];
    for (int l = 0; l < 3; ++l) {
      const float* Wa = br ? lw[l][2] : lw[l][0];
      const float* ba = br ? lw[l][3] : lw[l][1];
      const float* Wb = br ? lw[l][0] : lw[l][2];
      const float* bb = br ? lw[l][1] : lw[l][3];
      if ((rc = launch_cp4d_layer(in, B, h, w, h, w, ch[l], ch[l + 1], Wa, ba, Wb, bb, outs[l], bst))) return rc;
      in = outs[l];
    }
  }
  if (fork) {
    CWT_HIP(hipEventRecord(ctx->ev_join, ctx->aux));
    CWT_HIP(hipStreamWaitEvent(st, ctx->ev_join, 0));
  }
  }
  if (saved) {  // y = o[0][2] (+ o[1][2]) into its own slot: the ReLU outputs stay for the backward
    CWT_HIP(hipMemcpyAsync(S.y, S.o[0][2], (size_t)B * P * 4, hipMemcpyDeviceToDevice, st));
    if (symmetric && (rc = launch_add_inplace(S.y, (const float*)S.o[1][2], B * P, st))) return rc;
    y1 = S.y;
  } else if (symmetric && !mm_fuse() && (rc = launch_add_inplace(y1, y2, B * P, st))) {
    return rc;
  }
  if ((rc = mm_ws(ctx, B, (int)NA, (int)NB, 1, &rm, &cp, &cm))) return rc;
  if (!saved && symmetric && mm_fuse()) {  // MutualMatching of y1 + y2 (the sum folded into its two passes)
    if ((rc = launch_mutual_matching_sum(y1, y2, B, (int)NA, (int)NB, corr2d, rm, cp, cm, st))) return rc;
  } else if ((rc = launch_mutual_matching(y1, B, (int)NA, (int)NB, 1, corr2d, rm, cp, cm, st))) {
    return rc;
  }
  if (weighted_v) {
    // attn = softmax(temp * corr2d, dim=-1); weighted_v = bmm(v, attn^T) (match.py:151-153),
    // here as tokens [B][NA][Cv] = attn . v
    const int ldp = (int)((NB + 31) & ~31L);  // zero-padded to whole 32-deep K tiles (gemm_f32d)
    float *pw, *vt;
    if ((rc = ws(ctx, "match.attn", (size_t)B * NA * ldp, &pw)) ||
        (rc = ws(ctx, "match.vt", (size_t)B * Cv * ldp, &vt)))
      return rc;
    if (saved) pw = S.attn;
    if ((rc = launch_match_softmax(corr2d, B, (int)NA, (int)NB, temp, ldp, pw, st))) return rc;
    if ((rc = launch_match_vt(v, B, (int)NB, Cv, ldp, vt, st))) return rc;
    if ((rc = readout_gemm(ctx, pw, vt, B, (int)NA, Cv, ldp, weighted_v, st))) return rc;
  }
  p.end();
  return 0;
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
static int mm_bwd_ws(cwt_ctx* ctx, int B, int NA, int NB, int C, MmBwdWs* w) {
  const long nrb = cdiv(NA, 16), bc = (long)B * C;
  int rc;
  if ((rc = ws(ctx, "mb.rowmax", bc * NA, &w->rowmax)) || (rc = ws(ctx, "mb.rowarg", bc * NA, &w->rowarg)) ||
      (rc = ws(ctx, "mb.colpv", bc * nrb * NB, &w->colpv)) || (rc = ws(ctx, "mb.colpi", bc * nrb * NB, &w->colpi)) ||
      (rc = ws(ctx, "mb.colmax", bc * NB, &w->colmax)) || (rc = ws(ctx, "mb.colarg", bc * NB, &w->colarg)) ||
      (rc = ws(ctx, "mb.srow", bc * NA, &w->srow)) || (rc = ws(ctx, "mb.scol", bc * NB, &w->scol)))
    return rc;
  return 0;
}

int cwt_match_corr_saved_floats(int B, int L, int h, int w, int symmetric, int readout, int64_t* n) {
  if (!n || B < 1 || L < 1 || L > CWT_MATCH_MAX_L || h < 1 || w < 1)
    return fail(CWT_EARG, "bad arguments (in_channel 1 .. CWT_MATCH_MAX_L = 32)");
  *n = (int64_t)match_saved_layout(nullptr, B, L, (long)h * w, symmetric, readout, nullptr);
  return 0;
}

int cwt_match_corr_forward_train(cwt_ctx* ctx, const float* corr, int B, int L, int h, int w, const float* nc_params,
                                 int symmetric, float temp, const float* v, int Cv, float* corr2d, float* weighted_v,
                                 float* saved, void* stream) {
  if (!saved) return fail(CWT_EARG, "saved is NULL");
  return match_corr_forward(ctx, corr, B, L, h, w, nc_params, symmetric, temp, v, Cv, corr2d, weighted_v, stream, false,
                            saved);
}

int cwt_match_corr_backward(cwt_ctx* ctx, const float* corr, int B, int L, int h, int w, const float* nc_params,
                            int symmetric, float temp, const float* v, int Cv, const float* saved,
                            const float* d_corr2d, const float* d_weighted_v, float* d_corr, float* d_params,
                            float* d_v, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(corr && nc_params && saved && d_params && B >= 1 && 1 <= L && L <= CWT_MATCH_MAX_L && h >= 1 && w >= 1,
            "bad arguments (in_channel 1 .. CWT_MATCH_MAX_L = 32)");
  CWT_CHECK(!d_weighted_v || (v && Cv >= 4 && Cv % 4 == 0), "d_weighted_v needs v and Cv % 4 == 0");
  CWT_CHECK(!d_v || d_weighted_v, "d_v needs d_weighted_v");
  CWT_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const long NA = (long)h * w, NB = NA, P = NA * NB, E = (long)B * P, ldp = ld32(NB);
  MatchSaved S;
  match_saved_layout((float*)saved, B, L, NA, symmetric, d_weighted_v != nullptr, &S);
  const int ch[4] = {L, 10, 10, 1};
  const float* lw[3][4];
  float* dlw[3][4];
  long np = 0;
  for (int l = 0; l < 3; ++l) {
    const long n = (long)ch[l + 1] * ch[l] * 9;
    const long off[4] = {np, np + n, np + n + ch[l + 1], np + 2 * n + ch[l + 1]};
    for (int q = 0; q < 4; ++q) {
      lw[l][q] = nc_params + off[q];
      dlw[l][q] = d_params + off[q];
    }
    np += 2 * (n + ch[l + 1]);
  }
  const size_t part_floats = (size_t)cp4d_wgrad_part_floats();
  float *g2d, *dy, *gA, *gm, *dx0, *part;
  int rc;
  if ((rc = ws(ctx, "mb.g2d", (size_t)E, &g2d)) || (rc = ws(ctx, "mb.dy", (size_t)E, &dy)) ||
      (rc = ws(ctx, "mb.gA", (size_t)E * 10, &gA)) || (rc = ws(ctx, "mb.gm", (size_t)E * 10, &gm)) ||
      (rc = ws(ctx, "mb.dx0", (size_t)E * L, &dx0)) || (rc = ws(ctx, "mb.part", part_floats, &part)))
    return rc;
  MmBwdWs mw;
  if ((rc = mm_bwd_ws(ctx, B, (int)NA, (int)NB, L, &mw))) return rc;
  Prof p(ctx, st, "match_corr_backward", 2.0 * 2.0 * B * P * 2 * (18.0 * L * 10 + 18.0 * 100 + 18.0 * 10),
         4.0 * B * P * (L + 44));
  CWT_HIP(hipMemsetAsync(d_params, 0, (size_t)np * 4, st));
  // the gradient at corr2d: the caller's, plus the softmax readout's (match.py:151-153)
  if (d_corr2d)
    CWT_HIP(hipMemcpyAsync(g2d, d_corr2d, (size_t)E * 4, hipMemcpyDeviceToDevice, st));
  else
    CWT_HIP(hipMemsetAsync(g2d, 0, (size_t)E * 4, st));
  if (d_weighted_v) {
    float* dA;
    if ((rc = ws(ctx, "mb.dA", (size_t)E, &dA))) return rc;
    for (int b = 0; b < B; ++b)  // dA = d_wv . v^T
      if ((rc = gemm_nt(ctx, d_weighted_v + (long)b * NA * Cv, v + (long)b * NB * Cv, (int)NA, (int)NB, Cv,
                        dA + (long)b * NA * NB, st)))
        return rc;
    if ((rc = launch_match_softmax_bwd(S.attn, (int)ldp, dA, (int)(B * NA), (int)NB, temp, 1, g2d, st))) return rc;
    if (d_v) {  // d_v[b] = attn[b]^T . d_wv[b]
      const long lda = ld32(NA);
      float *pt, *dwt;
      if ((rc = ws(ctx, "mb.PT", (size_t)B * ldp * lda, &pt)) || (rc = ws(ctx, "mb.dwvT", (size_t)B * Cv * lda, &dwt)))
        return rc;
      if ((rc = launch_match_vt(S.attn, B, (int)NA, (int)ldp, (int)lda, pt, st)) ||
          (rc = launch_match_vt(d_weighted_v, B, (int)NA, Cv, (int)lda, dwt, st)))
        return rc;
      for (int b = 0; b < B; ++b)
        if ((rc = gemm_nt(ctx, pt + (long)b * ldp * lda, dwt + (long)b * Cv * lda, (int)NB, Cv, (int)lda,
                          d_v + (long)b * NB * Cv, st)))
          return rc;
    }
  }
  // the second MutualMatching (match.py:162)
  if ((rc = launch_mutual_matching_bwd(S.y, g2d, B, (int)NA, (int)NB, 1, dy, mw, st))) return rc;
  // NeighConsensus: both branches see the same output gradient (y = branch 0 + branch 1); branch 1
  // applied conv2's filter over the a plane and conv1's over the b plane (match.py:75-80)
  for (int br = 0; br < (symmetric ? 2 : 1); ++br) {
    const float* gcur = dy;
    for (int l = 2; l >= 0; --l) {
      const int cin = ch[l], cout = ch[l + 1];
      const float* out = S.o[br][l];
      const float* in = l ? S.o[br][l - 1] : S.x0;
      if ((rc = launch_relu_mask(gcur, out, E * cout, gm, st))) return rc;
      const float* Wa = br ? lw[l][2] : lw[l][0];
      const float* Wb = br ? lw[l][0] : lw[l][2];
      float* dWa = br ? dlw[l][2] : dlw[l][0];
      float* dWb = br ? dlw[l][0] : dlw[l][2];
      if ((rc = launch_cp4d_wgrad(in, gm, B, h, w, h, w, cin, cout, part, part_floats, dWa, dWb, dlw[l][1], dlw[l][3],
                                  st)))
        return rc;
      if (l > 0) {
        if ((rc = launch_cp4d_dgrad(gm, B, h, w, h, w, cout, cin, Wa, Wb, gA, 0, st))) return rc;
        gcur = gA;
      } else if (d_corr) {
        if ((rc = launch_cp4d_dgrad(gm, B, h, w, h, w, cout, cin, Wa, Wb, dx0, br, st))) return rc;
      }
    }
  }
  // the first MutualMatching (match.py:160), back to the caller's channel-first layout
  if (d_corr) {
    if (L == 1) {
      if ((rc = launch_mutual_matching_bwd(corr, dx0, B, (int)NA, (int)NB, 1, d_corr, mw, st))) return rc;
    } else {
      float *xcl, *dxcl;
      if ((rc = ws(ctx, "mb.xcl", (size_t)E * L, &xcl)) || (rc = ws(ctx, "mb.dxcl", (size_t)E * L, &dxcl))) return rc;
      if ((rc = launch_to_channels_last(corr, B, L, P, xcl, st)) ||
          (rc = launch_mutual_matching_bwd(xcl, dx0, B, (int)NA, (int)NB, L, dxcl, mw, st)) ||
          (rc = launch_to_channels_first(dxcl, B, L, P, d_corr, st)))
        return rc;
    }
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
  const int ldp = (int)((NB + 31) & ~31L);  // zero-padded to whole 32-deep K tiles (gemm_f32d)
  float *pw, *vt;
  int rc;
  if ((rc = ws(ctx, "match.attn", (size_t)B * NA * ldp, &pw)) || (rc = ws(ctx, "match.vt", (size_t)B * Cv * ldp, &vt)))
    return rc;
  Prof p(ctx, st, "match_readout", 2.0 * B * NA * (double)NB * Cv, 4.0 * B * ((double)NA * NB * 2 + (double)NB * Cv));
  if ((rc = launch_match_softmax(corr2d, B, NA, NB, temp, ldp, pw, st))) return rc;
  if ((rc = launch_match_vt(v, B, NB, Cv, ldp, vt, st))) return rc;
  if ((rc = readout_gemm(ctx, pw, vt, B, NA, Cv, ldp, weighted_v, st))) return rc;
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
  const int ldp = (int)((NB + 31) & ~31L);
  const long E = (long)B * NA * NB;
  float *pw, *dA;
  int rc;
  if ((rc = ws(ctx, "match.attn", (size_t)B * NA * ldp, &pw)) || (rc = ws(ctx, "mb.dA", (size_t)E, &dA))) return rc;
  Prof p(ctx, st, "match_readout_backward", 2.0 * 2.0 * B * NA * (double)NB * Cv,
         4.0 * B * ((double)NA * NB * 4 + (double)(NA + NB) * Cv * 2));
  if (d_weighted_v) {
    // attn = softmax(temp corr2d) again (the forward's masked corr2d), dA = d_wv . v^T
    if ((rc = launch_match_softmax(corr2d, B, NA, NB, temp, ldp, pw, st))) return rc;
    for (int b = 0; b < B; ++b)
      if ((rc = gemm_nt(ctx, d_weighted_v + (long)b * NA * Cv, v + (long)b * NB * Cv, NA, NB, Cv,
                        dA + (long)b * NA * NB, st)))
        return rc;
    // d corr2d += temp P (dA - <P, dA>) (accumulating into the caller's gradient at corr2d)
    if ((rc = launch_match_softmax_bwd(pw, ldp, dA, B * NA, NB, temp, 1, d_corr2d, st))) return rc;
  }
  if (ig_mask && (rc = launch_match_zero_ig_cols(d_corr2d, ig_mask, B, NA, NB, st))) return rc;
  if (d_v) {  // d_v[b] = attn[b]^T . d_wv[b]
    const long lda = ld32(NA);
    float *pt, *dwt;
    if ((rc = ws(ctx, "mb.PT", (size_t)B * ldp * lda, &pt)) || (rc = ws(ctx, "mb.dwvT", (size_t)B * Cv * lda, &dwt)))
      return rc;
    if ((rc = launch_match_vt(pw, B, NA, ldp, (int)lda, pt, st)) ||
        (rc = launch_match_vt(d_weighted_v, B, NA, Cv, (int)lda, dwt, st)))
      return rc;
    for (int b = 0; b < B; ++b)
      if ((rc = gemm_nt(ctx, pt + (long)b * ldp * lda, dwt + (long)b * Cv * lda, NB, Cv, (int)lda,
                        d_v + (long)b * NB * Cv, st)))
        return rc;
  }
  p.end();
  return 0;
}

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
