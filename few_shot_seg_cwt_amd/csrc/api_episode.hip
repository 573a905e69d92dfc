// Episode entry points of libcwt.so (include/cwt.h): the inner adaptation loop and its fused tail,
// the CWT attention forward / backward / inference, the classifiers, metrics, losses and the SGD step.
#include <algorithm>
#include <cstdlib>

#include "ctx.h"
#include "tail_body.h"

using namespace cwt;

// CUs of the first device a plan is asked for (the persistent loop needs its workgroups co-resident);
// 0 where the query fails, and the next call asks again
static int adapt_cu_count() {
  static int cu = 0;
  int dev = 0;
  if (!cu && (hipGetDevice(&dev) != hipSuccess ||
              hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess))
    cu = 0;
  return cu;
}

// This call's plan of the inner loop (adapt_plan.h), made once: the launch, the profile names, the
// fused-tail decision and the workgroup count all read it
static AdaptPlan adapt_plan_for(cwt_ctx* ctx, int E, int n, int h, int w, int iters, const AdaptKnobs& kn) {
  return adapt_plan(E, n, h, w, iters, ctx->adapt_upw, adapt_cu_count(), kn);
}

// The loop's workspaces
static int adapt_ws(cwt_ctx* ctx, int E, int n, int h, int w, int S, AdaptWs* out) {
  void *fws, *lbl, *sc, *acc, *wb, *dargs;
  size_t b_f, b_lbl, b_sc, b_acc, b_wb, b_args;
  adapt_ws_sizes(E, n, h, w, S, &b_f, &b_lbl, &b_sc, &b_acc, &b_wb, &b_args);
  int rc;
  if ((rc = ensure_ws(ctx, "adapt.f", b_f, &fws)) || (rc = ensure_ws(ctx, "adapt.args", b_args, &dargs)) ||
      (rc = ensure_ws(ctx, "adapt.lbl", b_lbl, &lbl)) || (rc = ensure_ws(ctx, "adapt.sc", b_sc, &sc)) ||
      (rc = ensure_ws(ctx, "adapt.acc", b_acc, &acc)) ||  // [E][3][ADAPT_RMAX][512]
      (rc = ensure_ws(ctx, "adapt.wbuf", b_wb, &wb)))
    return rc;
  *out = AdaptWs{(float*)fws, (uint8_t*)lbl, (AdaptScalars*)sc, (float*)acc, (float*)wb, (AdaptDevArgs*)dargs};
  return 0;
}

// cwt_inner_adapt_tail fuses the tail into the loop's launch where the loop runs as the two-unit
// register form (EpisodePipeline's adapt context) in its product instantiation
static bool fused_tail_applies(const AdaptPlan& plan, const AdaptKnobs& kn) {
  const char* fz = getenv("CWT_FUSED_LOOP_TAIL");
  const char* tst = getenv("CWT_TAIL_STAMPS");
  return plan.persist && plan.form == PA_PAIR_REG && plan.E == 1 && kn.dbg == 0 && !(fz && fz[0] == '0') &&
         !(tst && tst[0] == '1');
}

extern "C" {

int cwt_inner_adapt_batch(cwt_ctx* ctx, const float* f_s, const int64_t* s_label, int E, int n, int h, int w, int C,
                          int S, float lr, int iters, float* W_inout, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(f_s && s_label && W_inout, "null buffer");
  CWT_CHECK(C == 512, "C must be 512");
  CWT_CHECK(E >= 1 && E <= 64 && n >= 1 && h >= 2 && w >= 2 && iters >= 0, "bad sizes");
  CWT_CHECK(S - 1 == 8 * (h - 1) && S - 1 == 8 * (w - 1), "need S-1 == 8*(h-1) == 8*(w-1)");
  CWT_HIP(hipSetDevice(ctx->device));
  AdaptWs aws;
  int rc;
  if ((rc = adapt_ws(ctx, E, n, h, w, S, &aws))) return rc;
  const AdaptPlan plan = adapt_plan_for(ctx, E, n, h, w, iters, adapt_knobs_from_env());
  const char* kname = adapt_plan_kernel_name(plan);
  // algorithmic work: per step 2 x (2*2*C*h*w*n) FLOPs; minimal bytes = f_s + labels once per step
  Prof p(ctx, (hipStream_t)stream,
         "inner_adapt x" + std::to_string(iters) + (E > 1 ? " E=" + std::to_string(E) : "") + " [" + kname + "]",
         (double)E * iters * 2.0 * (4.0 * C * h * w * n), (double)E * iters * ((double)n * h * w * C * 4 + (double)n * S * S),
         1);
  // the persistent kernel alone (no label prep / setup kernels): the launch rocprofv3 times
  Prof pk(ctx, (hipStream_t)stream, std::string("inner_adapt_kernel [") + kname + "]",
          (double)E * iters * 2.0 * (4.0 * C * h * w * n), (double)E * iters * ((double)n * h * w * C * 4 + (double)n * S * S),
          1, plan.persist);
  rc = launch_adapt(plan, f_s, s_label, S, lr, W_inout, aws, ctx->use_graph ? &ctx->adapt_graphs : nullptr,
                    ctx->status_dev, ctx->adapt_spin_limit, (hipStream_t)stream, pk.ev0(), pk.ev1());
  p.end();
  return rc;
}

int cwt_inner_adapt(cwt_ctx* ctx, const float* f_s, const int64_t* s_label, int n, int h, int w, int C, int S,
                    float lr, int iters, float* W_inout, void* stream) {
  return cwt_inner_adapt_batch(ctx, f_s, s_label, 1, n, h, w, C, S, lr, iters, W_inout, stream);
}

int cwt_inner_adapt_nway(cwt_ctx* ctx, const float* f_s, const int64_t* s_label, int n, int h, int w, int C, int S,
                         int N, int fg_idx, float tp, float lr, int iters, float* W_inout, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(f_s && s_label && W_inout, "null buffer");
  CWT_CHECK(C == 512, "C must be 512");
  CWT_CHECK(N >= 2 && N <= CWT_ADAPT_MAX_WAY, "N must be in [2, 64]");
  CWT_CHECK(fg_idx >= -1 && fg_idx < N, "fg_idx must be -1 or in [0, N)");
  CWT_CHECK(n >= 1 && h >= 2 && w >= 2 && iters >= 0, "bad sizes");
  CWT_CHECK(S - 1 == 8 * (h - 1) && S - 1 == 8 * (w - 1), "need S-1 == 8*(h-1) == 8*(w-1)");
  CWT_HIP(hipSetDevice(ctx->device));
  size_t b_lbl, b_sc, b_acc, b_wb;
  adapt_nway_ws_sizes(n, S, N, &b_lbl, &b_sc, &b_acc, &b_wb);
  void *lbl, *sc, *acc, *wb;
  int rc;
  if ((rc = ensure_ws(ctx, "nway.lbl", b_lbl, &lbl)) || (rc = ensure_ws(ctx, "nway.sc", b_sc, &sc)) ||
      (rc = ensure_ws(ctx, "nway.acc", b_acc, &acc)) || (rc = ensure_ws(ctx, "nway.wbuf", b_wb, &wb)))
    return rc;
  const AdaptNwayWs aws{(uint8_t*)lbl, sc, (unsigned long long*)acc, (float*)wb};
  // per step 2 x (2*N*C*h*w*n) FLOPs; minimal bytes = f_s + labels once per step
  Prof p(ctx, (hipStream_t)stream, "inner_adapt_nway x" + std::to_string(iters) + " N=" + std::to_string(N),
         (double)iters * 2.0 * (2.0 * N * C * h * w * n), (double)iters * ((double)n * h * w * C * 4 + (double)n * S * S), 1);
  rc = launch_adapt_nway(f_s, s_label, n, h, w, S, N, fg_idx, tp, lr, iters, W_inout, aws,
                         ctx->use_graph ? &ctx->adapt_nway_graphs : nullptr, (hipStream_t)stream);
  p.end();
  return rc;
}

int cwt_relabel_support(cwt_ctx* ctx, const float* logits, const int64_t* s_label, int B, int N, int h, int w, int S,
                        int idx_cls, int64_t* out, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(logits && s_label && out, "null buffer");
  CWT_CHECK(N >= 2 && N <= CWT_ADAPT_MAX_WAY, "N must be in [2, 64]");
  CWT_CHECK(idx_cls >= 0 && idx_cls < N, "idx_cls must be in [0, N)");
  CWT_CHECK(B >= 1 && B <= 64 && h >= 2 && w >= 2 && S >= 2 && (long)h * w <= (1L << 24) && S <= 32768,
            "need 1 <= B <= 64 and h, w, S >= 2");
  CWT_HIP(hipSetDevice(ctx->device));
  Prof p(ctx, (hipStream_t)stream, "relabel_support N=" + std::to_string(N), 10.0 * B * N * S * S,
         16.0 * B * S * S + 4.0 * B * N * h * w);
  const int rc = launch_relabel_support(logits, s_label, B, N, h, w, S, idx_cls, out, (hipStream_t)stream);
  p.end();
  return rc;
}

int cwt_seg_metrics_nway(cwt_ctx* ctx, const float* logits, const int64_t* target, int B, int N, int h, int w, int S,
                         int idx_cls, float* iut_out, double* ce_out, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(logits && target && iut_out, "null buffer");
  CWT_CHECK(N >= 2 && N <= CWT_ADAPT_MAX_WAY, "N must be in [2, 64]");
  CWT_CHECK(idx_cls >= 0 && idx_cls < N, "idx_cls must be in [0, N)");
  CWT_CHECK(B >= 1 && B <= 64 && h >= 2 && w >= 2 && S >= 2 && (long)h * w <= (1L << 24) && S <= 32768,
            "need 1 <= B <= 64 and h, w, S >= 2");
  CWT_HIP(hipSetDevice(ctx->device));
  void* cnt;
  int rc;
  if ((rc = ensure_ws(ctx, "nway.metrics", nway_metrics_ws_bytes(B), &cnt))) return rc;
  Prof p(ctx, (hipStream_t)stream, "seg_metrics_nway N=" + std::to_string(N), 30.0 * B * N * S * S,
         8.0 * B * S * S + 4.0 * B * N * h * w);
  rc = launch_seg_metrics_nway(logits, target, B, N, h, w, S, idx_cls, iut_out, ce_out, cnt, (hipStream_t)stream);
  p.end();
  return rc;
}

int cwt_normalize(cwt_ctx* ctx, const float* f, int B, int P_per_b, int C, float* out, const float* W0,
                  float* logits0, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(f && out && C == 512 && B >= 1 && P_per_b >= 1, "bad arguments");
  CWT_CHECK((W0 == nullptr) == (logits0 == nullptr), "W0 and logits0 go together");
  CWT_HIP(hipSetDevice(ctx->device));
  return launch_normalize(f, B, P_per_b, out, W0, logits0, (hipStream_t)stream);
}

size_t cwt_attention_saved_floats(int B, int hw, int C, int H) { return attention_saved_floats(B, hw, C, H); }

int cwt_attention_fwd_train(cwt_ctx* ctx, const float* q, const float* f, int B, int hw, int C, int H,
                            const float* w_qkvs, const float* fc_w, const float* fc_b, const float* ln_w,
                            const float* ln_b, float* out, float* saved, float attn_dropout, float out_dropout,
                            uint64_t seed, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(q && f && w_qkvs && fc_w && fc_b && ln_w && ln_b && out, "null buffer");
  CWT_CHECK(B >= 1 && B <= 4 && hw >= 1 && C == 512, "need 1 <= B <= 4, C == 512");
  CWT_CHECK(attn_dropout >= 0.f && attn_dropout < 1.f && out_dropout >= 0.f && out_dropout < 1.f,
            "dropout probabilities must lie in [0, 1)");
  CWT_HIP(hipSetDevice(ctx->device));
  float* buf;
  int rc;
  if ((rc = ws(ctx, "attn.ws", attention_ws_floats(B, hw, C, H), &buf))) return rc;
  // reference-formulation FLOPs: k/v projections 2 x 2*hw*C*C*H + QK^T/AV 2 x 2*H*2*hw*C
  Prof p(ctx, (hipStream_t)stream, "attention_fwd",
         (double)B * (2.0 * 2.0 * hw * C * C * H + 2.0 * 2.0 * H * 2.0 * hw * C),
         4.0 * ((double)B * hw * C + 2.0 * H * C * C + 2.0 * C), 1);
  rc = attention_fwd(q, f, B, hw, C, H, w_qkvs, fc_w, fc_b, ln_w, ln_b, out, saved, buf, (hipStream_t)stream,
                     attn_dropout, out_dropout, (unsigned long long)seed);
  p.end();
  return rc;
}

int cwt_attention_fwd(cwt_ctx* ctx, const float* q, const float* f, int B, int hw, int C, int H,
                      const float* w_qkvs, const float* fc_w, const float* fc_b, const float* ln_w, const float* ln_b,
                      float* out, float* saved, void* stream) {
  return cwt_attention_fwd_train(ctx, q, f, B, hw, C, H, w_qkvs, fc_w, fc_b, ln_w, ln_b, out, saved, 0.f, 0.f, 0,
                                 stream);
}

int cwt_attention_bwd_train(cwt_ctx* ctx, const float* q, const float* f, int B, int hw, int C, int H,
                            const float* w_qkvs, const float* fc_w, const float* fc_b, const float* ln_w,
                            const float* ln_b, const float* saved, const float* d_out, float* g_w_qkvs, float* g_fc_w,
                            float* g_fc_b, float* g_ln_w, float* g_ln_b, float attn_dropout, float out_dropout,
                            uint64_t seed, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(q && f && w_qkvs && fc_w && fc_b && ln_w && ln_b && saved && d_out, "null buffer");
  CWT_CHECK(g_w_qkvs && g_fc_w && g_fc_b && g_ln_w && g_ln_b, "null gradient buffer");
  CWT_CHECK(B >= 1 && B <= 4 && hw >= 1 && C == 512, "need 1 <= B <= 4, C == 512");
  CWT_CHECK(attn_dropout >= 0.f && attn_dropout < 1.f && out_dropout >= 0.f && out_dropout < 1.f,
            "dropout probabilities must lie in [0, 1)");
  CWT_HIP(hipSetDevice(ctx->device));
  float* buf;
  int rc;
  if ((rc = ws(ctx, "attn.bws", attention_bwd_ws_floats(B, hw, C, H), &buf))) return rc;
  return attention_bwd(q, f, B, hw, C, H, w_qkvs, fc_w, fc_b, ln_w, ln_b, saved, d_out, g_w_qkvs, g_fc_w, g_fc_b,
                       g_ln_w, g_ln_b, buf, (hipStream_t)stream, attn_dropout, out_dropout, (unsigned long long)seed);
}

int cwt_attention_bwd(cwt_ctx* ctx, const float* q, const float* f, int B, int hw, int C, int H,
                      const float* w_qkvs, const float* fc_w, const float* fc_b, const float* ln_w, const float* ln_b,
                      const float* saved, const float* d_out, float* g_w_qkvs, float* g_fc_w, float* g_fc_b,
                      float* g_ln_w, float* g_ln_b, void* stream) {
  return cwt_attention_bwd_train(ctx, q, f, B, hw, C, H, w_qkvs, fc_w, fc_b, ln_w, ln_b, saved, d_out, g_w_qkvs,
                                 g_fc_w, g_fc_b, g_ln_w, g_ln_b, 0.f, 0.f, 0, stream);
}

int cwt_attention_infer(cwt_ctx* ctx, const float* q, const float* f, int B, int hw, int C, int H,
                        const float* w_qkvs, const float* fc_w, const float* fc_b, const float* ln_w,
                        const float* ln_b, int64_t params_version, float* out, float* inv_norm, float* logits0,
                        void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(q && f && w_qkvs && fc_w && fc_b && ln_w && ln_b && out && inv_norm, "null buffer");
  CWT_CHECK(B >= 1 && B <= 4 && hw >= 1 && hw <= 512 * 32 && C == 512 && H == 4,
            "need 1 <= B <= 4, 1 <= hw <= 16384, C == 512, H == 4");
  CWT_HIP(hipSetDevice(ctx->device));
  const hipStream_t st = (hipStream_t)stream;
  float *fold, *buf;
  int rc;
  if ((rc = ws(ctx, "attn.fold", attention_fold_floats(C, H), &fold)) ||
      (rc = ws(ctx, "attn.iws", std::max(attention_infer_ws_floats(B, hw, C, H), (size_t)4 << 20), &buf)))
    return rc;
  Prof p(ctx, st, "attention_fwd", (double)B * (2.0 * 2.0 * hw * C * C * H + 2.0 * 2.0 * H * 2.0 * hw * C),
         4.0 * ((double)B * hw * C + 2.0 * H * C * C + 2.0 * C), 1);
  if (ctx->fold_w != w_qkvs || ctx->fold_fc != fc_w || ctx->fold_ver != params_version || ctx->fold_H != H) {
    if ((rc = attention_fold(w_qkvs, fc_w, C, H, fold, buf, (size_t)4 << 20, st))) return rc;
    ctx->fold_w = w_qkvs;
    ctx->fold_fc = fc_w;
    ctx->fold_ver = params_version;
    ctx->fold_H = H;
  }
  rc = attention_infer(q, f, B, hw, C, H, fold, fc_b, ln_w, ln_b, out, inv_norm, logits0, buf, st);
  p.end();
  return rc;
}

int cwt_episode_tail(cwt_ctx* ctx, const float* q, const float* f, int B, int h, int w, int S, const int64_t* q_label,
                     const float* w_qkvs, const float* fc_w, const float* fc_b, const float* ln_w, const float* ln_b,
                     int64_t params_version, float* out, float* logits, float* logits0, float* iut, double* ce,
                     float* iut0, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(q && f && q_label && w_qkvs && fc_w && fc_b && ln_w && ln_b && out && logits && logits0 && iut && ce && iut0,
            "null buffer");
  const int hw = h * w;
  CWT_CHECK(B >= 1 && B <= 4 && h >= 1 && w >= 1 && hw <= 512 * 32 && S - 1 == 8 * (h - 1) && S - 1 == 8 * (w - 1),
            "need 1 <= B <= 4, h*w <= 16384, S - 1 == 8 (h - 1) == 8 (w - 1)");
  CWT_HIP(hipSetDevice(ctx->device));
  const hipStream_t st = (hipStream_t)stream;
  constexpr int C = 512, H = 4;
  int cu = 0;
  CWT_HIP(hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, ctx->device));
  // G co-resident 512-thread workgroups (~54 KB of LDS each): the whole chip (up to 256)
  // on a context that runs alone; 64 on one whose inner loop shares the chip with another
  // stream's extractor pass (cwt_ctx_set_adapt_units >= 2: EpisodePipeline's adapt context).
  // CWT_TAIL_G for A/B
  int G = std::min(ctx->adapt_upw >= 2 ? 64 : 256, cu);
  if (const char* gs = getenv("CWT_TAIL_G")) G = std::max(1, std::min(atoi(gs), cu));
  float *fold, *buf;
  unsigned* cnt;
  int rc;
  if ((rc = ws(ctx, "attn.fold", attention_fold_floats(C, H), &fold)) ||
      (rc = ws(ctx, "tail.ws", std::max(episode_tail_ws_floats(B, hw, G), (size_t)4 << 20), &buf)) ||
      (rc = ws(ctx, "tail.cnt", episode_tail_cnt_words(), &cnt)))
    return rc;
  // phase record (the fold when the parameters changed + the launch) and the kernel alone
  Prof p(ctx, st, "post_loop_tail", (double)B * (2.0 * 2.0 * hw * C * C * H + 2.0 * 2.0 * H * 2.0 * hw * C),
         4.0 * ((double)B * hw * C + 2.0 * H * C * C + 2.0 * C), 1);
  Prof pk(ctx, st, "episode_tail_kernel", (double)B * (2.0 * 2.0 * hw * C * C * H + 2.0 * 2.0 * H * 2.0 * hw * C),
          4.0 * ((double)B * hw * C * 2 + 2.0 * H * C * C) + 9.0 * B * S * S, 1, true);
  if (ctx->fold_w != w_qkvs || ctx->fold_fc != fc_w || ctx->fold_ver != params_version || ctx->fold_H != H) {
    if ((rc = attention_fold(w_qkvs, fc_w, C, H, fold, buf, (size_t)4 << 20, st))) return rc;
    ctx->fold_w = w_qkvs;
    ctx->fold_fc = fc_w;
    ctx->fold_ver = params_version;
    ctx->fold_H = H;
  }
  if (ctx->tail_epoch > episode_tail_max_epoch(G) || ctx->tail_G != G) {  // fresh, wrapped, aborted or re-sized
    CWT_HIP(hipMemsetAsync(cnt, 0, episode_tail_cnt_words() * 4, st));
    ctx->tail_epoch = 0;
    ctx->tail_G = G;
  }
  // timing study (CWT_TAIL_STAMPS=1): per-workgroup phase stamps (cwt_debug_tail_stamps)
  unsigned long long* stamps = nullptr;
  if (getenv("CWT_TAIL_STAMPS") && getenv("CWT_TAIL_STAMPS")[0] == '1' &&
      (rc = ws(ctx, "tail.stamps", (size_t)G * 16, &stamps)))
    return rc;
  ctx->tail_stamp_G = stamps ? G : 0;
  if (pk.ev0()) CWT_HIP(hipEventRecord(pk.ev0(), st));
  rc = launch_episode_tail(q, f, B, hw, h, w, S, q_label, fold, fc_b, ln_w, ln_b, out, logits, logits0, iut, ce, iut0,
                           buf, cnt, ctx->tail_epoch++, G, ctx->adapt_spin_limit,
                           ctx->status_dev + 1, st, stamps);  // the tail's status word
  if (pk.ev1()) CWT_HIP(hipEventRecord(pk.ev1(), st));
  p.end();
  return rc;
}

int cwt_inner_adapt_tail(cwt_ctx* ctx, const float* f_s, const int64_t* s_label, int n, int h, int w, int C, int S,
                         float lr, int iters, float* W_inout, const float* f_q, const int64_t* q_label,
                         const float* w_qkvs, const float* fc_w, const float* fc_b, const float* ln_w,
                         const float* ln_b, int64_t params_version, float* out, float* logits, float* logits0,
                         float* iut, double* ce, float* iut0, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(f_s && s_label && W_inout && f_q && q_label && w_qkvs && fc_w && fc_b && ln_w && ln_b && out && logits &&
                logits0 && iut && ce && iut0,
            "null buffer");
  CWT_CHECK(C == 512, "C must be 512");
  CWT_CHECK(n >= 1 && h >= 2 && w >= 2 && iters >= 0 && h * w <= 512 * 32, "bad sizes");
  CWT_CHECK(S - 1 == 8 * (h - 1) && S - 1 == 8 * (w - 1), "need S-1 == 8*(h-1) == 8*(w-1)");
  CWT_HIP(hipSetDevice(ctx->device));
  // fused where the loop runs as the two-unit register form (EpisodePipeline's adapt context) in
  // its product instantiation; everything else (and CWT_FUSED_LOOP_TAIL=0) runs the two calls
  const AdaptKnobs knobs = adapt_knobs_from_env();
  const AdaptPlan plan = adapt_plan_for(ctx, 1, n, h, w, iters, knobs);
  if (!fused_tail_applies(plan, knobs)) {
    int rc = cwt_inner_adapt(ctx, f_s, s_label, n, h, w, C, S, lr, iters, W_inout, stream);
    if (rc) return rc;
    return cwt_episode_tail(ctx, W_inout, f_q, 1, h, w, S, q_label, w_qkvs, fc_w, fc_b, ln_w, ln_b, params_version, out,
                            logits, logits0, iut, ce, iut0, stream);
  }
  const hipStream_t st = (hipStream_t)stream;
  constexpr int H = 4;
  const int hw = h * w;
  const int G = plan.G;  // the tail runs on the loop's workgroups
  CWT_CHECK(G >= 1 && G <= 512, "fused tail: loop geometry");
  AdaptWs aws;
  int rc;
  if ((rc = adapt_ws(ctx, 1, n, h, w, S, &aws))) return rc;
  // the tail's (cwt_episode_tail), over the loop's G workgroups
  float *fold, *tws, *wq;
  unsigned* cnt;
  if ((rc = ws(ctx, "attn.fold", attention_fold_floats(C, H), &fold)) ||
      (rc = ws(ctx, "tail.ws", std::max(episode_tail_ws_floats(1, hw, G), (size_t)4 << 20), &tws)) ||
      (rc = ws(ctx, "tail.cnt", episode_tail_cnt_words(), &cnt)) || (rc = ws(ctx, "tail.wq", (size_t)G * 2 * C, &wq)))
    return rc;
  if (ctx->fold_w != w_qkvs || ctx->fold_fc != fc_w || ctx->fold_ver != params_version || ctx->fold_H != H) {
    if ((rc = attention_fold(w_qkvs, fc_w, C, H, fold, tws, (size_t)4 << 20, st))) return rc;
    ctx->fold_w = w_qkvs;
    ctx->fold_fc = fc_w;
    ctx->fold_ver = params_version;
    ctx->fold_H = H;
  }
  if (ctx->tail_epoch > episode_tail_max_epoch(G) || ctx->tail_G != G) {  // fresh, wrapped, aborted or re-sized
    CWT_HIP(hipMemsetAsync(cnt, 0, episode_tail_cnt_words() * 4, st));
    ctx->tail_epoch = 0;
    ctx->tail_G = G;
  }
  // this launch's stamp slot: {start (min), loop end (max), tail end (max)}, pre-set {~0, 0, 0}; only
  // when the profile records it (otherwise no memsets on the adapt stream and no stamp atomics: the
  // kernel guards every use of a null slot)
  constexpr int kFSlots = 4096;
  int slot = -1;
  unsigned long long* fst = nullptr;
  if (ctx->prof_level >= 1) {
    if (!ctx->fstamps) CWT_HIP(hipMalloc(&ctx->fstamps, (size_t)kFSlots * 3 * sizeof(unsigned long long)));
    slot = ctx->fstamp_next;
    ctx->fstamp_next = (ctx->fstamp_next + 1) % kFSlots;
    fst = ctx->fstamps + 3 * slot;
    CWT_HIP(hipMemsetAsync(fst, 0xFF, sizeof(unsigned long long), st));
    CWT_HIP(hipMemsetAsync(fst + 1, 0, 2 * sizeof(unsigned long long), st));
  }
  TailArgs ta;
  if ((rc = fill_episode_tail_args(W_inout, f_q, 1, hw, h, w, S, q_label, fold, fc_b, ln_w, ln_b, out, logits, logits0,
                                   iut, ce, iut0, tws, cnt, ctx->tail_epoch++, G, ctx->adapt_spin_limit,
                                   ctx->status_dev + 1, nullptr, &ta)))
    return rc;
  const FusedTail ft{&ta, wq, fst};
  const std::string kn = "adapt_persist_tail_kernel<5";
  const double lfl = (double)iters * 2.0 * (4.0 * C * h * w * n), lby = (double)iters * ((double)n * h * w * C * 4 + (double)n * S * S);
  const double tfl = 2.0 * 2.0 * hw * C * C * H + 2.0 * 2.0 * H * 2.0 * hw * C;
  Prof p(ctx, st, "inner_adapt x" + std::to_string(iters) + " [" + kn + "]", lfl, lby, 1);
  // the launch's loop part and tail part (its stamps; the events only order the read-back)
  Prof pk(ctx, st, "inner_adapt_kernel [" + kn + "]", lfl, lby, 1, true);
  if (pk.idx >= 0) ctx->recs[pk.idx].fslot = slot;
  rc = launch_adapt(plan, f_s, s_label, S, lr, W_inout, aws, nullptr, ctx->status_dev, ctx->adapt_spin_limit, st,
                    pk.ev0(), pk.ev1(), &ft);
  p.end();
  if (rc) return rc;
  for (const char* tn : {"post_loop_tail", "episode_tail_kernel"}) {
    Prof pt(ctx, st, tn, tfl, 4.0 * ((double)hw * C * 2 + 2.0 * H * C * C) + 9.0 * S * S, 1);
    pt.end();
    if (pt.idx >= 0) {
      ctx->recs[pt.idx].fslot = slot;
      ctx->recs[pt.idx].fpart = 1;
    }
  }
  return 0;
}

int cwt_classify_scaled(cwt_ctx* ctx, const float* W, const float* f, const float* inv_norm, int B, int P, int C,
                        float* logits, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(W && f && inv_norm && logits && C == 512 && B >= 1 && P >= 1, "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  return launch_classify_scaled(W, f, inv_norm, B, P, logits, (hipStream_t)stream);
}

int cwt_classify(cwt_ctx* ctx, const float* W, const float* f, int B, int P, int C, float* logits, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(W && f && logits && C >= 64 && C % 64 == 0 && C <= 2048 && B >= 1 && P >= 1, "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  return launch_classify_c(W, 2L * C, f, B, P, C, logits, (hipStream_t)stream);
}

int cwt_classify_bwd(cwt_ctx* ctx, const float* dlogits, const float* f, int B, int P, int C, float* dW,
                     void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(dlogits && f && dW && C == 512 && B >= 1 && P >= 1, "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  return launch_classify_bwd(dlogits, f, B, P, dW, (hipStream_t)stream);
}

int cwt_cos_classify(cwt_ctx* ctx, const float* x, int B, int P, int C, int n, float* weight, const float* g,
                     const float* bias, const float* scale, int mode, float* out, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(x && weight && scale && out && C == 512 && B >= 1 && P >= 1, "bad arguments");
  CWT_CHECK(n >= 1 && n <= 64, "n_classes must be in [1, 64]");
  CWT_CHECK(mode >= 0 && mode <= 3 && (!(mode & 1) || g), "mode: bit 0 WeightNorm (needs g), bit 1 weight_norm");
  CWT_HIP(hipSetDevice(ctx->device));
  float *weff, *vn;
  int rc;
  if ((rc = ws(ctx, "heads.weff", (size_t)n * C, &weff)) || (rc = ws(ctx, "heads.vnorm", 64, &vn))) return rc;
  hipStream_t st = (hipStream_t)stream;
  if ((rc = launch_cos_weight(weight, g, n, C, mode, weff, vn, st))) return rc;
  return launch_cos_cls_fwd(x, P, B, n, weff, bias, scale, out, st);
}

int cwt_cos_classify_bwd(cwt_ctx* ctx, const float* x, int B, int P, int C, int n, float* weight, const float* g,
                         const float* bias, const float* scale, int mode, const float* dscores, float* d_weight,
                         float* d_g, float* d_bias, float* d_scale, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(x && weight && scale && dscores && d_weight && C == 512 && B >= 1 && P >= 1, "bad arguments");
  CWT_CHECK(n >= 1 && n <= 64, "n_classes must be in [1, 64]");
  CWT_CHECK(mode >= 0 && mode <= 3 && (!(mode & 1) || (g && d_g)), "mode: bit 0 WeightNorm (needs g, d_g)");
  CWT_HIP(hipSetDevice(ctx->device));
  const int nb = cos_cls_bwd_blocks((long)B * P);
  float *weff, *vn, *part, *parts;
  int rc;
  if ((rc = ws(ctx, "heads.weff", (size_t)n * C, &weff)) || (rc = ws(ctx, "heads.vnorm", 64, &vn)) ||
      (rc = ws(ctx, "heads.part", (size_t)nb * n * C, &part)) ||
      (rc = ws(ctx, "heads.parts", (size_t)nb * n * 2, &parts)))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  // the forward's weight (for weight_norm the stored weight is already normalised: idempotent)
  if ((rc = launch_cos_weight(weight, g, n, C, mode, weff, vn, st))) return rc;
  return launch_cos_cls_bwd(x, P, B, n, weff, bias, scale, dscores, part, parts, mode, weight, g, vn, d_weight, d_g,
                            d_bias, d_scale, st);
}

int cwt_seg_metrics(cwt_ctx* ctx, const float* logits, const int64_t* target, int B, int h, int w, int S,
                    float* iut_out, double* ce_out, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(logits && target && iut_out && B >= 1 && B <= 64 && h >= 1 && w >= 1 && S >= 1, "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  void* cnt;
  int rc;
  if ((rc = ensure_ws(ctx, "metrics.cnt", (size_t)B * 256 * (2 * 6 * 4 + 2 * 8) + 16, &cnt))) return rc;
  return launch_seg_metrics(logits, target, B, h, w, S, iut_out, ce_out, (unsigned*)cnt, (hipStream_t)stream);
}

int cwt_seg_metrics_pair(cwt_ctx* ctx, const float* logits, const float* logits0, const int64_t* target, int B,
                         int h, int w, int S, float* iut_out, double* ce_out, float* iut0_out, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(logits && logits0 && target && iut_out && iut0_out && B >= 1 && B <= 64 && h >= 1 && w >= 1 && S >= 1,
            "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  void* cnt;
  int rc;
  if ((rc = ensure_ws(ctx, "metrics.cnt", (size_t)B * 256 * (2 * 6 * 4 + 2 * 8) + 16, &cnt))) return rc;
  return launch_seg_metrics(logits, target, B, h, w, S, iut_out, ce_out, (unsigned*)cnt, (hipStream_t)stream,
                            logits0, iut0_out);
}

int cwt_seg_ce_fwd_bwd(cwt_ctx* ctx, const float* logits, const int64_t* target, int B, int h, int w, int S,
                       float* loss_out, float* dlogits, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(logits && target && loss_out && dlogits && B >= 1, "bad arguments");
  CWT_CHECK(S - 1 == 8 * (h - 1) && S - 1 == 8 * (w - 1), "need S-1 == 8*(h-1) == 8*(w-1)");
  CWT_HIP(hipSetDevice(ctx->device));
  void *lbl, *sc, *num;
  int rc;
  if ((rc = ensure_ws(ctx, "ce.lbl", (size_t)B * S * S, &lbl)) || (rc = ensure_ws(ctx, "ce.sc", 8192, &sc)) ||
      (rc = ensure_ws(ctx, "ce.num", 64, &num)))
    return rc;
  return launch_seg_ce(logits, target, B, h, w, S, loss_out, dlogits, (uint8_t*)lbl, (AdaptScalars*)sc,
                       (double*)num, (hipStream_t)stream);
}

// the two loss heads' argument checks; nway: the head that takes N and idx_cls (its logits hold N floats a pixel)
static int check_head_args(cwt_ctx* ctx, const float* W, const float* f, int B, int h, int w, int C,
                           const int64_t* target, int S, int loss_type, const float* loss_out, bool nway, int N,
                           int idx_cls) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(W && f && target && loss_out, "null buffer");
  if (nway) {
    CWT_CHECK(N >= 2 && N <= CWT_ADAPT_MAX_WAY, "N must be in [2, 64]");
    CWT_CHECK(idx_cls >= 0 && idx_cls < N, "idx_cls must be in [0, N)");
  }
  CWT_CHECK(C >= 64 && C % 64 == 0 && C <= 2048, "C must be a multiple of 64, at most 2048");
  CWT_CHECK(B >= 1 && B <= 8, "need 1 <= B <= 8");
  CWT_CHECK(h >= 2 && w >= 2 && S >= 2 && (long)h * w <= (1L << 24) / (nway ? N : 1) && S <= 32768, "need h, w, S >= 2");
  CWT_CHECK(loss_type >= 0 && loss_type <= 2, "loss_type: 0 wt_ce, 1 wt_dc, 2 ce");
  return 0;
}

int cwt_seg_head_loss(cwt_ctx* ctx, const float* W, const float* f, int B, int h, int w, int C,
                      const int64_t* target, int S, int loss_type, float* loss_out, float* logits_out, float* d_f,
                      void* stream) {
  if (int bad = check_head_args(ctx, W, f, B, h, w, C, target, S, loss_type, loss_out, false, 2, 1)) return bad;
  CWT_HIP(hipSetDevice(ctx->device));
  const hipStream_t st = (hipStream_t)stream;
  float *lg, *sc;
  double* part;
  int rc;
  if ((rc = ws(ctx, "shl.logits", (size_t)B * 2 * h * w, &lg)) ||
      (rc = ws(ctx, "shl.part", seg_head_loss_part_doubles(B), &part)) ||
      (rc = ws(ctx, "shl.sc", seg_head_loss_sc_floats(B), &sc)))
    return rc;
  if (logits_out) lg = logits_out;
  // classifier 2 x 2*C per pixel (+ the same for d_f); per hi-res pixel two bilinear taps and a loss term, twice
  Prof p(ctx, st, "seg_head_loss", (double)B * h * w * 4.0 * C * (d_f ? 2 : 1) + 40.0 * B * S * S * (d_f ? 2 : 1),
         4.0 * B * h * w * C * (d_f ? 2 : 1) + 8.0 * B * S * S * (d_f ? 2 : 1));
  if ((rc = launch_classify_c(W, 0, f, B, h * w, C, lg, st))) return rc;
  rc = launch_seg_head_loss(W, lg, B, h, w, C, target, S, loss_type, loss_out, d_f, part, sc, st);
  p.end();
  return rc;
}

int cwt_seg_head_loss_nway(cwt_ctx* ctx, const float* W, const float* f, int B, int h, int w, int C, int N,
                           const int64_t* target, int S, int idx_cls, int loss_type, float* loss_out,
                           float* logits_out, float* d_f, float* iut_out, void* stream) {
  if (int bad = check_head_args(ctx, W, f, B, h, w, C, target, S, loss_type, loss_out, true, N, idx_cls)) return bad;
  CWT_HIP(hipSetDevice(ctx->device));
  const hipStream_t st = (hipStream_t)stream;
  float *lg, *sc, *pix = nullptr;
  void* part;
  int rc;
  if ((rc = ws(ctx, "shn.logits", (size_t)B * h * w * N, &lg)) ||
      (rc = ensure_ws(ctx, "shn.part", seg_head_loss_nway_part_bytes(B), &part)) ||
      (rc = ws(ctx, "shn.sc", seg_head_loss_sc_floats(B), &sc)) ||
      (d_f && (rc = ws(ctx, "shn.pix", seg_head_loss_nway_pix_floats(B, S), &pix))))
    return rc;
  // classifier N x 2*C per pixel (+ the same for d_f); per hi-res pixel N four-tap logits and exponentials, twice
  Prof p(ctx, st, "seg_head_loss_nway N=" + std::to_string(N),
         (double)B * h * w * 2.0 * N * C * (d_f ? 2 : 1) + 20.0 * N * B * S * S * (d_f ? 2 : 1),
         4.0 * B * h * w * C * (d_f ? 2 : 1) + 8.0 * B * S * S * (d_f ? 2 : 1) + (d_f ? 24.0 * B * S * S : 0.0));
  // the low-resolution logits are cwt_linear's own, pixel-major [B*h*w][N]
  if ((rc = cwt_linear(ctx, f, (int64_t)B * h * w, C, W, nullptr, N, 0, 0, lg, stream))) return rc;
  rc = launch_seg_head_loss_nway(W, lg, B, N, h, w, C, target, S, idx_cls, loss_type, loss_out, logits_out, d_f,
                                 iut_out, part, sc, pix, st);
  p.end();
  return rc;
}

int cwt_seg_metrics_nway_mix(cwt_ctx* ctx, const float* logits0, const float* logits1, double att_wt,
                             const int64_t* target, int B, int N, int h, int w, int S, int idx_cls, float* iut_out,
                             void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(logits0 && logits1 && target && iut_out, "null buffer");
  CWT_CHECK(N >= 2 && N <= CWT_ADAPT_MAX_WAY, "N must be in [2, 64]");
  CWT_CHECK(idx_cls >= 0 && idx_cls < N, "idx_cls must be in [0, N)");
  CWT_CHECK(B >= 1 && B <= 64 && h >= 2 && w >= 2 && S >= 2 && (long)h * w <= (1L << 24) && S <= 32768,
            "need 1 <= B <= 64 and h, w, S >= 2");
  CWT_CHECK(att_wt >= 0.0 && att_wt <= 1.0, "att_wt must be in [0, 1]");
  CWT_HIP(hipSetDevice(ctx->device));
  void* cnt;
  int rc;
  if ((rc = ensure_ws(ctx, "nway.metrics", nway_metrics_ws_bytes(B), &cnt))) return rc;
  Prof p(ctx, (hipStream_t)stream, "seg_metrics_nway_mix N=" + std::to_string(N), 120.0 * B * N * S * S,
         8.0 * B * S * S + 8.0 * B * N * h * w);
  rc = launch_seg_metrics_nway_mix(logits0, logits1, att_wt, target, B, N, h, w, S, idx_cls, iut_out, cnt,
                                   (hipStream_t)stream);
  p.end();
  return rc;
}

int cwt_iou_preds(cwt_ctx* ctx, const int64_t* preds, const int64_t* target, int64_t n, int num_classes,
                  int ignore_index, float* iut_out, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  // n == 0: an empty tensor has no storage (null pointers), and the kernel reads nothing
  CWT_CHECK(((preds && target) || n == 0) && iut_out && n >= 0 && num_classes >= 1 && num_classes <= 16,
            "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  unsigned* cnt;
  int rc;
  if ((rc = ws(ctx, "iou.cnt", 3 * 16, &cnt))) return rc;
  return launch_iou_preds(preds, target, n, num_classes, ignore_index, iut_out, cnt, (hipStream_t)stream);
}

int cwt_adapt_workgroups(cwt_ctx* ctx, int E, int n, int h, int w, int iters, int* G) {
  if (!ctx || !G || E < 1 || n < 1 || h < 2 || w < 2) return fail(CWT_EARG, "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  *G = adapt_plan_for(ctx, E, n, h, w, iters, adapt_knobs_from_env()).G;
  return 0;
}

int cwt_adapt_fuses_tail(cwt_ctx* ctx, int n, int h, int w, int iters, int* fused) {
  if (!ctx || !fused || n < 1 || h < 2 || w < 2 || iters < 0) return fail(CWT_EARG, "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  const AdaptKnobs kn = adapt_knobs_from_env();
  *fused = fused_tail_applies(adapt_plan_for(ctx, 1, n, h, w, iters, kn), kn) ? 1 : 0;
  return 0;
}

int cwt_sgd_step(cwt_ctx* ctx, float* param, const float* grad, float* momentum_buf, int64_t n, float lr,
                 float momentum, float weight_decay, int nesterov, int first_step, void* stream) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(param && grad && n >= 0, "bad arguments");
  CWT_CHECK(momentum == 0.f || momentum_buf, "momentum needs a buffer");
  CWT_HIP(hipSetDevice(ctx->device));
  return launch_sgd(param, grad, momentum_buf, n, lr, momentum, weight_decay, nesterov, first_step,
                    (hipStream_t)stream);
}

}  // extern "C"
