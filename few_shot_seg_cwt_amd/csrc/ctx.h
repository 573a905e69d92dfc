// Host side of libcwt.so shared by the api*.hip units and pretrain.hip: the context (workspace
// pool, profiler, per-context state), the fp32 GEMM helpers on the LDS-DMA conv body, and the conv
// layer and Winograd conv the extractor shares with the debug hooks (the extractor's geometry and
// plan: extract_plan.h; the architecture: backbone_arch.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/cwt.h"
#include "common.h"
#include "extract_plan.h"
#include "kernels.h"
#include "match_plan.h"  // ld32, the row padding the GEMM helpers below share with the match pass's plan

namespace cwt {

struct WsBuf {
  void* p = nullptr;
  size_t bytes = 0;
};

}  // namespace cwt

struct cwt_ctx {
  int device = 0;
  std::map<std::string, cwt::WsBuf> ws;
  size_t ws_total = 0;
  // optional per-launch profiling: events recorded on the caller's stream around each
  // instrumented launch (cwt_profile_enable); read back after a sync
  // 0 off, 1 phases + the bottleneck conv, 2 every launch, 3 also the Winograd form's sub-records
  // (run_wino_conv's wino_in / wino_gemm / wino_out: their event pairs add ~10 us of gaps inside each
  // Winograd conv's own bracket, so levels 1 and 2 leave them out)
  int prof_level = 0;
  struct Rec {
    std::string name;
    double flops, bytes;
    hipEvent_t e0, e1;
    int fslot = -1;  // a fused loop + tail launch: its slot in fstamps, and which part (0 loop, 1 tail)
    int fpart = 0;
  };
  // the fused loop + tail launches' realtime stamps ({start, loop end, tail end} per slot, a ring)
  unsigned long long* fstamps = nullptr;
  int fstamp_next = 0;
  std::vector<Rec> recs;
  std::vector<hipEvent_t> evpool;
  size_t ev_used = 0;
  // inner loop: captured graphs of the step sequence (disable with CWT_ADAPT_GRAPH=0)
  cwt::AdaptGraphCache adapt_graphs;
  cwt::AdaptGraphCache adapt_nway_graphs;  // the N-way loop's linear step graphs (adapt_nway.hip)
  bool use_graph = true;
  // conv arithmetic (CWT_CONV_ARITH_*): fp32 width on the bf16 matrix cores, operands split three
  // ways in registers (default, CWT_CONV=x6); bf16x3 over S-layout activations (CWT_CONV=x3s,
  // ~16-bit operands: a declared approximation); exact fp32 MFMA (CWT_CONV=f32)
  int conv_arith = CWT_CONV_ARITH_BF16X6;
  // persistent inner loop: units per workgroup (0 automatic, 1, 2), cwt_ctx_set_adapt_units
  int adapt_upw = 0;
  // asynchronous status word (cwt_ctx_status): mapped, coherent host memory the kernels OR
  // CWT_STATUS_* bits into (system-scope stores; written only on failure)
  unsigned* status_host = nullptr;
  unsigned* status_dev = nullptr;
  long adapt_spin_limit = 0;  // 0: the persistent loop's default bound (cwt_debug_adapt_spin_limit)
  // cwt_episode_tail's counters: this context's next launch number on them; ~0u = re-zero first
  unsigned tail_epoch = ~0u;
  int tail_G = 0;
  int tail_stamp_G = 0;  // workgroups of the last stamped tail launch (CWT_TAIL_STAMPS)
  // folded CWT weights of cwt_attention_infer (M_h = W_h^T W_h, P = [fc_h W_h]) and the
  // parameter identity they were folded from (buffers + the caller's version counter)
  const float* fold_w = nullptr;
  const float* fold_fc = nullptr;
  int64_t fold_ver = -1;
  int fold_H = 0;
  // a second stream for independent work inside one call (the symmetric NeighConsensus
  // branches), forked from and joined back into the caller's stream by events
  hipStream_t aux = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
};

namespace cwt {

// Profiling bracket: Prof p(ctx, st, name, flops, bytes); ... launches ...; p.end();
struct Prof {
  cwt_ctx* c;
  hipStream_t st;
  int idx = -1;
  // deferred form (Prof(..., level, true)): the record's two events, for a callee to record around one
  // launch with ev0() / ev1(), in place of the constructor / end()
  Prof(cwt_ctx* ctx, hipStream_t s, const std::string& name, double flops, double bytes, int level = 2,
       bool deferred = false)
      : c(ctx), st(s) {
    if (c->prof_level < level || !push(name, flops, bytes) || deferred) return;
    (void)hipEventRecord(c->recs[idx].e0, st);
  }
  void end() {
    if (idx >= 0) (void)hipEventRecord(c->recs[idx].e1, st);
    idx = -1;
  }
  hipEvent_t ev0() const { return idx >= 0 ? c->recs[idx].e0 : nullptr; }
  hipEvent_t ev1() const { return idx >= 0 ? c->recs[idx].e1 : nullptr; }

 private:
  // two events from the context's pool (grown on demand) and a new record holding them
  bool push(const std::string& name, double flops, double bytes) {
    hipEvent_t ev[2];
    for (int k = 0; k < 2; ++k) {
      if (c->ev_used == c->evpool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return false;
        c->evpool.push_back(e);
      }
      ev[k] = c->evpool[c->ev_used++];
    }
    c->recs.push_back({name, flops, bytes, ev[0], ev[1]});
    idx = (int)c->recs.size() - 1;
    return true;
  }
};

// The bracket of a planned record (ExtractRec, extract_plan.h; level 0: none at any profile level)
static inline Prof open_record(cwt_ctx* ctx, hipStream_t st, const ExtractRec& r) {
  return Prof(ctx, st, r.name, r.flops, r.bytes, r.level > 0 ? r.level : 1 << 30);
}

// The context's named workspace pool (api.hip): a buffer grows (256-B rounding, after a device
// synchronise) and never shrinks; ws<T> is ensure_ws with the size in elements of T
int ensure_ws(cwt_ctx* ctx, const std::string& name, size_t bytes, void** out);
template <class T>
int ws(cwt_ctx* ctx, const char* name, size_t count, T** out) {
  void* p = nullptr;
  const int rc = ensure_ws(ctx, name, count * sizeof(T), &p);
  *out = (T*)p;
  return rc;
}
int zero_line(cwt_ctx* ctx, const __bf16** out);

// exact-fp32 GEMMs on the LDS-DMA conv body (api.hip)
int gemm_f32d_mode();
bool gemm_f32d_ok(int M, int N, int K, const void* A, const void* Bm, const void* Cm, const void* res);
int gemm_f32d(cwt_ctx* ctx, const float* A, const float* Bm, int M, int N, int K, float* Cm, const float* bias,
              const float* res, int res_ld, hipStream_t st, int relu = 0);
int readout_gemm(cwt_ctx* ctx, const float* P, const float* vt, int B, int NA, int Cv, int ldp, float* out,
                 hipStream_t st);
int gemm_nt(cwt_ctx* ctx, const float* A, const float* W, int M, int N, int K, float* C, hipStream_t st);
// MutualMatching backward's scratch from the pool (api_match.hip; cwt_debug_mutual_matching_bwd shares it)
int mm_bwd_ws(cwt_ctx* ctx, int B, int NA, int NB, int C, MmBwdWs* w);

// A zeroed ConvSArgs / ConvArgs with the conv's geometry, M and K set (down2, conv_out_size: extract_plan.h)
template <class Args>
static inline Args conv_geom(int N, int Hi, int Wi, int Ci, int Co, int k, int stride, int pad, int dil) {
  Args a;
  memset(&a, 0, sizeof(a));
  a.N = N;
  a.Hi = Hi;
  a.Wi = Wi;
  a.Ci = Ci;
  a.Ho = conv_out_size(Hi, k, stride, pad, dil);
  a.Wo = conv_out_size(Wi, k, stride, pad, dil);
  a.Co = Co;
  a.kh = a.kw = k;
  a.stride = stride;
  a.pad = pad;
  a.dil = dil;
  a.M = N * a.Ho * a.Wo;
  a.K = k * k * Ci;
  return a;
}
static inline ConvSArgs conv_s_geom(int N, int Hi, int Wi, int Ci, int Co, int k, int stride, int pad, int dil) {
  return conv_geom<ConvSArgs>(N, Hi, Wi, Ci, Co, k, stride, pad, dil);
}

// ---- the extractor's conv layers (api_extract.hip), shared with the debug hooks ----
struct ConvLayer {
  int Ci = 0, Co = 0, k = 1, stride = 1, pad = 0, dil = 1;
  float* w = nullptr;  // device, packed [Co][k][k][Ci] (stem conv1: [ci][ky][kx][co])
  __bf16* w_s = nullptr;   // S-layout [Co][K/32][hi 32 | lo 32] of the same split (conv_x3s.hip)
  __bf16* w_l = nullptr;   // x6: the third term w - hi - lo, [Co][K/32][32] (exact in bf16)
  // x6 Winograd forms (stride-1 3x3, Ci >= 256; wino.hip): U = G g G^T per transformed
  // position, [P][Co][Ci] split like w_s / w_l; wino_s / wino_l F(2x2,3x3) (P = 16), wino4_s /
  // wino4_l F(4x4,3x3) (P = 36)
  __bf16* wino_s = nullptr;
  __bf16* wino_l = nullptr;
  __bf16* wino4_s = nullptr;
  __bf16* wino4_l = nullptr;
  __bf16* w_b = nullptr;   // plain bf16 [Co][K], K in packed_k64 order (bf16 conv stack; Ci % 64 == 0)
  float* scale = nullptr;
  float* shift = nullptr;
  float* bn = nullptr;  // [4][Co] gamma, beta, running_mean, running_var (training-mode BN)
};

// The input of a Winograd conv still in its producer's split-K partial planes (x = part
// [nsplit][N*H*W][Ci]): the input transform sums them and applies the producer's BN and ReLU itself
struct WinoSplitKSrc {
  int nsplit;
  const float *scale, *shift;
  int relu;
};

int force_conv_form(int prec, int bm, int bn, int Co, ConvPlan* p);
// One Winograd conv as wp plans it (wino_plan, extract_plan.h: geometry, GEMM plan, sub-records)
int run_wino_conv(cwt_ctx* ctx, const float* x, int Ci, int Co, const WinoPlan& wp, const __bf16* us, const __bf16* ul,
                  const float* scale, const float* shift, const float* res, int res_ld, int relu, float* y, int y_ld,
                  int y_off, hipStream_t st, const WinoSplitKSrc* sk = nullptr);

}  // namespace cwt
