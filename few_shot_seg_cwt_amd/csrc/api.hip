// C ABI of libcwt.so (include/cwt.h has the contract of each entry point and the reference call site it
// replaces): error state, context, workspace pool, the exact-fp32 GEMM helpers and the profiler.  The
// other entry points: api_extract.hip, api_episode.hip, api_heads.hip, api_debug.hip.
#include <cstdlib>

#include "ctx.h"

namespace cwt {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

int ensure_ws(cwt_ctx* ctx, const std::string& name, size_t bytes, void** out) {
  WsBuf& b = ctx->ws[name];
  if (b.bytes < bytes) {
    if (b.p) {
      CWT_HIP(hipDeviceSynchronize());  // the old buffer may still be in use by queued work
      CWT_HIP(hipFree(b.p));
      ctx->ws_total -= b.bytes;
      b.p = nullptr;
      b.bytes = 0;
    }
    size_t nb = (bytes + 255) & ~(size_t)255;
    CWT_HIP(hipMalloc(&b.p, nb));
    b.bytes = nb;
    ctx->ws_total += nb;
  }
  *out = b.p;
  return 0;
}

// 256 B of zeros on the device (the LDS-DMA source of zero-padding taps in conv_x3s)
int zero_line(cwt_ctx* ctx, const __bf16** out) {
  const bool fresh = ctx->ws.find("zero") == ctx->ws.end();
  __bf16* p;
  int rc;
  if ((rc = ws(ctx, "zero", 128, &p))) return rc;
  if (fresh) CWT_HIP(hipMemset(p, 0, 256));
  *out = p;
  return 0;
}

// C = A . Bm^T (+ bias[N]) (+ res, pixel stride res_ld) in exact fp32 on the LDS-DMA conv body:
// conv_igemm_f32d as a 1x1 conv over M "pixels" (A's [M][K] rows) with the [N][K] weights Bm (a
// 1x1 conv's fp32 packing is plain row-major [Co][Ci]); the epilogue is fmaf(acc, 1, bias) then
// + res, the order of the separate bias / residual passes it replaces.  Shapes: K % 32 == 0,
// N % 64 == 0, 16-B aligned operands (gemm_f32d_ok); the rest stay on corr_gemm_kernel.
// Used for MatchNet's readout, cwt_linear and (with the measured plans of the heads' GEMM shapes,
// conv_plans_f32d.inc from tools/conv_s_sweep.py --configs 0:60:1, profiles/r4/sweeps) the
// WeightAverage GEMMs -- with the heuristic plans those measured slower than corr_gemm_kernel
// (0.72 against 0.66 ms for the layer-4 module, profiles/r4/run_i).  CWT_GEMM_F32D=0 keeps
// every GEMM on corr_gemm_kernel.
int gemm_f32d_mode() {
  static const int m = getenv("CWT_GEMM_F32D") ? atoi(getenv("CWT_GEMM_F32D")) : 1;
  return m;
}
bool gemm_f32d_ok(int M, int N, int K, const void* A, const void* Bm, const void* Cm, const void* res) {
  const bool on = gemm_f32d_mode() != 0;
  const uintptr_t al = (uintptr_t)A | (uintptr_t)Bm | (uintptr_t)Cm | (uintptr_t)res;
  return on && M >= 1 && K % 32 == 0 && N % 64 == 0 && N <= 8192 && (al & 15) == 0;
}

int gemm_f32d(cwt_ctx* ctx, const float* A, const float* Bm, int M, int N, int K, float* Cm, const float* bias,
              const float* res, int res_ld, hipStream_t st, int relu) {
  const bool fresh = ctx->ws.find("gemm.one") == ctx->ws.end();
  float *one, *zer, *part;
  const __bf16* zero;
  int rc;
  if ((rc = ws(ctx, "gemm.one", 8192, &one)) || (rc = ws(ctx, "gemm.zero", 8192, &zer)) || (rc = zero_line(ctx, &zero)))
    return rc;
  if (fresh) {
    CWT_HIP(hipMemsetD32((hipDeviceptr_t)one, 0x3f800000u, 8192));  // 1.0f
    CWT_HIP(hipMemset(zer, 0, 8192 * 4));
  }
  const ConvPlan pl = plan_conv_s(0, M, N, K);
  const size_t part_floats = pl.nsplit > 1 ? (size_t)pl.nsplit * M * N : 1;
  if ((rc = ws(ctx, "gemm.part", part_floats, &part))) return rc;
  ConvSArgs a = conv_s_geom(1, M, 1, K, N, 1, 1, 0, 1);  // a 1x1 conv over M pixels
  a.xs = (const __bf16*)A;
  a.ws = (const __bf16*)Bm;
  a.zero = zero;
  a.scale = one;
  a.shift = bias ? bias : zer;
  a.res = res;
  a.res_ld = res_ld;
  a.y = Cm;
  a.y_ld = N;
  a.relu = relu;
  return launch_conv_x3s(a, pl, 0, part, part_floats, st, 0);
}

// MatchNet's readout weighted_v[b] = attn[b] . v[b] as tokens [B][NA][Cv] = P[b] . vt[b]^T
int readout_gemm(cwt_ctx* ctx, const float* P, const float* vt, int B, int NA, int Cv, int ldp, float* out,
                 hipStream_t st) {
  if (!gemm_f32d_ok(NA, Cv, ldp, P, vt, out, nullptr)) return launch_gemm_abt(P, vt, B, NA, Cv, ldp, out, st);
  for (int b = 0; b < B; ++b) {
    int rc = gemm_f32d(ctx, P + (long)b * NA * ldp, vt + (long)b * Cv * ldp, NA, Cv, ldp, out + (long)b * NA * Cv,
                       nullptr, nullptr, 0, st);
    if (rc) return rc;
  }
  return 0;
}

// C [M][N] = A [M][K] . W [N][K]^T (K % 4 == 0): the exact-fp32 conv body where its shape rules
// allow (gemm_f32d), else corr_gemm_kernel
int gemm_nt(cwt_ctx* ctx, const float* A, const float* W, int M, int N, int K, float* C, hipStream_t st) {
  if (gemm_f32d_ok(M, N, K, A, W, C, nullptr)) return gemm_f32d(ctx, A, W, M, N, K, C, nullptr, nullptr, 0, st);
  if (K % 4) return fail(CWT_EARG, "gemm_nt: K % 4 != 0");
  return launch_gemm_abt(A, W, 1, M, N, K, C, st);
}

}  // namespace cwt

using namespace cwt;

extern "C" {

#ifndef CWT_SRC_HASH
#define CWT_SRC_HASH "unknown"
#endif
// the content hash of the HIP sources and headers this library was built from (build.py
// source_hash); _lib.load_library refuses a library whose hash differs from the tree's
const char* cwt_version(void) { return "libcwt 0.2 (gfx950) src=" CWT_SRC_HASH; }

const char* cwt_last_error(void) { return g_err.c_str(); }

int cwt_ctx_create(int device, cwt_ctx** out) {
  if (!out) return fail(CWT_EARG, "out is NULL");
  int n = 0;
  CWT_HIP(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return fail(CWT_EARG, "no such device");
  CWT_HIP(hipSetDevice(device));
  cwt_ctx* c = new cwt_ctx();
  c->device = device;
  const char* g = getenv("CWT_ADAPT_GRAPH");
  c->use_graph = !(g && g[0] == '0');
  const char* cv = getenv("CWT_CONV");
  const std::string mode = cv ? std::string(cv) : std::string("x6");
  if (mode != "x6" && mode != "x3s" && mode != "f32") {
    delete c;
    return fail(CWT_EARG, "CWT_CONV must be x6 (default), x3s or f32");
  }
  c->conv_arith = mode == "x6" ? CWT_CONV_ARITH_BF16X6 : mode == "x3s" ? CWT_CONV_ARITH_BF16X3 : CWT_CONV_ARITH_F32;
  if (hipHostMalloc((void**)&c->status_host, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
      hipHostGetDevicePointer((void**)&c->status_dev, c->status_host, 0) != hipSuccess) {
    if (c->status_host) (void)hipHostFree(c->status_host);
    delete c;
    return fail(CWT_ESTATE, "cwt_ctx_create: mapped status word");
  }
  for (int i = 0; i < 16; ++i) ((volatile unsigned*)c->status_host)[i] = 0u;
  *out = c;
  return 0;
}

int cwt_ctx_destroy(cwt_ctx* ctx) {
  if (!ctx) return 0;
  (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  for (auto& kv : ctx->ws)
    if (kv.second.p) (void)hipFree(kv.second.p);
  if (ctx->status_host) (void)hipHostFree(ctx->status_host);
  if (ctx->fstamps) (void)hipFree(ctx->fstamps);
  if (ctx->aux) (void)hipStreamDestroy(ctx->aux);
  if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
  if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
  delete ctx;
  return 0;
}

int cwt_ctx_status(cwt_ctx* ctx, uint32_t* status, int clear) {
  if (!ctx || !status) return fail(CWT_EARG, "null argument");
  // one word per failure source (plain stores from the kernels, no PCIe atomics): word 0 the inner
  // loop, word 1 the post-loop tail; the caller sees their OR
  volatile unsigned* w = ctx->status_host;
  const unsigned w0 = w[0], w1 = w[1];
  *status = w0 | w1;
  // the tail aborted, or the inner loop did (a fused tail then never ran its barriers): the tail's
  // counters are re-zeroed before the next tail
  if (w0 || w1) ctx->tail_epoch = ~0u;
  if (clear) {
    w[0] = 0u;
    w[1] = 0u;
  }
  return 0;
}

size_t cwt_workspace_bytes(cwt_ctx* ctx) { return ctx ? ctx->ws_total : 0; }

int cwt_ctx_set_conv_arith(cwt_ctx* ctx, int arith) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(arith == CWT_CONV_ARITH_BF16X3 || arith == CWT_CONV_ARITH_F32 || arith == CWT_CONV_ARITH_BF16X6,
            "arith must be CWT_CONV_ARITH_BF16X3 (0), CWT_CONV_ARITH_F32 (1) or CWT_CONV_ARITH_BF16X6 (2)");
  ctx->conv_arith = arith;
  return 0;
}

int cwt_ctx_set_adapt_units(cwt_ctx* ctx, int units_per_workgroup) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  CWT_CHECK(units_per_workgroup >= 0 && units_per_workgroup <= 3, "units per workgroup must be 0 (automatic), 1, 2 or 3");
  ctx->adapt_upw = units_per_workgroup;
  return 0;
}

int cwt_profile_enable(cwt_ctx* ctx, int on) {
  if (!ctx) return fail(CWT_EARG, "ctx is NULL");
  ctx->prof_level = on;
  if (on) {
    ctx->recs.clear();
    ctx->ev_used = 0;
  }
  return 0;
}

int cwt_profile_count(cwt_ctx* ctx) { return ctx ? (int)ctx->recs.size() : 0; }

int cwt_profile_record(cwt_ctx* ctx, int i, char* name, int name_len, double* flops, double* bytes, float* ms) {
  if (!ctx || i < 0 || i >= (int)ctx->recs.size()) return fail(CWT_EARG, "no such profile record");
  auto& r = ctx->recs[i];
  if (name && name_len > 0) {
    strncpy(name, r.name.c_str(), name_len - 1);
    name[name_len - 1] = 0;
  }
  if (flops) *flops = r.flops;
  if (bytes) *bytes = r.bytes;
  if (ms) {
    CWT_HIP(hipEventSynchronize(r.e1));
    if (r.fslot >= 0) {  // a fused loop + tail launch: its part from the kernel's realtime stamps (100 MHz)
      unsigned long long v[3];
      CWT_HIP(hipMemcpy(v, ctx->fstamps + 3 * r.fslot, sizeof(v), hipMemcpyDeviceToHost));
      const unsigned long long t0 = r.fpart ? v[1] : v[0], t1 = r.fpart ? v[2] : v[1];
      *ms = t1 > t0 ? (float)((double)(t1 - t0) * 1e-5) : 0.f;
    } else {
      CWT_HIP(hipEventElapsedTime(ms, r.e0, r.e1));
    }
  }
  return 0;
}

int cwt_cu_count(cwt_ctx* ctx, int* count) {
  if (!ctx || !count) return fail(CWT_EARG, "null argument");
  hipDeviceProp_t prop;
  CWT_HIP(hipGetDeviceProperties(&prop, ctx->device));
  *count = prop.multiProcessorCount;
  return 0;
}

int cwt_stream_create_masked(cwt_ctx* ctx, const uint32_t* mask, int mask_words, void** stream) {
  if (!ctx || !mask || !stream || mask_words < 1) return fail(CWT_EARG, "bad arguments");
  CWT_HIP(hipSetDevice(ctx->device));
  hipStream_t s;
  CWT_HIP(hipExtStreamCreateWithCUMask(&s, (uint32_t)mask_words, mask));
  *stream = (void*)s;
  return 0;
}

int cwt_stream_destroy(void* stream) {
  if (!stream) return fail(CWT_EARG, "stream is NULL");
  CWT_HIP(hipStreamDestroy((hipStream_t)stream));
  return 0;
}

}  // extern "C"
