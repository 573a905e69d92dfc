// fp32 width on the bf16 matrix cores (conv_igemm_x6, PREC 6 of the shared body, conv_body.h):
// the kernels, their launcher (the forms: conv_forms.h) and the weights' split.
#include "conv_body.h"
#include "conv_forms.h"

namespace cwt {

// fp32 width on the bf16 matrix cores: conv_igemm_f32d's activations split three ways in registers,
// the weights pre-split (conv_body.h, PREC 6)
template <int BM, int BN, int WAVES_M, int WAVES_N, int NSTG, int STAGE, int PF = 0>
__global__ __launch_bounds__(WAVES_M* WAVES_N * 64) void conv_igemm_x6(ConvSArgs a) {
  // a stage also holds the weights' lo plane: rings that would overflow the 160 KB of LDS lose a stage
  constexpr int STG = (BM + BN) * 128 + BN * 64;
  constexpr int NS = NSTG * STG <= 163840 ? NSTG : 163840 / STG;
  static_assert(NS >= 2, "x6: a two-stage ring must fit in LDS");
  conv_s_body<BM, BN, WAVES_M, WAVES_N, NS, 6, (PF | 8)>(a);
}

// fp32 packed weights [R][K] (K % 32 == 0) -> the x6 kernel's two weight planes: the S-layout
// line [R][K/32][32 hi | 32 mid] and the lo plane [R][K/32][32 lo] (hi = bf16_rne(w), mid =
// bf16_rne(w - hi), lo = w - hi - mid, exact)
__global__ void split_w3_kernel(const float* w, long n8, int K, __bf16* ws, __bf16* wl) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n8) return;
  const long e = idx * 8;  // 8 consecutive k of one row
  const long r = e / K;
  const int k = (int)(e - r * K);
  const f32x4 v0 = *(const f32x4*)(w + e), v1 = *(const f32x4*)(w + e + 4);
  bf16x8 h, m, l;
  split3_bf16(v0, v1, h, m, l);
  __bf16* sp = ws + (r * (K >> 5) + (k >> 5)) * 64 + (k & 31);
  *(bf16x8*)sp = h;
  *(bf16x8*)(sp + 32) = m;
  *(bf16x8*)(wl + (r * (K >> 5) + (k >> 5)) * 32 + (k & 31)) = l;
}

int launch_split_w3(const float* w, long R, int K, __bf16* ws, __bf16* wl, hipStream_t st) {
  if (K % 32) return fail(CWT_EARG, "split_w3: K % 32");
  const long n8 = R * K / 8;
  hipLaunchKernelGGL(split_w3_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, st, w, n8, K, ws, wl);
  CWT_LAUNCH_CHECK();
  return 0;
}

// Timing study (cwt_debug_occupy): each workgroup holds a whole CU -- 1024 threads and all 160 KB of
// its LDS -- and sleeps on the 100 MHz realtime clock for `ticks`, so a conv timed meanwhile on
// another stream gets the CUs the pipeline's resident inner loop leaves it.  Bounded by `ticks`.
__global__ __launch_bounds__(1024) void occupy_kernel(long ticks) {
  extern __shared__ char occ_lds[];
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  if (threadIdx.x == 0) occ_lds[0] = 0;
  while (__builtin_amdgcn_s_memrealtime() - t0 < (unsigned long long)ticks) __builtin_amdgcn_s_sleep(127);
}

int launch_occupy(int nwg, int us, hipStream_t st) {
  constexpr int kLds = 160 * 1024;
  static const hipError_t attr =
      hipFuncSetAttribute((const void*)occupy_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kLds);
  if (attr != hipSuccess) return fail(CWT_ESTATE, "occupy: 160 KB of dynamic LDS refused");
  hipLaunchKernelGGL(occupy_kernel, dim3(nwg), dim3(1024), kLds, st, (long)us * 100);
  CWT_LAUNCH_CHECK();
  return 0;
}

// The forms (plan.var on each tile, the timing-study forms among them) and their launcher:
// conv_forms.h.  p names a row directly (launch_conv_x3s has resolved it).
CWT_CONV_FAMILY(FamX6, conv_igemm_x6, true, false);

// A GEMM-shaped launch (kh = kw = 1, pad = 0: every K-tile reads the same pixels) takes its row's
// GEMM body (PF bit 256, conv_body.h) where the row has one (CWT_CONV_GEMM_ROWS_X6).
// CWT_X6_GEMM_BODY=0 keeps the general body: the A/B switch, read at every launch so that one
// process can run both.
static bool x6_gemm_body(const ConvSArgs& a) {
  if (a.kh != 1 || a.kw != 1 || a.pad != 0) return false;
  const char* v = getenv("CWT_X6_GEMM_BODY");
  return !(v && v[0] == '0');
}

void launch_tiles_x6(int stage, const ConvSArgs& a, const ConvPlan& p, dim3 grid, hipStream_t st) {
  const bool gemm = x6_gemm_body(a);
  with_stage<8>(stage, [&](auto s) { launch_form<FamX6, decltype(s)::value>(p, a, grid, st, gemm); });
}

}  // namespace cwt
