// N-way support-set inner loop (reference pspnet.py:207-221 increment_inner_loop with
// model_util.py:76-97 Adapt_SegLoss / weighted_adpt_ce_loss), 2 <= N <= 64 classes.
//
// The 2-way loop (adapt.hip) keeps z1 - z0 in place of the logits and reduces dW[1] alone; with N
// classes neither shortcut exists.  One kernel per SGD step does, per (lo-res row pair r, 16-column
// block cb) and for every shot in turn:
//   f tile  -> LDS                          2 x 17 lo-res pixels (right halo included) x 512
//   z       = W . f                         wave v owns classes v, v+16, v+32, v+48 (W rows in
//                                           registers: the update W -= lr dW never leaves them)
//   z_hi    = bilinear(align_corners)(z)    a wave takes one 8 x 8 block of hi-res pixels (the
//                                           pixels that share their four lo-res corners)
//   p       = softmax_N(z_hi)               max-subtracted; classes >= N are never read
//   g_hi    = w_y (p - onehot_y)            y in [0, N), everything else is ignored
//   g_lo    = U^T g_hi                      four weighted 64-lane sums per (block, class) into
//                                           slots of their own, gathered in a fixed order
//   dW     += g_lo . f^T                    32 FMAs per lane per lo-res pixel
// The exchange between steps is the persistent 2-way loop's: 64-bit fixed-point integer atomics
// (exact, order-free: two calls on the same inputs give the same bits), scaled from
// max|f| * sum_p w_{y_p}; no float atomics anywhere, LDS included.  The next step's launch applies
// W <- W - lr / sum(w) * dW on the fly while it loads its W rows, so a step is one launch, and the
// launches are captured as a linear graph.  Fixed-order float partials were weighed and dropped:
// at N = 64 a workgroup's partial is 128 KB, and every workgroup of the next step would have to
// read all ~236 of them (30 MB per workgroup per step); the integer sums cost each workgroup one
// 256 KB read.  Three accumulator slots rotate (step s adds into s % 3, reads (s - 1) % 3 and
// zeroes (s + 1) % 3); no workgroup ever waits for another.
// Arithmetic: fp32 FMA throughout.  v_mfma_f32_16x16x4_f32 fits both GEMMs with the classes on
// the 16-row side; that form was not built, so the two were never measured against each other,
// and where the step's time goes has not been profiled (DESIGN.md section 3 holds what was
// measured: the whole loop against eager torch and against the 2-way step launches).
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace cwt {

constexpr int NWAY_C = 512;
constexpr int NWAY_T = 1024;               // threads per workgroup
constexpr int NWAY_NW = NWAY_T / 64;       // waves: class c belongs to wave c % 16
constexpr int NWAY_CB = 16;                // lo-res columns a workgroup owns
constexpr int NWAY_NC = NWAY_CB + 1;       // held columns (right halo)
constexpr int NWAY_NP = 2 * NWAY_NC;       // lo-res pixels of a tile
constexpr int NWAY_PREP_MAXBLK = 256;

struct NwayScalars {
  unsigned long long nfg, nvalid;  // pixels labelled fg_idx; pixels labelled in [0, N)
  float wfg;                       // float32(float32(bg / fg) ** tp); 1 for fg_idx = -1
  float lr_eff;                    // lr / sum_p w_{y_p}; 0 where every pixel is ignored; NaN for non-finite input
  double fx_scale, fx_inv;         // the exchange's fixed point (AdaptScalars, adapt.hip): sums below 2^58
};

struct NwayDevArgs {  // per-call pointers, read from device memory: one captured graph serves every call
  const float* f;     // NHWC [n][h][w][512]
  const float* w_in;  // [N][512]
  float* w_out;
};

// int64 labels -> u8 (y in [0, N) kept, everything else 255), per-block counts of fg_idx and of
// the kept labels, and the per-block max |f| as float bits (NaN / Inf above every finite value)
__global__ __launch_bounds__(1024) void nway_prep_kernel(const int64_t* __restrict__ lbl, long total, int N,
                                                         int fg_idx, uint8_t* __restrict__ out,
                                                         unsigned long long* __restrict__ part,
                                                         const float* __restrict__ f, long fcount,
                                                         unsigned* __restrict__ fpart) {
  unsigned mb = 0u;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < fcount / 4; i += (long)gridDim.x * blockDim.x) {
    const f32x4 v = ((const f32x4*)f)[i];
    mb = max(max(mb, __float_as_uint(fabsf(v[0]))), __float_as_uint(fabsf(v[1])));
    mb = max(max(mb, __float_as_uint(fabsf(v[2]))), __float_as_uint(fabsf(v[3])));
  }
  unsigned long long nf = 0, nv = 0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int64_t v = lbl[i];
    const bool keep = v >= 0 && v < N;
    out[i] = (uint8_t)(keep ? v : 255);
    nv += keep;
    nf += (keep && v == fg_idx);
  }
  for (int o = 32; o > 0; o >>= 1) {
    mb = max(mb, (unsigned)__shfl_xor((int)mb, o, 64));
    nf += __shfl_xor(nf, o, 64);
    nv += __shfl_xor(nv, o, 64);
  }
  __shared__ unsigned long long red[2][16];
  __shared__ unsigned fred[16];
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = nf;
    red[1][threadIdx.x >> 6] = nv;
    fred[threadIdx.x >> 6] = mb;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) {  // integer sums and maxima: order-free
      nf += red[0][i];
      nv += red[1][i];
      mb = max(mb, fred[i]);
    }
    part[2 * blockIdx.x] = nf;
    part[2 * blockIdx.x + 1] = nv;
    fpart[blockIdx.x] = mb;
  }
}

// One block: counts -> class weight, effective learning rate and fixed-point scale; the call's
// pointers; accumulator slot 0 zeroed
__global__ __launch_bounds__(NWAY_PREP_MAXBLK) void nway_setup_kernel(
    const unsigned long long* __restrict__ part, const unsigned* __restrict__ fpart, int nblk, int N, int fg_idx,
    float tp, float lr, NwayScalars* sc, NwayDevArgs* dargs, const float* f, const float* w_in, float* w_out,
    unsigned long long* zero, long nzero) {
  __shared__ unsigned long long red[2][NWAY_PREP_MAXBLK];
  __shared__ unsigned fred[NWAY_PREP_MAXBLK];
  const int t = threadIdx.x;
  red[0][t] = t < nblk ? part[2 * t] : 0ull;
  red[1][t] = t < nblk ? part[2 * t + 1] : 0ull;
  unsigned mb = t < nblk ? fpart[t] : 0u;
  for (int i = t; i < N * NWAY_C; i += NWAY_PREP_MAXBLK) {  // a non-finite W0 takes the exit of a non-finite f
    const unsigned wb = __float_as_uint(fabsf(w_in[i]));
    if (wb >= 0x7f800000u) mb = max(mb, wb);
  }
  fred[t] = mb;
  __syncthreads();
  for (int o = NWAY_PREP_MAXBLK / 2; o > 0; o >>= 1) {
    if (t < o) {
      red[0][t] += red[0][t + o];
      red[1][t] += red[1][t + o];
      fred[t] = max(fred[t], fred[t + o]);
    }
    __syncthreads();
  }
  if (t == 0) {
    const unsigned long long nfg = fg_idx >= 0 ? red[0][0] : 0ull, nvalid = red[1][0];
    sc->nfg = nfg;
    sc->nvalid = nvalid;
    const double fg = (double)nfg, bg = (double)(nvalid - nfg);
    float wfg = 1.f;
    if (fg_idx >= 0) {
      wfg = (float)(bg / fg);  // bincount ratio as float32 (inf with no fg pixel, NaN with no pixel at all)
      if (tp != 1.f) wfg = powf(wfg, tp);
    }
    sc->wfg = wfg;
    // sum_p w_{y_p}: the fg term only where a pixel carries it (0 pixels x an infinite weight is no term)
    const double sumw = bg + (nfg ? fg * (double)wfg : 0.0);
    // every pixel ignored: the reference's gradient is exactly zero, W stays as it is
    sc->lr_eff = nvalid ? (float)((double)lr / sumw) : 0.f;
    if (fred[0] >= 0x7f800000u) {
      sc->fx_scale = 0.0;
      sc->fx_inv = __builtin_nan("");
      sc->lr_eff = __builtin_nanf("");
    } else {
      const double bound = (double)__uint_as_float(fred[0]) * (sumw > 1.0 ? sumw : 1.0);
      const int k = (bound > 0.0 && bound < 1e300) ? 57 - ilogb(bound) : 0;
      sc->fx_scale = ldexp(1.0, k);
      sc->fx_inv = ldexp(1.0, -k);
    }
    dargs->f = f;
    dargs->w_in = w_in;
    dargs->w_out = w_out;
  }
  for (long i = t; i < nzero; i += NWAY_PREP_MAXBLK) zero[i] = 0ull;
}

struct NwayStepArgs {
  const NwayDevArgs* dargs;
  const uint8_t* lbl;  // [n][S][S]
  const NwayScalars* sc;
  const float* w_src;                  // W before the previous step's update, [N][512]; null at step 0 (dargs->w_in)
  const unsigned long long* acc_prev;  // the previous step's dW, [R][N][512] fixed point; null at step 0
  float* w_dst;                        // workgroup (0, 0) stores the current W here
  unsigned long long* acc_cur;         // this step's dW (zeroed)
  unsigned long long* acc_zero;        // the next step's slot: every workgroup zeroes its share
  int h, w, S, nshot, N, fg_idx, nrep;
};

// dynamic LDS of the step kernel for NJ class tiles of 16: the f tile, z and g_lo [pixel][class]
// (odd stride: the 8 x 8 blocks of a wave read eight pixels at once), and the adjoint's slots
// [block row][block column][corner][class]
template <int NJ>
struct NwayLds {
  static constexpr int NPAD = 16 * NJ, ZS = NPAD + 1;
  static constexpr int F = 0, Z = F + NWAY_NP * NWAY_C, G = Z + NWAY_NP * ZS, Q = G + NWAY_NP * ZS,
                       FLOATS = Q + 2 * NWAY_NC * 4 * NPAD;
};

__device__ __forceinline__ float nway_wave_sum(float v) { return wave_sum_dpp(v); }

template <int NJ>
__global__ __launch_bounds__(NWAY_T) void adapt_nway_step_kernel(NwayStepArgs a) {
  using L = NwayLds<NJ>;
  constexpr int C = NWAY_C, ZS = L::ZS, NPAD = L::NPAD;
  extern __shared__ float nway_lds[];
  float* fl = nway_lds + L::F;
  float* zl = nway_lds + L::Z;
  float* gl = nway_lds + L::G;
  float* ql = nway_lds + L::Q;
  const int t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const int cb = blockIdx.x, r = blockIdx.y, ncb = gridDim.x;
  const int N = a.N, S = a.S, h = a.h, w = a.w;
  const int x0 = cb * NWAY_CB;
  const int ncol = min(NWAY_NC, w - x0);         // held lo-res columns that exist
  const int nbx = cb == ncb - 1 ? ncol : NWAY_CB;  // owned block columns: the last one is hi-res column S-1 alone
  const int nby = r == h - 2 ? 2 : 1;              // the last row pair also owns hi-res row S-1
  const NwayScalars sc = *a.sc;
  const float* fimg = a.dargs->f;

  // ---- current W rows of this wave's classes: W_src - lr_eff * (sum of the previous step's replicas) ----
  float wr[NJ][8], dw[NJ][8];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = wv + NWAY_NW * j;
#pragma unroll
    for (int q = 0; q < 8; ++q) wr[j][q] = dw[j][q] = 0.f;
    if (c < N) {
      const float* ws = (a.w_src ? a.w_src : a.dargs->w_in) + (long)c * C + lane * 8;
      const f32x4 u = *(const f32x4*)ws, v = *(const f32x4*)(ws + 4);
      wr[j][0] = u[0]; wr[j][1] = u[1]; wr[j][2] = u[2]; wr[j][3] = u[3];
      wr[j][4] = v[0]; wr[j][5] = v[1]; wr[j][6] = v[2]; wr[j][7] = v[3];
      if (a.acc_prev) {
        long long s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int rr = 0; rr < a.nrep; ++rr) {
          const long long* ap = (const long long*)a.acc_prev + ((long)rr * N + c) * C + lane * 8;
#pragma unroll
          for (int q = 0; q < 8; ++q) s[q] += ap[q];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) wr[j][q] -= sc.lr_eff * (float)((double)s[q] * sc.fx_inv);
      }
      if ((cb | r) == 0 && a.w_dst) {
        float* wd = a.w_dst + (long)c * C + lane * 8;
        *(f32x4*)wd = f32x4{wr[j][0], wr[j][1], wr[j][2], wr[j][3]};
        *(f32x4*)(wd + 4) = f32x4{wr[j][4], wr[j][5], wr[j][6], wr[j][7]};
      }
    }
  }
  if (a.acc_zero) {  // this workgroup's share of the next step's slot
    const long total = (long)a.nrep * N * C, nwg = (long)gridDim.x * gridDim.y;
    const long wg = blockIdx.x + (long)gridDim.x * blockIdx.y;
    const long i0 = total * wg / nwg, i1 = total * (wg + 1) / nwg;
    for (long i = i0 + t; i < i1; i += NWAY_T) a.acc_zero[i] = 0ull;
  }

  const int yy = lane >> 3, xx = lane & 7;
  const float ly1 = (float)yy * 0.125f, ly0 = 1.f - ly1, lx1 = (float)xx * 0.125f, lx0 = 1.f - lx1;
  for (int k = 0; k < a.nshot; ++k) {
    // ---- the tile's f pixels; held columns past the image are zero ----
    const float* fk = fimg + (long)k * h * w * C;
    for (int i = t; i < NWAY_NP * (C / 4); i += NWAY_T) {
      const int p = i >> 7, q4 = i & 127;
      const int ri = p / NWAY_NC, xi = p - ri * NWAY_NC;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (xi < ncol) v = *(const f32x4*)(fk + ((long)(r + ri) * w + x0 + xi) * C + q4 * 4);
      *(f32x4*)(fl + p * C + q4 * 4) = v;
    }
    __syncthreads();
    // ---- z[p][c] = W[c] . f[p] ----
#pragma unroll 1
    for (int p = 0; p < NWAY_NP; ++p) {
      const f32x4 u = *(const f32x4*)(fl + p * C + lane * 8), v = *(const f32x4*)(fl + p * C + lane * 8 + 4);
      const float f8[8] = {u[0], u[1], u[2], u[3], v[0], v[1], v[2], v[3]};
      float s[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        s[j] = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) s[j] = fmaf(wr[j][q], f8[q], s[j]);
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) s[j] = nway_wave_sum(s[j]);
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        if (lane == 0) zl[p * ZS + wv + NWAY_NW * j] = s[j];  // classes >= N hold W = 0 and are never read
    }
    __syncthreads();
    // ---- hi-res pass: wave per 8 x 8 block (oy, ox); lane (yy, xx) is pixel (8 (r + oy) + yy, 8 (x0 + ox) + xx) ----
    const uint8_t* lk = a.lbl + (long)k * S * S;
    for (int b = wv; b < nby * nbx; b += NWAY_NW) {
      const int oy = b / nbx, ox = b - oy * nbx;
      const int Y = 8 * (r + oy) + yy, X = 8 * (x0 + ox) + xx;
      const bool in = Y < S && X < S;  // row S-1 / column S-1 are the only pixels of their blocks
      const int y = in ? lk[(long)Y * S + X] : 255;
      const bool live = y < N;
      // lo-res corners: rows oy, oy+1 and columns ox, ox+1, clamped where the far corner's weight is 0
      const float* z00 = zl + (oy * NWAY_NC + ox) * ZS;
      const float* z01 = zl + (oy * NWAY_NC + min(ox + 1, ncol - 1)) * ZS;
      const float* z10 = zl + (NWAY_NC + ox) * ZS;
      const float* z11 = zl + (NWAY_NC + min(ox + 1, ncol - 1)) * ZS;
      auto zh = [&](int c) { return ly0 * (lx0 * z00[c] + lx1 * z01[c]) + ly1 * (lx0 * z10[c] + lx1 * z11[c]); };
      float m = zh(0);
      for (int c = 1; c < N; ++c) m = fmaxf(m, zh(c));
      float se = 0.f;
      for (int c = 0; c < N; ++c) se += __expf(zh(c) - m);
      const float inv = 1.f / se;
      const float wy = live ? (y == a.fg_idx ? sc.wfg : 1.f) : 0.f;
      float* qb = ql + (oy * NWAY_NC + ox) * 4 * NPAD;
      for (int c = 0; c < N; ++c) {
        float g = 0.f;
        if (live) g = wy * (__expf(zh(c) - m) * inv - (c == y ? 1.f : 0.f));
        const float gx0 = lx0 * g, gx1 = lx1 * g;
        const float s00 = nway_wave_sum(ly0 * gx0), s01 = nway_wave_sum(ly0 * gx1);
        const float s10 = nway_wave_sum(ly1 * gx0), s11 = nway_wave_sum(ly1 * gx1);
        if (lane == 0) {
          qb[c] = s00;
          qb[NPAD + c] = s01;
          qb[2 * NPAD + c] = s10;
          qb[3 * NPAD + c] = s11;
        }
      }
    }
    __syncthreads();
    // ---- g_lo[ri][xi][c]: the blocks' corner sums in a fixed order ----
    for (int i = t; i < NWAY_NP * N; i += NWAY_T) {
      const int p = i / N, c = i - p * N;
      const int ri = p / NWAY_NC, xi = p - ri * NWAY_NC;
      float g = 0.f;
#pragma unroll
      for (int bx = 0; bx < 2; ++bx) {
        const int ox = xi - bx;
        if (ox < 0 || ox >= nbx) continue;
        // block row 0 reaches lo-res row ri with its corner row ri; block row 1 (hi-res row S-1) row 1 with weight 1
        g += ql[((0 * NWAY_NC + ox) * 4 + 2 * ri + bx) * NPAD + c];
        if (ri == 1 && nby == 2) g += ql[((1 * NWAY_NC + ox) * 4 + bx) * NPAD + c];
      }
      gl[p * ZS + c] = g;
    }
    __syncthreads();
    // ---- dW[c] += sum_p g_lo[p][c] f[p] ----
#pragma unroll 1
    for (int p = 0; p < NWAY_NP; ++p) {
      const f32x4 u = *(const f32x4*)(fl + p * C + lane * 8), v = *(const f32x4*)(fl + p * C + lane * 8 + 4);
      const float f8[8] = {u[0], u[1], u[2], u[3], v[0], v[1], v[2], v[3]};
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int c = wv + NWAY_NW * j;
        const float g = c < N ? gl[p * ZS + c] : 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) dw[j][q] = fmaf(g, f8[q], dw[j][q]);
      }
    }
    __syncthreads();  // the next shot's tile overwrites fl
  }

  // ---- exchange: exact integer adds into replica (workgroup % nrep) ----
  const long wg = blockIdx.x + (long)gridDim.x * blockIdx.y;
  unsigned long long* acc = a.acc_cur + (wg % a.nrep) * (long)N * C;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = wv + NWAY_NW * j;
    if (c < N) {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const long long iv = (long long)rint((double)dw[j][q] * sc.fx_scale);
        if (iv) atomicAdd(acc + (long)c * C + lane * 8 + q, (unsigned long long)iv);
      }
    }
  }
}

__global__ void adapt_nway_final_kernel(const float* w_src, const unsigned long long* acc, const NwayScalars* sc,
                                        const NwayDevArgs* dargs, int N, int nrep) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * NWAY_C) return;
  long long s = 0;
  for (int rr = 0; rr < nrep; ++rr) s += (long long)acc[(long)rr * N * NWAY_C + i];
  dargs->w_out[i] = w_src[i] - sc->lr_eff * (float)((double)s * sc->fx_inv);
}

static int nway_nj(int N) { return (N + 15) / 16; }

int adapt_nway_replicas(int N) {
  return std::max(1, 4 / nway_nj(N));  // 4, 2, 1, 1: 128-256 KB of replica reads per workgroup and step
}

void adapt_nway_ws_sizes(int n, int S, int N, size_t* lbl, size_t* sc, size_t* acc, size_t* wbuf) {
  *lbl = (size_t)n * S * S;
  *sc = 256 + NWAY_PREP_MAXBLK * (2 * sizeof(unsigned long long) + sizeof(unsigned));
  *acc = (size_t)3 * adapt_nway_replicas(N) * N * NWAY_C * sizeof(unsigned long long);
  *wbuf = (size_t)2 * N * NWAY_C * sizeof(float);
}

template <int NJ>
static int nway_launch_step(dim3 grid, hipStream_t st, const NwayStepArgs& a) {
  hipLaunchKernelGGL((adapt_nway_step_kernel<NJ>), grid, dim3(NWAY_T), NwayLds<NJ>::FLOATS * sizeof(float), st, a);
  CWT_LAUNCH_CHECK();
  return 0;
}

// The step kernels hold more LDS than the 64 KB a launch gets unasked.  The attribute belongs to
// the current device, so every call sets it for its own kernel (a host-side call, outside any capture)
template <int NJ>
static hipError_t nway_lds_attr() {
  return hipFuncSetAttribute((const void*)adapt_nway_step_kernel<NJ>, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)(NwayLds<NJ>::FLOATS * sizeof(float)));
}
static int nway_prepare(int N) {
  switch (nway_nj(N)) {
    case 1: CWT_HIP(nway_lds_attr<1>()); break;
    case 2: CWT_HIP(nway_lds_attr<2>()); break;
    case 3: CWT_HIP(nway_lds_attr<3>()); break;
    default: CWT_HIP(nway_lds_attr<4>()); break;
  }
  return 0;
}

static int enqueue_nway_steps(const AdaptNwayWs& ws, int n, int h, int w, int S, int N, int fg_idx, int iters,
                              hipStream_t st) {
  NwayStepArgs a;
  a.dargs = (const NwayDevArgs*)((char*)ws.sc + 128);
  a.lbl = ws.lbl;
  a.sc = (const NwayScalars*)ws.sc;
  a.h = h;
  a.w = w;
  a.S = S;
  a.nshot = n;
  a.N = N;
  a.fg_idx = fg_idx;
  a.nrep = adapt_nway_replicas(N);
  const long slot = (long)a.nrep * N * NWAY_C, wsz = (long)N * NWAY_C;
  const dim3 grid(cdiv(w - 1, NWAY_CB), h - 1);
  for (int s = 0; s < iters; ++s) {
    a.w_src = s ? ws.wbuf + ((s - 1) & 1) * wsz : nullptr;
    a.acc_prev = s ? ws.acc + ((s - 1) % 3) * slot : nullptr;
    a.w_dst = ws.wbuf + (s & 1) * wsz;
    a.acc_cur = ws.acc + (s % 3) * slot;
    a.acc_zero = ws.acc + ((s + 1) % 3) * slot;
    int rc;
    switch (nway_nj(N)) {
      case 1: rc = nway_launch_step<1>(grid, st, a); break;
      case 2: rc = nway_launch_step<2>(grid, st, a); break;
      case 3: rc = nway_launch_step<3>(grid, st, a); break;
      default: rc = nway_launch_step<4>(grid, st, a); break;
    }
    if (rc) return rc;
  }
  const int last = iters - 1;
  hipLaunchKernelGGL(adapt_nway_final_kernel, dim3(cdiv(N * NWAY_C, 256)), dim3(256), 0, st,
                     (const float*)(ws.wbuf + (last & 1) * wsz), (const unsigned long long*)(ws.acc + (last % 3) * slot),
                     a.sc, a.dargs, N, a.nrep);
  CWT_LAUNCH_CHECK();
  return 0;
}

int launch_adapt_nway(const float* f, const int64_t* lbl64, int n, int h, int w, int S, int N, int fg_idx, float tp,
                      float lr, int iters, float* W, const AdaptNwayWs& ws, AdaptGraphCache* cache, hipStream_t st) {
  const long total = (long)n * S * S;
  if (int rc = nway_prepare(N)) return rc;
  NwayScalars* sc = (NwayScalars*)ws.sc;
  NwayDevArgs* dargs = (NwayDevArgs*)((char*)ws.sc + 128);
  unsigned long long* part = (unsigned long long*)((char*)ws.sc + 256);
  unsigned* fpart = (unsigned*)(part + 2 * NWAY_PREP_MAXBLK);
  const int pblocks = (int)std::min<long>(NWAY_PREP_MAXBLK, cdiv(total, 1024));
  const int nrep = adapt_nway_replicas(N);
  hipLaunchKernelGGL(nway_prep_kernel, dim3(pblocks), dim3(1024), 0, st, lbl64, total, N, fg_idx, ws.lbl, part, f,
                     (long)n * h * w * NWAY_C, fpart);
  CWT_LAUNCH_CHECK();
  hipLaunchKernelGGL(nway_setup_kernel, dim3(1), dim3(NWAY_PREP_MAXBLK), 0, st, (const unsigned long long*)part,
                     (const unsigned*)fpart, pblocks, N, fg_idx, tp, lr, sc, dargs, f, (const float*)W, W, ws.acc,
                     iters > 0 ? (long)nrep * N * NWAY_C : 0L);
  CWT_LAUNCH_CHECK();
  if (iters <= 0) return 0;
  if (!cache) return enqueue_nway_steps(ws, n, h, w, S, N, fg_idx, iters, st);
  // one instantiated linear graph per (geometry, classes, workspace pointers)
  AdaptGraphCache::Entry key{N * 256 + nrep * 4096 * 16 + (fg_idx + 1), n, h, w, S, iters, nullptr, (const void*)ws.lbl,
                             (const void*)ws.sc, (const void*)ws.acc, (const void*)ws.wbuf, nullptr, nullptr};
  hipGraphExec_t exec = nullptr;
  for (auto& e : cache->entries)
    if (e.same(key)) exec = e.exec;
  if (!exec) {
    if (!cache->cap_stream) CWT_HIP(hipStreamCreateWithFlags(&cache->cap_stream, hipStreamNonBlocking));
    hipGraph_t g;
    CWT_HIP(hipStreamBeginCapture(cache->cap_stream, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue_nway_steps(ws, n, h, w, S, N, fg_idx, iters, cache->cap_stream);
    const hipError_t e2 = hipStreamEndCapture(cache->cap_stream, &g);
    if (rc) {
      if (e2 == hipSuccess) (void)hipGraphDestroy(g);
      return rc;
    }
    if (e2 != hipSuccess) return fail((int)e2, std::string("adapt_nway graph capture: ") + hipGetErrorString(e2));
    const hipError_t e3 = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e3 != hipSuccess) return fail((int)e3, std::string("adapt_nway graph instantiate: ") + hipGetErrorString(e3));
    key.exec = exec;
    cache->entries.push_back(key);
  }
  CWT_HIP(hipGraphLaunch(exec, st));
  return 0;
}

}  // namespace cwt
