// MatchNet's 4-D matching head and the MMN head around it (reference
// src/model/match.py:21-163, src/model/conv4d.py:11-62, src/model/mmn.py:11-71,
// src/model/msm/msm_func.py:50-104): the run_match_model chain of corr_forward,
//   MutualMatching -> NeighConsensus (symmetric, three CenterPivotConv4d + ReLU) ->
//   MutualMatching -> softmax(temp * corr2d) -> v . attn^T,
// over a correlation of NA = hA*wA query positions by NB = hB*wB support positions.
//
// Layout: a 4-D tensor x[B][C][hA][wA][hB][wB] (torch) is held channels-last,
// [B][a][b][C] with a = (ha, wa), b = (hb, wb) row-major: the C channels of one (a, b) pair (10 inside
// the consensus stack, 1 .. CWT_MATCH_MAX_L = 32 at its input) are one contiguous run, the b positions of one a a contiguous [hB][wB][C] image.
//
// CenterPivotConv4d (stride 1, kernel 3, padding 1) is two 2-D convolutions summed: conv1 over
// the a plane for every fixed b, conv2 over the b plane for every fixed a (conv4d.py:40-62).
// NeighConsensus in symmetric mode is conv(x) + conv(x^T)^T (match.py:75-80); the transposed
// branch is the same layer stack with the two convolutions' roles swapped (conv1 over b, conv2
// over a), so neither branch moves the 4-D tensor: the layer's kernels (cp4d.hip, planned by
// cp4d_plan.h) take the a-plane and b-plane weights as arguments.  This file holds the rest of the
// head: MutualMatching, the layout changes, the readout, Conv4d ('cv4'), the masks, the context
// descriptor and WeightAverage.
//
// Arithmetic: exact fp32 everywhere (VALU fmaf for the tiny-channel 4-D convs, the f32 MFMA
// GEMM of heads.hip for v . attn^T); MutualMatching uses the reference's operation order
// (corr * ((corr / (max_B + eps)) * (corr / (max_A + eps)))).
#include <cstdlib>

#include "../../include/cwt.h"
#include "common.h"
#include "kernels.h"

namespace cwt {

// ---- MutualMatching (match.py:34-53), per channel of x[B][NA][NB][C] (C = 1 or 2: the vector forms;
// any other C: the scalar forms below) ----
// row maxima (over b for each a) and per-row-block partial column maxima; a thread reads the C
// channels of a pair as one vector (both channels of a 128-B line in the same block)
constexpr int MM_RB = 16;  // rows of a per block (the scalar form)
constexpr int MM_RBV = 8;  // rows per block of the vector forms (450 workgroups at 60^2)
// PLANAR: x is the torch layout [B][C][NA][NB] (channel planes) instead of channels-last
template <int C, int RB = MM_RBV, bool PLANAR = false>
__global__ __launch_bounds__(256) void mm_rowcol_kernel(const float* __restrict__ x, int NA, int NB,
                                                        float* __restrict__ rowmax, float* __restrict__ colpart,
                                                        const float* __restrict__ x2 = nullptr) {
  // grid: (cdiv(NA, RB), B); rowmax [B*C][NA], colpart [B*C][cdiv(NA,RB)][NB]
  typedef float vec_t __attribute__((ext_vector_type(C)));
  const int b = blockIdx.y;
  const int a0 = blockIdx.x * RB;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const vec_t* xb = (const vec_t*)(x + (long)b * NA * NB * C);
  __shared__ float rm[4][RB][C];
  float rmax[RB][C];
#pragma unroll
  for (int r = 0; r < RB; ++r)
#pragma unroll
    for (int c = 0; c < C; ++c) rmax[r][c] = -INFINITY;
  for (int j = t; j < NB; j += 256) {
    float cm[C];
#pragma unroll
    for (int c = 0; c < C; ++c) cm[c] = -INFINITY;
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      const int a = a0 + r;
      if (a < NA) {
        vec_t v;
        if (PLANAR) {
#pragma unroll
          for (int c = 0; c < C; ++c) {
            const float pv = x[((long)(b * C + c) * NA + a) * NB + j];
            if (C == 1) v[0] = pv; else v[c] = pv;
          }
        } else {
          v = xb[(long)a * NB + j];
          if (C == 1 && x2) v[0] = v[0] + x2[(long)b * NA * NB + (long)a * NB + j];  // the symmetric branches' sum
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const float vc = C == 1 ? v[0] : v[c];
          cm[c] = fmaxf(cm[c], vc);
          rmax[r][c] = fmaxf(rmax[r][c], vc);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) colpart[((long)(b * C + c) * gridDim.x + blockIdx.x) * NB + j] = cm[c];
  }
#pragma unroll
  for (int r = 0; r < RB; ++r)
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float v = rmax[r][c];
      for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
      if (lane == 0) rm[wv][r][c] = v;
    }
  __syncthreads();
  if (t < RB * C) {
    const int r = t / C, c = t % C;
    if (a0 + r < NA)
      rowmax[(long)(b * C + c) * NA + a0 + r] = fmaxf(fmaxf(rm[0][r][c], rm[1][r][c]), fmaxf(rm[2][r][c], rm[3][r][c]));
  }
}

// column maxima from the row blocks' partials: block = 64 columns x 4 slices of the row blocks
// (the one-column-per-thread form ran 225 dependent loads per thread on 30 workgroups)
__global__ __launch_bounds__(256) void mm_colmax_kernel(const float* __restrict__ colpart, int nrb, int NB,
                                                        float* __restrict__ colmax) {
  __shared__ float part[4][64];
  const int bc = blockIdx.y;
  const int jl = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + jl;
  float m = -INFINITY;
  if (j < NB)
    for (int rb = sl; rb < nrb; rb += 4) m = fmaxf(m, colpart[((long)bc * nrb + rb) * NB + j]);
  part[sl][jl] = m;
  __syncthreads();
  if (sl == 0 && j < NB) colmax[(long)bc * NB + j] = fmaxf(fmaxf(part[0][jl], part[1][jl]), fmaxf(part[2][jl], part[3][jl]));
}

// y = x * ((x / (rowmax + eps)) * (x / (colmax + eps))); x, y [B][NA][NB][C] (y may alias x).
// grid (NA, B): block (a, b) walks the row's NB pairs (C channels each as one vector)
template <int C, bool PLANAR = false>  // PLANAR: x channel planes [B][C][NA][NB], y channels-last
__global__ __launch_bounds__(256) void mm_apply_kernel(const float* x, int NA, int NB,
                                                       const float* __restrict__ rowmax,
                                                       const float* __restrict__ colmax, float* y,
                                                       const float* __restrict__ x2 = nullptr) {
  typedef float vec_t __attribute__((ext_vector_type(C)));
  const float eps = 1e-5f;
  const int a = blockIdx.x, b = blockIdx.y;
  const long row = ((long)b * NA + a) * NB;
  const vec_t* xr = (const vec_t*)x + row;
  vec_t* yr = (vec_t*)y + row;
  float ra[C];
#pragma unroll
  for (int c = 0; c < C; ++c) ra[c] = rowmax[(long)(b * C + c) * NA + a] + eps;
  for (int j = threadIdx.x; j < NB; j += 256) {
    vec_t v;
    if (PLANAR) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float pv = x[((long)(b * C + c) * NA + a) * NB + j];
        if (C == 1) v[0] = pv; else v[c] = pv;
      }
    } else {
      v = xr[j];
      if (C == 1 && x2) v[0] = v[0] + x2[row + j];
    }
    vec_t o;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float vc = C == 1 ? v[0] : v[c];
      const float vb = vc / (colmax[(long)(b * C + c) * NB + j] + eps);  // corr4d_B: max over the A positions
      const float va = vc / ra[c];                                       // corr4d_A: max over the B positions
      if (C == 1) o[0] = vc * (va * vb); else o[c] = vc * (va * vb);
    }
    yr[j] = o;
  }
}

// any C (cwt_mutual_matching takes up to 64): the scalar forms
__global__ __launch_bounds__(256) void mm_apply_any_kernel(const float* x, long total, int NA, int NB, int C,
                                                       const float* __restrict__ rowmax,
                                                       const float* __restrict__ colmax, float* y) {
  const float eps = 1e-5f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C);
    const long p = i / C;
    const int j = (int)(p % NB);
    const long ab = p / NB;
    const int a = (int)(ab % NA), b = (int)(ab / NA);
    const int bc = b * C + c;
    const float v = x[i];
    const float vb = v / (colmax[(long)bc * NB + j] + eps);  // corr4d_B: max over the A positions
    const float va = v / (rowmax[(long)bc * NA + a] + eps);  // corr4d_A: max over the B positions
    y[i] = v * (va * vb);
  }
}
__global__ __launch_bounds__(256) void mm_rowcol_any_kernel(const float* __restrict__ x, int NA, int NB, int C,
                                                        float* __restrict__ rowmax, float* __restrict__ colpart) {
  // grid: (cdiv(NA, MM_RB), B * C); rowmax [B*C][NA], colpart [B*C][cdiv(NA,MM_RB)][NB]
  const int bc = blockIdx.y, b = bc / C, c = bc - b * C;
  const int a0 = blockIdx.x * MM_RB;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const float* xb = x + (long)b * NA * NB * C + c;
  __shared__ float rm[4][MM_RB];
  float rmax[MM_RB];
#pragma unroll
  for (int r = 0; r < MM_RB; ++r) rmax[r] = -INFINITY;
  for (int j = t; j < NB; j += 256) {
    float cm = -INFINITY;
#pragma unroll
    for (int r = 0; r < MM_RB; ++r) {
      const int a = a0 + r;
      if (a < NA) {
        const float v = xb[((long)a * NB + j) * C];
        cm = fmaxf(cm, v);
        rmax[r] = fmaxf(rmax[r], v);
      }
    }
    colpart[((long)bc * gridDim.x + blockIdx.x) * NB + j] = cm;
  }
#pragma unroll
  for (int r = 0; r < MM_RB; ++r) {
    float v = rmax[r];
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    if (lane == 0) rm[wv][r] = v;
  }
  __syncthreads();
  if (t < MM_RB && a0 + t < NA)
    rowmax[(long)bc * NA + a0 + t] = fmaxf(fmaxf(rm[0][t], rm[1][t]), fmaxf(rm[2][t], rm[3][t]));
}

// x [B][C][P] (channel planes) -> y [B][P][C] (channels last)
__global__ void to_channels_last_kernel(const float* __restrict__ x, int B, int C, long P, float* __restrict__ y) {
  const long total = (long)B * C * P;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C);
    const long p = (i / C) % P;
    const long b = i / ((long)C * P);
    y[i] = x[(b * C + c) * P + p];
  }
}

// y += x (element count n)
__global__ void add_inplace_kernel(float* __restrict__ y, const float* __restrict__ x, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) y[i] += x[i];
}

// softmax(temp * corr2d) over b, one workgroup per row a, written with row stride ldp (the pad
// columns zero): P[B][NA][ldp]
__global__ __launch_bounds__(256) void match_softmax_kernel(const float* __restrict__ corr, int NA, int NB, float temp,
                                                            int ldp, float* __restrict__ P) {
  const long row = blockIdx.x;  // b * NA + a
  const float* cr = corr + row * NB;
  float* pr = P + row * ldp;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  __shared__ float red[4];
  float m = -INFINITY;
  for (int j = t; j < NB; j += 256) m = fmaxf(m, cr[j] * temp);
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if (lane == 0) red[wv] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float s = 0.f;
  for (int j = t; j < NB; j += 256) s += __expf(cr[j] * temp - m);
  s = wave_sum_dpp(s);
  if (lane == 0) red[wv] = s;
  __syncthreads();
  const float inv = 1.f / ((red[0] + red[1]) + (red[2] + red[3]));
  for (int j = t; j < ldp; j += 256) pr[j] = j < NB ? __expf(cr[j] * temp - m) * inv : 0.f;
}

// v tokens [B][NB][C] -> vT [B][C][ldp] (pad columns zero)
__global__ __launch_bounds__(256) void match_vt_kernel(const float* __restrict__ v, int NB, int C, int ldp,
                                                       float* __restrict__ vt) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z;
  const int j0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int r = ty; r < 32; r += 8) {
    const int j = j0 + r, c = c0 + tx;
    tile[r][tx] = (j < NB && c < C) ? v[((long)b * NB + j) * C + c] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int c = c0 + r, j = j0 + tx;
    if (c < C && j < ldp) vt[((long)b * C + c) * ldp + j] = tile[tx][r];
  }
}

// ---- Conv4d ('cv4', src/model/conv4d.py:64-138) + ReLU, one NeighConsensus layer ----
// x, y channels last [B][hA wA][hB wB][C].  W is the reference's pre-permuted filter
// [k0][co][ci][k1][k2][k3] (Conv4d permutes it in its constructor), kernel 3, zero padding 1:
// y(i,j,k,l) = relu(bias + sum W[d0][co][ci][d1][d2][d3] x(i+d0-1, j+d1-1, k+d2-1, l+d3-1)), the
// per-slice conv3d sum of conv_4d.  swap = 1 applies the filter with (d0,d1) and (d2,d3)
// exchanged: conv(x^T)^T of the symmetric mode as one pass.  One thread per output position,
// every output channel; the filter tap-major in LDS (uniform broadcast reads).  fp32 VALU.
template <int CIN, int COUT>
__global__ __launch_bounds__(256) void cv4d_layer_kernel(const float* __restrict__ x, int B, int hA, int wA, int hB,
                                                         int wB, const float* __restrict__ W,
                                                         const float* __restrict__ bias, int swap,
                                                         float* __restrict__ y) {
  __shared__ float wl[81][CIN][COUT];
  for (int e = threadIdx.x; e < 81 * CIN * COUT; e += 256) {
    // e walks the stored layout [d0][co][ci][d1][d2][d3]
    const int d3 = e % 3, d2 = (e / 3) % 3, d1 = (e / 9) % 3;
    const int ci = (e / 27) % CIN, co = (e / (27 * CIN)) % COUT, d0 = e / (27 * CIN * COUT);
    const int tap = swap ? ((d2 * 3 + d3) * 3 + d0) * 3 + d1 : ((d0 * 3 + d1) * 3 + d2) * 3 + d3;
    wl[tap][ci][co] = W[e];
  }
  __syncthreads();
  const long NB = (long)hB * wB, P = (long)hA * wA * NB, total = (long)B * P;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
    const int b = (int)(q / P);
    const long pos = q - (long)b * P;
    const int l = (int)(pos % wB), k = (int)((pos / wB) % hB);
    const long pa = pos / NB;
    const int j = (int)(pa % wA), i = (int)(pa / wA);
    float acc[COUT];
#pragma unroll
    for (int co = 0; co < COUT; ++co) acc[co] = bias[co];
    for (int d0 = 0; d0 < 3; ++d0) {
      const int ii = i + d0 - 1;
      if ((unsigned)ii >= (unsigned)hA) continue;
      for (int d1 = 0; d1 < 3; ++d1) {
        const int jj = j + d1 - 1;
        if ((unsigned)jj >= (unsigned)wA) continue;
        for (int d2 = 0; d2 < 3; ++d2) {
          const int kk = k + d2 - 1;
          if ((unsigned)kk >= (unsigned)hB) continue;
#pragma unroll
          for (int d3 = 0; d3 < 3; ++d3) {
            const int ll = l + d3 - 1;
            if ((unsigned)ll >= (unsigned)wB) continue;
            const float* xp = x + ((long)b * P + ((long)ii * wA + jj) * NB + (long)kk * wB + ll) * CIN;
            const int tap = ((d0 * 3 + d1) * 3 + d2) * 3 + d3;
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci) {
              const float xv = xp[ci];
#pragma unroll
              for (int co = 0; co < COUT; ++co) acc[co] = fmaf(wl[tap][ci][co], xv, acc[co]);
            }
          }
        }
      }
    }
    float* yp = y + q * COUT;
#pragma unroll
    for (int co = 0; co < COUT; ++co) yp[co] = fmaxf(acc[co], 0.f);
  }
}

// ---- Spatial context descriptor (src/model/base/spatial_context.py:13-65) ----
// x tokens [B][h][w][C]; g [B][h w][ldg]: g[o] = <x(p), x(p + offset o)> over the k x k window
// (zero outside the map), then featureL2Norm: g / sqrt(sum g^2 + 1e-6); columns k^2 .. ldg-1 zero.
// One workgroup per pixel: the pixel's feature in LDS, each wave one window offset at a time
// (lanes over channels, coalesced), the window in LDS for the norm.
constexpr int SCE_MAXK2 = 32 * 32;
__global__ __launch_bounds__(256) void sce_descriptor_kernel(const float* __restrict__ x, int h, int w, int C, int k,
                                                             int ldg, float* __restrict__ g) {
  extern __shared__ float sm_sce[];  // q [C], win [k*k]
  float* q = sm_sce;
  float* win = sm_sce + C;
  const long pix = blockIdx.x;  // b * h * w + y * w + xx
  const long hw = (long)h * w;
  const int b = (int)(pix / hw);
  const int yy = (int)((pix % hw) / w), xx = (int)(pix % w);
  const float* xb = x + (long)b * hw * C;
  for (int c = threadIdx.x; c < C; c += 256) q[c] = xb[((long)yy * w + xx) * C + c];
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, pad = k / 2, k2 = k * k;
  for (int o = wv; o < k2; o += 4) {
    const int ny = yy + o / k - pad, nx = xx + o % k - pad;
    float s = 0.f;
    if ((unsigned)ny < (unsigned)h && (unsigned)nx < (unsigned)w) {
      const float* xn = xb + ((long)ny * w + nx) * C;
      for (int c = lane; c < C; c += 64) s = fmaf(q[c], xn[c], s);
      s = wave_sum_dpp(s);
    }
    if (lane == 0) win[o] = s;
  }
  __syncthreads();
  float ss = 0.f;
  for (int o = threadIdx.x; o < k2; o += 256) ss = fmaf(win[o], win[o], ss);
  ss = wave_sum_dpp(ss);
  __shared__ float red[4];
  if (lane == 0) red[wv] = ss;
  __syncthreads();
  const float inv = 1.f / sqrtf(((red[0] + red[1]) + (red[2] + red[3])) + 1e-6f);
  float* gp = g + pix * ldg;
  for (int o = threadIdx.x; o < ldg; o += 256) gp[o] = o < k2 ? win[o] * inv : 0.f;
}

// ---- MMN agg 'sum' (mmn.py:62-63): y[b][p] = sum over l of x[b][l][p], l in order ----
__global__ void channel_sum_kernel(const float* __restrict__ x, int B, int L, long P, float* __restrict__ y) {
  const long total = (long)B * P;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int b = (int)(e / P);
    const long p = e - (long)b * P;
    const float* xb = x + (long)b * L * P + p;
    float s = xb[0];
    for (int l = 1; l < L; ++l) s += xb[(long)l * P];
    y[e] = s;
  }
}

// ---- MatchNet's support masks (match.py:117-126, run_cyc match.py:165-182) ----
// ig_mask [B][NB] (uint8, nullable): corr2d[b][a][j] = 1e-4 where ig_mask[b][j] (every query a).
// The cycle mask: k2q[j] = argmax over a of corr2d[a][j], q2k[a] = argmax over j of corr2d[a][j]
// (after the ig mask; first index on ties, as torch's max on the CPU), inconsistent[j] =
// s_mask[j] != s_mask[q2k[k2q[j]]], and corr2d += inconsistent[j] * -1000 (Dropout(0.1) of the
// mask is the identity in eval mode).
__device__ __forceinline__ float masked_corr(const float* cr, const uint8_t* ig, int j) {
  return (ig && ig[j]) ? 1e-4f : cr[j];
}

__device__ __forceinline__ void argmax_merge(float& v, int& i, float v2, int i2) {
  if (v2 > v || (v2 == v && i2 < i)) {
    v = v2;
    i = i2;
  }
}

// q2k: one workgroup per row (b, a)
__global__ __launch_bounds__(256) void match_row_argmax_kernel(const float* __restrict__ corr, const uint8_t* ig,
                                                               int NA, int NB, int* __restrict__ q2k) {
  const long row = blockIdx.x;  // b * NA + a
  const int b = (int)(row / NA);
  const float* cr = corr + row * NB;
  const uint8_t* igb = ig ? ig + (long)b * NB : nullptr;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  float v = -INFINITY;
  int idx = 0x7fffffff;
  for (int j = t; j < NB; j += 256) argmax_merge(v, idx, masked_corr(cr, igb, j), j);
  for (int o = 32; o > 0; o >>= 1) argmax_merge(v, idx, __shfl_xor(v, o, 64), __shfl_xor(idx, o, 64));
  __shared__ float rv[4];
  __shared__ int ri[4];
  if (lane == 0) {
    rv[wv] = v;
    ri[wv] = idx;
  }
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < 4; ++w) argmax_merge(v, idx, rv[w], ri[w]);
    q2k[row] = (idx >= 0 && idx < NB) ? idx : 0;  // an all-NaN row: keep the index in range
  }
}

// k2q partials: workgroup (column block of 64, row chunk, b); 4 waves stride the chunk's rows,
// lanes own columns; partial (value, index) per (b, chunk, column)
constexpr int MATCH_COL_CHUNKS = 16;
__global__ __launch_bounds__(256) void match_col_argmax_kernel(const float* __restrict__ corr, const uint8_t* ig,
                                                               int NA, int NB, float* __restrict__ pv,
                                                               int* __restrict__ pi) {
  const int b = blockIdx.z, chunk = blockIdx.y;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + lane;
  const int per = (NA + MATCH_COL_CHUNKS - 1) / MATCH_COL_CHUNKS;
  const int a0 = chunk * per, a1 = min(NA, a0 + per);
  float v = -INFINITY;
  int idx = 0x7fffffff;
  const bool masked = ig && j < NB && ig[(long)b * NB + j];
  if (j < NB)
    for (int a = a0 + wv; a < a1; a += 4) argmax_merge(v, idx, masked ? 1e-4f : corr[((long)b * NA + a) * NB + j], a);
  __shared__ float rv[4][64];
  __shared__ int ri[4][64];
  rv[wv][lane] = v;
  ri[wv][lane] = idx;
  __syncthreads();
  if (wv == 0 && j < NB) {
    for (int w = 1; w < 4; ++w) argmax_merge(v, idx, rv[w][lane], ri[w][lane]);
    const long o = ((long)b * MATCH_COL_CHUNKS + chunk) * NB + j;
    pv[o] = v;
    pi[o] = idx;
  }
}

// inconsistent[b][j] from the chunk partials, q2k and s_mask
__global__ void match_cyc_kernel(const float* __restrict__ pv, const int* __restrict__ pi, const int* __restrict__ q2k,
                                 const int64_t* __restrict__ s_mask, int B, int NA, int NB, float* __restrict__ incons) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)B * NB) return;
  const int b = (int)(e / NB), j = (int)(e - (long)b * NB);
  float v = -INFINITY;
  int k2q = 0x7fffffff;
  for (int c = 0; c < MATCH_COL_CHUNKS; ++c) {
    const long o = ((long)b * MATCH_COL_CHUNKS + c) * NB + j;
    argmax_merge(v, k2q, pv[o], pi[o]);
  }
  if (k2q < 0 || k2q >= NA) k2q = 0;  // an all-NaN column: torch would return some index; keep it in range
  const int r = q2k[(long)b * NA + k2q];
  incons[e] = s_mask[(long)b * NB + j] != s_mask[(long)b * NB + r] ? 1.f : 0.f;
}

__global__ void match_mask_apply_kernel(float* __restrict__ corr, const uint8_t* ig, const float* incons, int B, int NA,
                                        int NB) {
  const long total = (long)B * NA * NB;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int j = (int)(e % NB);
    const int b = (int)(e / ((long)NA * NB));
    float v = corr[e];
    if (ig && ig[(long)b * NB + j]) v = 1e-4f;
    if (incons) v = v + incons[(long)b * NB + j] * -1000.f;
    corr[e] = v;
  }
}

// Train-mode Dropout(0.1) of the cycle mask (match.py:97 ass_drop, applied in run_cyc
// match.py:181): inconsistent[b][j] *= dropout_scale(p, seed, stream 5, b NB + j) -- kept entries
// become 1 / (1 - p), as nn.Dropout scales them; the mask is constant under autograd (argmax
// indices), so no gradient passes through it.
__global__ void match_cyc_dropout_kernel(float* __restrict__ incons, long n, float p, unsigned long long seed) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) incons[i] *= dropout_scale(p, seed, 5u, (unsigned long long)i);
}

// d corr2d[b][i][j] = 0 where ig_mask[b][j]: the masked entries were overwritten with the constant
// 1e-4 (match.py:117-119), so nothing flows back through them
__global__ void match_zero_ig_cols_kernel(float* __restrict__ g, const uint8_t* __restrict__ ig, int B, int NA, int NB) {
  const long total = (long)B * NA * NB;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int j = (int)(e % NB);
    const int b = (int)(e / ((long)NA * NB));
    if (ig[(long)b * NB + j]) g[e] = 0.f;
  }
}

int launch_match_zero_ig_cols(float* g, const uint8_t* ig, int B, int NA, int NB, hipStream_t st) {
  const long total = (long)B * NA * NB;
  hipLaunchKernelGGL(match_zero_ig_cols_kernel, dim3((unsigned)std::min<long>(65536, cdiv(total, 256))), dim3(256), 0, st,
                     g, ig, B, NA, NB);
  CWT_LAUNCH_CHECK();
  return 0;
}

// ---- WeightAverage (src/model/msm/msm_func.py:50-104), R = 3 ----
// tpg [N][P][3co]: theta | phi | g of every pixel (1x1 convs as one GEMM, biases not yet
// added); per pixel: cos_r = CosineSimilarity(phi(x_r), theta(x)) over its 3x3 replicate-padded
// neighbourhood r (torch: dot / (max(|phi|, 1e-8) max(|theta|, 1e-8))), softmax over the 9,
// wavg = sum_r softmax_r g(x_r).  One workgroup per pixel, co / 256 channels per thread (PART:
// co < 256, the threads past co idle).  Training mode (msm_func.py:63,90): att_drop scales the
// nine softmax weights by dropout_scale(p_att, seed, 6, pix 9 + r) before the average.
#define WA_ON(k) (!PART || t + 256 * (k) < co)
template <int CPT, bool PART = false>
__global__ __launch_bounds__(256) void wa_attn_kernel(const float* __restrict__ tpg, int h, int w, int co,
                                                      const float* __restrict__ bt, const float* __restrict__ bp,
                                                      const float* __restrict__ bg, float* __restrict__ wavg,
                                                      float p_att, unsigned long long seed) {
  const long P = (long)h * w;
  const long pix = blockIdx.x;  // n * P + p
  const long n = pix / P;
  const int p = (int)(pix - n * P), y = p / w, x = p - y * w;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const long ld = 3L * co;
  __shared__ float red[4][19];
  __shared__ float sm[9];
  float th[CPT];
  const float* tp = tpg + pix * ld;
#pragma unroll
  for (int k = 0; k < CPT; ++k) th[k] = WA_ON(k) ? tp[t + 256 * k] + bt[t + 256 * k] : 0.f;
  float part[19];
  part[18] = 0.f;
#pragma unroll
  for (int k = 0; k < CPT; ++k) part[18] = fmaf(th[k], th[k], part[18]);
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    const int yy = min(max(y + r / 3 - 1, 0), h - 1), xx = min(max(x + r % 3 - 1, 0), w - 1);
    const float* q = tpg + (n * P + (long)yy * w + xx) * ld + co;
    float d = 0.f, nn = 0.f;
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
      const float ph = WA_ON(k) ? q[t + 256 * k] + bp[t + 256 * k] : 0.f;
      d = fmaf(ph, th[k], d);
      nn = fmaf(ph, ph, nn);
    }
    part[r] = d;
    part[9 + r] = nn;
  }
#pragma unroll
  for (int i = 0; i < 19; ++i) {
    const float v = wave_sum_dpp(part[i]);
    if (lane == 0) red[wv][i] = v;
  }
  __syncthreads();
  if (t == 0) {
    float tot[19];
#pragma unroll
    for (int i = 0; i < 19; ++i) tot[i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
    const float tn = fmaxf(sqrtf(tot[18]), 1e-8f);
    float cs[9], m = -INFINITY;
#pragma unroll
    for (int r = 0; r < 9; ++r) {
      cs[r] = tot[r] / (fmaxf(sqrtf(tot[9 + r]), 1e-8f) * tn);
      m = fmaxf(m, cs[r]);
    }
    float se = 0.f;
#pragma unroll
    for (int r = 0; r < 9; ++r) {
      cs[r] = expf(cs[r] - m);
      se += cs[r];
    }
#pragma unroll
    for (int r = 0; r < 9; ++r) sm[r] = cs[r] / se;
    if (p_att > 0.f) {
#pragma unroll
      for (int r = 0; r < 9; ++r) sm[r] *= dropout_scale(p_att, seed, 6u, (unsigned long long)pix * 9 + r);
    }
  }
  __syncthreads();
  float acc[CPT];
#pragma unroll
  for (int k = 0; k < CPT; ++k) acc[k] = 0.f;
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    const int yy = min(max(y + r / 3 - 1, 0), h - 1), xx = min(max(x + r % 3 - 1, 0), w - 1);
    const float* q = tpg + (n * P + (long)yy * w + xx) * ld + 2 * co;
    const float a = sm[r];
#pragma unroll
    for (int k = 0; k < CPT; ++k)
      if (WA_ON(k)) acc[k] = fmaf(a, q[t + 256 * k] + bg[t + 256 * k], acc[k]);
  }
#pragma unroll
  for (int k = 0; k < CPT; ++k)
    if (WA_ON(k)) wavg[pix * co + t + 256 * k] = acc[k];
}
#undef WA_ON

// out = x + (back + b): conv_back's bias and WeightAverage's residual (msm_func.py:99-104)
__global__ void wa_residual_kernel(const float* __restrict__ x, const float* __restrict__ back,
                                   const float* __restrict__ b, long n, int C, float* __restrict__ out) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
    out[i] = x[i] + (back[i] + b[i % C]);
}

// training mode (msm_func.py:64,100): proj_drop on conv_back's output (bias included) before the
// residual add, element i of the NHWC map drawn as dropout_scale(p, seed, 7, i)
__global__ void wa_residual_drop_kernel(const float* __restrict__ x, const float* __restrict__ back,
                                        const float* __restrict__ b, long n, int C, float* __restrict__ out, float p,
                                        unsigned long long seed) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
    out[i] = x[i] + (back[i] + b[i % C]) * dropout_scale(p, seed, 7u, (unsigned long long)i);
}

// the backward's gradient at conv_back's output: out = d_out * the proj_drop mask
__global__ void wa_proj_mask_kernel(const float* __restrict__ d_out, long n, float p, unsigned long long seed,
                                    float* __restrict__ out) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
    out[i] = d_out[i] * dropout_scale(p, seed, 7u, (unsigned long long)i);
}

// MMN.forward's tail (mmn.py:65-67): att_mean = mean over the B support rows of att_fq;
// fq = f_q * (1 - att_wt) + att_mean * att_wt.  Tokens [B][P][C] / [P][C].
__global__ void mmn_blend_kernel(const float* __restrict__ fq_in, const float* __restrict__ att, int B, long n,
                                 float att_wt, float* __restrict__ att_mean, float* __restrict__ fq_out) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += att[(long)b * n + i];
    const float m = s / (float)B;
    att_mean[i] = m;
    fq_out[i] = fq_in[i] * (1.f - att_wt) + m * att_wt;
  }
}

int launch_wa_attn(const float* tpg, int N, int h, int w, int co, const float* bt, const float* bp, const float* bg,
                   float* wavg, hipStream_t st, float p_att, unsigned long long seed) {
  const dim3 grid((unsigned)((long)N * h * w));
#define CWT_WA(...) \
  hipLaunchKernelGGL((wa_attn_kernel<__VA_ARGS__>), grid, dim3(256), 0, st, tpg, h, w, co, bt, bp, bg, wavg, p_att, seed)
  if (co == 256) CWT_WA(1);
  else if (co == 512) CWT_WA(2);
  else if (co == 1024) CWT_WA(4);
  else if (co >= 32 && co < 256 && co % 32 == 0) CWT_WA(1, true);
  else return fail(CWT_EARG, "WeightAverage: c_in / 2 must be a multiple of 32 up to 256, or 512 or 1024");
#undef CWT_WA
  CWT_LAUNCH_CHECK();
  return 0;
}

int launch_wa_residual(const float* x, const float* back, const float* b, long n, int C, float* out, hipStream_t st,
                       float p_proj, unsigned long long seed) {
  const dim3 grid((unsigned)std::min<long>(65536, cdiv(n, 256)));
  if (p_proj > 0.f)
    hipLaunchKernelGGL(wa_residual_drop_kernel, grid, dim3(256), 0, st, x, back, b, n, C, out, p_proj, seed);
  else
    hipLaunchKernelGGL(wa_residual_kernel, grid, dim3(256), 0, st, x, back, b, n, C, out);
  CWT_LAUNCH_CHECK();
  return 0;
}

int launch_wa_proj_mask(const float* d_out, long n, float p_proj, unsigned long long seed, float* out, hipStream_t st) {
  hipLaunchKernelGGL(wa_proj_mask_kernel, dim3((unsigned)std::min<long>(65536, cdiv(n, 256))), dim3(256), 0, st, d_out,
                     n, p_proj, seed, out);
  CWT_LAUNCH_CHECK();
  return 0;
}

int launch_mmn_blend(const float* fq_in, const float* att, int B, long n, float att_wt, float* att_mean, float* fq_out,
                     hipStream_t st) {
  hipLaunchKernelGGL(mmn_blend_kernel, dim3((unsigned)std::min<long>(65536, cdiv(n, 256))), dim3(256), 0, st, fq_in,
                     att, B, n, att_wt, att_mean, fq_out);
  CWT_LAUNCH_CHECK();
  return 0;
}

// the same on the torch layout x [B][2][NA][NB] (channel planes), y channels-last [B][NA][NB][2]: the
// transposition folded into the two passes over x (MatchNet's in_channel 2 correlation)
int launch_mutual_matching_planar2(const float* x, int B, int NA, int NB, float* y, float* rowmax, float* colpart,
                                   float* colmax, hipStream_t st) {
  const int nrbv = cdiv(NA, MM_RBV);
  hipLaunchKernelGGL((mm_rowcol_kernel<2, MM_RBV, true>), dim3(nrbv, B), dim3(256), 0, st, x, NA, NB, rowmax, colpart);
  CWT_LAUNCH_CHECK();
  hipLaunchKernelGGL(mm_colmax_kernel, dim3(cdiv(NB, 64), B * 2), dim3(256), 0, st, (const float*)colpart, nrbv, NB,
                     colmax);
  CWT_LAUNCH_CHECK();
  hipLaunchKernelGGL((mm_apply_kernel<2, true>), dim3(NA, B), dim3(256), 0, st, x, NA, NB, (const float*)rowmax,
                     (const float*)colmax, y);
  CWT_LAUNCH_CHECK();
  return 0;
}

// one channel, on the sum x + x2 of two [B][NA][NB] tensors (NeighConsensus' symmetric branches;
// the add the separate pass did, in the same order)
int launch_mutual_matching_sum(const float* x, const float* x2, int B, int NA, int NB, float* y, float* rowmax,
                               float* colpart, float* colmax, hipStream_t st) {
  const int nrbv = cdiv(NA, MM_RBV);
  hipLaunchKernelGGL((mm_rowcol_kernel<1>), dim3(nrbv, B), dim3(256), 0, st, x, NA, NB, rowmax, colpart, x2);
  CWT_LAUNCH_CHECK();
  hipLaunchKernelGGL(mm_colmax_kernel, dim3(cdiv(NB, 64), B), dim3(256), 0, st, (const float*)colpart, nrbv, NB,
                     colmax);
  CWT_LAUNCH_CHECK();
  hipLaunchKernelGGL((mm_apply_kernel<1>), dim3(NA, B), dim3(256), 0, st, x, NA, NB, (const float*)rowmax,
                     (const float*)colmax, y, x2);
  CWT_LAUNCH_CHECK();
  return 0;
}

int launch_mutual_matching(const float* x, int B, int NA, int NB, int C, float* y, float* rowmax, float* colpart,
                           float* colmax, hipStream_t st) {
  const int nrb = cdiv(NA, MM_RB);
  if (C != 1 && C != 2) {  // the scalar forms
    hipLaunchKernelGGL(mm_rowcol_any_kernel, dim3(nrb, B * C), dim3(256), 0, st, x, NA, NB, C, rowmax, colpart);
    CWT_LAUNCH_CHECK();
    hipLaunchKernelGGL(mm_colmax_kernel, dim3(cdiv(NB, 64), B * C), dim3(256), 0, st, (const float*)colpart, nrb,
                       NB, colmax);
    CWT_LAUNCH_CHECK();
    const long total = (long)B * NA * NB * C;
    hipLaunchKernelGGL(mm_apply_any_kernel, dim3((unsigned)std::min<long>(65536, cdiv(total, 256))), dim3(256), 0, st,
                       x, total, NA, NB, C, (const float*)rowmax, (const float*)colmax, y);
    CWT_LAUNCH_CHECK();
    return 0;
  }
  const int nrbv = cdiv(NA, MM_RBV);
  if (C == 1)
    hipLaunchKernelGGL((mm_rowcol_kernel<1>), dim3(nrbv, B), dim3(256), 0, st, x, NA, NB, rowmax, colpart);
  else
    hipLaunchKernelGGL((mm_rowcol_kernel<2>), dim3(nrbv, B), dim3(256), 0, st, x, NA, NB, rowmax, colpart);
  CWT_LAUNCH_CHECK();
  hipLaunchKernelGGL(mm_colmax_kernel, dim3(cdiv(NB, 64), B * C), dim3(256), 0, st, (const float*)colpart, nrbv, NB,
                     colmax);
  CWT_LAUNCH_CHECK();
  if (C == 1)
    hipLaunchKernelGGL(mm_apply_kernel<1>, dim3(NA, B), dim3(256), 0, st, x, NA, NB, (const float*)rowmax,
                       (const float*)colmax, y);
  else
    hipLaunchKernelGGL(mm_apply_kernel<2>, dim3(NA, B), dim3(256), 0, st, x, NA, NB, (const float*)rowmax,
                       (const float*)colmax, y);
  CWT_LAUNCH_CHECK();
  return 0;
}

int launch_to_channels_last(const float* x, int B, int C, long P, float* y, hipStream_t st) {
  const long n = (long)B * C * P;
  hipLaunchKernelGGL(to_channels_last_kernel, dim3((unsigned)std::min<long>(65536, cdiv(n, 256))), dim3(256), 0, st, x,
                     B, C, P, y);
  CWT_LAUNCH_CHECK();
  return 0;
}

int launch_add_inplace(float* y, const float* x, long n, hipStream_t st) {
  hipLaunchKernelGGL(add_inplace_kernel, dim3((unsigned)std::min<long>(65536, cdiv(n, 256))), dim3(256), 0, st, y, x, n);
  CWT_LAUNCH_CHECK();
  return 0;
}

int launch_match_softmax(const float* corr, int B, int NA, int NB, float temp, int ldp, float* P, hipStream_t st) {
  hipLaunchKernelGGL(match_softmax_kernel, dim3(B * NA), dim3(256), 0, st, corr, NA, NB, temp, ldp, P);
  CWT_LAUNCH_CHECK();
  return 0;
}

int launch_match_vt(const float* v, int B, int NB, int C, int ldp, float* vt, hipStream_t st) {
  hipLaunchKernelGGL(match_vt_kernel, dim3(cdiv(ldp, 32), cdiv(C, 32), B), dim3(256), 0, st, v, NB, C, ldp, vt);
  CWT_LAUNCH_CHECK();
  return 0;
}

int launch_match_masks(float* corr, int B, int NA, int NB, const uint8_t* ig, const int64_t* s_mask, float* incons,
                       int* q2k, float* pv, int* pi, hipStream_t st, float drop_p, unsigned long long seed) {
  if (s_mask) {
    hipLaunchKernelGGL(match_row_argmax_kernel, dim3(B * NA), dim3(256), 0, st, (const float*)corr, ig, NA, NB, q2k);
    CWT_LAUNCH_CHECK();
    hipLaunchKernelGGL(match_col_argmax_kernel, dim3(cdiv(NB, 64), MATCH_COL_CHUNKS, B), dim3(256), 0, st,
                       (const float*)corr, ig, NA, NB, pv, pi);
    CWT_LAUNCH_CHECK();
    hipLaunchKernelGGL(match_cyc_kernel, dim3(cdiv((long)B * NB, 256)), dim3(256), 0, st, (const float*)pv,
                       (const int*)pi, (const int*)q2k, s_mask, B, NA, NB, incons);
    CWT_LAUNCH_CHECK();
    if (drop_p > 0.f) {
      hipLaunchKernelGGL(match_cyc_dropout_kernel, dim3(cdiv((long)B * NB, 256)), dim3(256), 0, st, incons, (long)B * NB,
                         drop_p, seed);
      CWT_LAUNCH_CHECK();
    }
  }
  if (ig || s_mask) {
    const long total = (long)B * NA * NB;
    hipLaunchKernelGGL(match_mask_apply_kernel, dim3((unsigned)std::min<long>(65536, cdiv(total, 256))), dim3(256), 0,
                       st, corr, ig, s_mask ? (const float*)incons : (const float*)nullptr, B, NA, NB);
    CWT_LAUNCH_CHECK();
  }
  return 0;
}

int launch_cv4d_layer(const float* x, int B, int hA, int wA, int hB, int wB, int cin, int cout, const float* W,
                      const float* bias, int swap, float* y, hipStream_t st) {
  const long total = (long)B * hA * wA * hB * wB;
  const dim3 grid((unsigned)std::min<long>(65536, cdiv(total, 256)));
#define CWT_CV4D(CI, CO)                                                                                      \
  if (cin == CI && cout == CO) {                                                                              \
    hipLaunchKernelGGL((cv4d_layer_kernel<CI, CO>), grid, dim3(256), 0, st, x, B, hA, wA, hB, wB, W, bias, swap, y); \
    CWT_LAUNCH_CHECK();                                                                                       \
    return 0;                                                                                                 \
  }
  CWT_CV4D(1, 10)
  CWT_CV4D(2, 10)
  CWT_CV4D(10, 10)
  CWT_CV4D(10, 1)
#undef CWT_CV4D
  return fail(CWT_EARG, "cv4d layer: channels (1|2 -> 10, 10 -> 10, 10 -> 1) only");
}

int launch_sce_descriptor(const float* x, int B, int h, int w, int C, int k, int ldg, float* g, hipStream_t st) {
  if (k < 1 || k % 2 == 0 || k * k > SCE_MAXK2 || ldg < k * k) return fail(CWT_EARG, "sce: odd kernel size, k*k <= 1024");
  const size_t lds = (size_t)(C + k * k) * 4;
  if (lds > 64 * 1024) return fail(CWT_EARG, "sce: C + k*k floats must fit 64 KB of LDS");
  hipLaunchKernelGGL(sce_descriptor_kernel, dim3((unsigned)((long)B * h * w)), dim3(256), lds, st, x, h, w, C, k, ldg, g);
  CWT_LAUNCH_CHECK();
  return 0;
}

int launch_channel_sum(const float* x, int B, int L, long P, float* y, hipStream_t st) {
  const long total = (long)B * P;
  hipLaunchKernelGGL(channel_sum_kernel, dim3((unsigned)std::min<long>(65536, cdiv(total, 256))), dim3(256), 0, st, x, B,
                     L, P, y);
  CWT_LAUNCH_CHECK();
  return 0;
}

}  // namespace cwt
