// Backward of MatchNet's corr_forward chain and of the MMN head's WeightAverage / get_corr
// (VERDICT r3 item 6): reference src/model/match.py:21-163 (MutualMatching,
// NeighConsensus, corr_forward), src/model/conv4d.py:40-62 (CenterPivotConv4d),
// src/model/msm/msm_func.py:66-104 (WeightAverage), src/model/model_util.py:101-109 (get_corr),
// src/model/mmn.py:65-67 (the blend) -- the modules MMN (train_cca.py:101, train_aug.py:102) and
// DeTr's cross attention (train_trans.py:100) train through.
//
// Exact fp32; every reduction runs in a fixed order (no atomics), so a backward is deterministic.
// Layouts are the forward's (match.hip): 4-D tensors channels-last [B][a][b][C], a = (ha, wa),
// b = (hb, wb); WeightAverage's tpg [N·P][3co] = theta | phi | g before their biases.
#include <cstdlib>

#include "../../include/cwt.h"
#include "common.h"
#include "kernels.h"

namespace cwt {

// ---- MutualMatching (match.py:34-53) backward, per channel of x[B][NA][NB][C] ----
// forward: u[a] = max_b x[a][b] + eps, v[b] = max_a x[a][b] + eps, y = x * ((x / u) * (x / v)).
// torch.max sends a maximum's gradient to ONE index (here the first maximal position), so
//   dx = dy * (x/u * x/v + x * (x/v / u + x/u / v))
//        - [b == argmax over b of row a] * sum_b' dy y / u[a]
//        - [a == argmax over a of column b] * sum_a' dy y / v[b].
constexpr int MB_RB = 16;  // rows of a per workgroup

__device__ __forceinline__ void argmax_merge(float& v, int& i, float v2, int i2) {
  if (v2 > v || (v2 == v && i2 < i)) {
    v = v2;
    i = i2;
  }
}

// row (max, first argmax) and per-row-block column partial (max, first argmax)
__global__ __launch_bounds__(256) void mmb_rowcol_kernel(const float* __restrict__ x, int NA, int NB, int C,
                                                         float* __restrict__ rowmax, int* __restrict__ rowarg,
                                                         float* __restrict__ colpv, int* __restrict__ colpi) {
  const int bc = blockIdx.y, b = bc / C, c = bc - b * C;
  const int a0 = blockIdx.x * MB_RB;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const float* xb = x + (long)b * NA * NB * C + c;
  __shared__ float sv[4][MB_RB];
  __shared__ int si[4][MB_RB];
  float rv[MB_RB];
  int ri[MB_RB];
#pragma unroll
  for (int r = 0; r < MB_RB; ++r) {
    rv[r] = -INFINITY;
    ri[r] = NB;
  }
  for (int j = t; j < NB; j += 256) {
    float cv = -INFINITY;
    int ci = NA;
#pragma unroll
    for (int r = 0; r < MB_RB; ++r) {
      const int a = a0 + r;
      if (a < NA) {
        const float v = xb[((long)a * NB + j) * C];
        if (v > cv) {
          cv = v;
          ci = a;
        }
        if (v > rv[r]) {
          rv[r] = v;
          ri[r] = j;
        }
      }
    }
    colpv[((long)bc * gridDim.x + blockIdx.x) * NB + j] = cv;
    colpi[((long)bc * gridDim.x + blockIdx.x) * NB + j] = ci;
  }
#pragma unroll
  for (int r = 0; r < MB_RB; ++r) {
    float v = rv[r];
    int i = ri[r];
    for (int o = 32; o > 0; o >>= 1) argmax_merge(v, i, __shfl_xor(v, o, 64), __shfl_xor(i, o, 64));
    if (lane == 0) {
      sv[wv][r] = v;
      si[wv][r] = i;
    }
  }
  __syncthreads();
  if (t < MB_RB && a0 + t < NA) {
    float v = sv[0][t];
    int i = si[0][t];
    for (int q = 1; q < 4; ++q) argmax_merge(v, i, sv[q][t], si[q][t]);
    rowmax[(long)bc * NA + a0 + t] = v;
    rowarg[(long)bc * NA + a0 + t] = i;
  }
}

__global__ __launch_bounds__(256) void mmb_colred_kernel(const float* __restrict__ colpv, const int* __restrict__ colpi,
                                                         int nrb, int NB, float* __restrict__ colmax,
                                                         int* __restrict__ colarg) {
  const int bc = blockIdx.y;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= NB) return;
  float v = -INFINITY;
  int i = 0x7fffffff;
  for (int rb = 0; rb < nrb; ++rb)
    argmax_merge(v, i, colpv[((long)bc * nrb + rb) * NB + j], colpi[((long)bc * nrb + rb) * NB + j]);
  colmax[(long)bc * NB + j] = v;
  colarg[(long)bc * NB + j] = i;
}

// srow[a] = sum_b dy y over the row; scolp[row block][b] = the block's partial column sums
__global__ __launch_bounds__(256) void mmb_sums_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                       int NA, int NB, int C, const float* __restrict__ rowmax,
                                                       const float* __restrict__ colmax, float* __restrict__ srow,
                                                       float* __restrict__ scolp) {
  const float eps = 1e-5f;
  const int bc = blockIdx.y, b = bc / C, c = bc - b * C;
  const int a0 = blockIdx.x * MB_RB;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const long base = (long)b * NA * NB * C + c;
  __shared__ float red[4][MB_RB];
  float rs[MB_RB];
#pragma unroll
  for (int r = 0; r < MB_RB; ++r) rs[r] = 0.f;
  float u[MB_RB];
#pragma unroll
  for (int r = 0; r < MB_RB; ++r) u[r] = a0 + r < NA ? rowmax[(long)bc * NA + a0 + r] + eps : 1.f;
  for (int j = t; j < NB; j += 256) {
    const float vb_den = colmax[(long)bc * NB + j] + eps;
    float cs = 0.f;
#pragma unroll
    for (int r = 0; r < MB_RB; ++r) {
      const int a = a0 + r;
      if (a < NA) {
        const long i = base + ((long)a * NB + j) * C;
        const float v = x[i];
        const float y = v * ((v / u[r]) * (v / vb_den));
        const float p = dy[i] * y;
        rs[r] += p;
        cs += p;
      }
    }
    scolp[((long)bc * gridDim.x + blockIdx.x) * NB + j] = cs;
  }
#pragma unroll
  for (int r = 0; r < MB_RB; ++r) {
    const float v = wave_sum_dpp(rs[r]);
    if (lane == 0) red[wv][r] = v;
  }
  __syncthreads();
  if (t < MB_RB && a0 + t < NA) srow[(long)bc * NA + a0 + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
}

__global__ __launch_bounds__(256) void mmb_colsum_kernel(const float* __restrict__ scolp, int nrb, int NB,
                                                         float* __restrict__ scol) {
  const int bc = blockIdx.y;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= NB) return;
  float s = 0.f;
  for (int rb = 0; rb < nrb; ++rb) s += scolp[((long)bc * nrb + rb) * NB + j];
  scol[(long)bc * NB + j] = s;
}

__global__ __launch_bounds__(256) void mmb_apply_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                        long total, int NA, int NB, int C,
                                                        const float* __restrict__ rowmax, const int* __restrict__ rowarg,
                                                        const float* __restrict__ colmax, const int* __restrict__ colarg,
                                                        const float* __restrict__ srow, const float* __restrict__ scol,
                                                        float* __restrict__ dx) {
  const float eps = 1e-5f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C);
    const long p = i / C;
    const int j = (int)(p % NB);
    const long ab = p / NB;
    const int a = (int)(ab % NA), b = (int)(ab / NA);
    const int bc = b * C + c;
    const float u = rowmax[(long)bc * NA + a] + eps, w = colmax[(long)bc * NB + j] + eps;
    const float v = x[i], g = dy[i];
    const float va = v / u, vb = v / w;
    float d = g * (va * vb + v * (vb / u + va / w));
    if (j == rowarg[(long)bc * NA + a]) d -= srow[(long)bc * NA + a] / u;
    if (a == colarg[(long)bc * NB + j]) d -= scol[(long)bc * NB + j] / w;
    dx[i] = d;
  }
}

int launch_mutual_matching_bwd(const float* x, const float* dy, int B, int NA, int NB, int C, float* dx,
                               const MmBwdWs& ws, hipStream_t st) {
  const int nrb = cdiv(NA, MB_RB);
  hipLaunchKernelGGL(mmb_rowcol_kernel, dim3(nrb, B * C), dim3(256), 0, st, x, NA, NB, C, ws.rowmax, ws.rowarg, ws.colpv,
                     ws.colpi);
  CWT_LAUNCH_CHECK();
  hipLaunchKernelGGL(mmb_colred_kernel, dim3(cdiv(NB, 256), B * C), dim3(256), 0, st, (const float*)ws.colpv,
                     (const int*)ws.colpi, nrb, NB, ws.colmax, ws.colarg);
  CWT_LAUNCH_CHECK();
  hipLaunchKernelGGL(mmb_sums_kernel, dim3(nrb, B * C), dim3(256), 0, st, x, dy, NA, NB, C, (const float*)ws.rowmax,
                     (const float*)ws.colmax, ws.srow, ws.colpv);
  CWT_LAUNCH_CHECK();
  hipLaunchKernelGGL(mmb_colsum_kernel, dim3(cdiv(NB, 256), B * C), dim3(256), 0, st, (const float*)ws.colpv, nrb, NB,
                     ws.scol);
  CWT_LAUNCH_CHECK();
  const long total = (long)B * NA * NB * C;
  hipLaunchKernelGGL(mmb_apply_kernel, dim3((unsigned)std::min<long>(65536, cdiv(total, 256))), dim3(256), 0, st, x, dy,
                     total, NA, NB, C, (const float*)ws.rowmax, (const int*)ws.rowarg, (const float*)ws.colmax,
                     (const int*)ws.colarg, (const float*)ws.srow, (const float*)ws.scol, dx);
  CWT_LAUNCH_CHECK();
  return 0;
}

// ---- ReLU backward: gm = g * (out > 0) (torch's threshold_backward on the ReLU's result) ----
__global__ void relu_mask_kernel(const float* __restrict__ g, const float* __restrict__ out, long n,
                                 float* __restrict__ gm) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
    gm[i] = out[i] > 0.f ? g[i] : 0.f;
}

int launch_relu_mask(const float* g, const float* out, long n, float* gm, hipStream_t st) {
  hipLaunchKernelGGL(relu_mask_kernel, dim3((unsigned)std::min<long>(65536, cdiv(n, 256))), dim3(256), 0, st, g, out, n,
                     gm);
  CWT_LAUNCH_CHECK();
  return 0;
}

// ---- softmax(temp * corr2d) readout backward (match.py:151-153) ----
// g[a][n] (+)= temp * P[a][n] * (dA[a][n] - sum_m P[a][m] dA[a][m]); one workgroup per row
__global__ __launch_bounds__(256) void match_softmax_bwd_kernel(const float* __restrict__ P, int ldp,
                                                                const float* __restrict__ dA, int NB, float temp,
                                                                int accum, float* __restrict__ g) {
  const long row = blockIdx.x;
  const float* pr = P + row * ldp;
  const float* dr = dA + row * NB;
  float* gr = g + row * NB;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  __shared__ float red[4];
  float s = 0.f;
  for (int j = t; j < NB; j += 256) s = fmaf(pr[j], dr[j], s);
  s = wave_sum_dpp(s);
  if (lane == 0) red[wv] = s;
  __syncthreads();
  const float dot = (red[0] + red[1]) + (red[2] + red[3]);
  for (int j = t; j < NB; j += 256) {
    const float v = temp * pr[j] * (dr[j] - dot);
    gr[j] = accum ? gr[j] + v : v;
  }
}

int launch_match_softmax_bwd(const float* P, int ldp, const float* dA, int rows, int NB, float temp, int accum,
                             float* g, hipStream_t st) {
  hipLaunchKernelGGL(match_softmax_bwd_kernel, dim3(rows), dim3(256), 0, st, P, ldp, dA, NB, temp, accum, g);
  CWT_LAUNCH_CHECK();
  return 0;
}

// ---- F.normalize (model_util.py:106-107) forward with the norms kept, and its backward ----
// xn = x / max(|x|, eps); dx = (dxn - xn (xn . dxn)) / |x| where |x| > eps, dxn / eps elsewhere
__global__ __launch_bounds__(256) void token_norm_kernel(const float* __restrict__ x, long T, int C, float eps,
                                                         float* __restrict__ xn, float* __restrict__ nrm) {
  const int lane = threadIdx.x & 63;
  for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < T; r += (long)gridDim.x * 4) {
    const float* xr = x + r * C;
    float ss = 0.f;
    for (int c = lane; c < C; c += 64) ss = fmaf(xr[c], xr[c], ss);
    const float n = sqrtf(wave_sum_dpp(ss));
    const float inv = 1.f / fmaxf(n, eps);
    for (int c = lane; c < C; c += 64) xn[r * C + c] = xr[c] * inv;
    if (lane == 0) nrm[r] = n;
  }
}

__global__ __launch_bounds__(256) void token_norm_bwd_kernel(const float* __restrict__ xn, const float* __restrict__ nrm,
                                                             const float* __restrict__ dxn, long T, int C, int ld_d,
                                                             float eps, int accum, float* __restrict__ dx) {
  const int lane = threadIdx.x & 63;
  for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < T; r += (long)gridDim.x * 4) {
    const float* xr = xn + r * C;
    const float* dr = dxn + r * ld_d;
    const float n = nrm[r];
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s = fmaf(xr[c], dr[c], s);
    s = wave_sum_dpp(s);
    for (int c = lane; c < C; c += 64) {
      const float v = n > eps ? (dr[c] - xr[c] * s) / n : dr[c] / eps;
      dx[r * C + c] = accum ? dx[r * C + c] + v : v;
    }
  }
}

int launch_token_norm(const float* x, long T, int C, float eps, float* xn, float* nrm, hipStream_t st) {
  hipLaunchKernelGGL(token_norm_kernel, dim3((unsigned)std::min<long>(4096, (T + 3) / 4)), dim3(256), 0, st, x, T, C, eps,
                     xn, nrm);
  CWT_LAUNCH_CHECK();
  return 0;
}

int launch_token_norm_bwd(const float* xn, const float* nrm, const float* dxn, long T, int C, int ld_d, float eps,
                          int accum, float* dx, hipStream_t st) {
  hipLaunchKernelGGL(token_norm_bwd_kernel, dim3((unsigned)std::min<long>(4096, (T + 3) / 4)), dim3(256), 0, st, xn, nrm,
                     dxn, T, C, ld_d, eps, accum, dx);
  CWT_LAUNCH_CHECK();
  return 0;
}

// ---- WeightAverage (msm_func.py:66-104) backward, R = 3 ----
// Per pixel p with theta = tpg_t + b_t, phi_r / g_r the neighbour r's (replicate padding),
// cos_r = theta . phi_r / (n_t n_r) (n = max(|.|, 1e-8)), s = softmax(cos), wavg = sum_r s_r g_r:
//   ds_r = dwavg . g_r, dcos_r = s_r (ds_r - sum s ds),
//   dtheta = sum_r dcos_r phi_r / (n_t n_r) - theta (sum_r dcos_r cos_r) / |theta|^2,
//   dphi_r += dcos_r theta / (n_t n_r) - phi_r dcos_r cos_r / |phi_r|^2,  dg_r += s_r dwavg
// (the |.|^2 terms only where the norm exceeds the clamp).  wa_bwd_pix_kernel forms dtheta and
// the per-(p, r) coefficients; wa_bwd_nbr_kernel gathers each pixel's dphi / dg from the pixels
// whose neighbourhood holds it (at most the 3 x 3 around it), in a fixed order.
// With att_drop (wavg = sum_r m_r s_r g_r, m_r = dropout_scale(p_att, seed, 6, pix 9 + r) drawn
// again here): ds_r = m_r dwavg . g_r, dg_r += m_r s_r dwavg; the softmax backward keeps the
// pre-dropout s.  PART: co < 256, the threads past co idle.
#define WA_ON(k) (!PART || t + 256 * (k) < co)
template <int CPT, bool PART = false>
__global__ __launch_bounds__(256) void wa_bwd_pix_kernel(const float* __restrict__ tpg, int h, int w, int co,
                                                         const float* __restrict__ bt, const float* __restrict__ bp,
                                                         const float* __restrict__ bg,
                                                         const float* __restrict__ dwavg, float* __restrict__ coef,
                                                         float* __restrict__ dtpg, float p_att,
                                                         unsigned long long seed) {
  const long P = (long)h * w;
  const long pix = blockIdx.x;
  const long n = pix / P;
  const int p = (int)(pix - n * P), y = p / w, x = p - y * w;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const long ld = 3L * co;
  __shared__ float red[4][28];
  __shared__ float cf[10];  // cA[9], cTh
  float th[CPT], dw[CPT];
  const float* tp = tpg + pix * ld;
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    th[k] = WA_ON(k) ? tp[t + 256 * k] + bt[t + 256 * k] : 0.f;
    dw[k] = WA_ON(k) ? dwavg[pix * co + t + 256 * k] : 0.f;
  }
  float part[28];
  part[18] = 0.f;
#pragma unroll
  for (int k = 0; k < CPT; ++k) part[18] = fmaf(th[k], th[k], part[18]);
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    const int yy = min(max(y + r / 3 - 1, 0), h - 1), xx = min(max(x + r % 3 - 1, 0), w - 1);
    const float* q = tpg + (n * P + (long)yy * w + xx) * ld;
    float d = 0.f, nn = 0.f, dg = 0.f;
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
      const float ph = WA_ON(k) ? q[co + t + 256 * k] + bp[t + 256 * k] : 0.f;
      const float gv = WA_ON(k) ? q[2 * co + t + 256 * k] + bg[t + 256 * k] : 0.f;
      d = fmaf(ph, th[k], d);
      nn = fmaf(ph, ph, nn);
      dg = fmaf(dw[k], gv, dg);
    }
    part[r] = d;
    part[9 + r] = nn;
    part[19 + r] = dg;
  }
#pragma unroll
  for (int i = 0; i < 28; ++i) {
    const float v = wave_sum_dpp(part[i]);
    if (lane == 0) red[wv][i] = v;
  }
  __syncthreads();
  if (t == 0) {
    float tot[28];
#pragma unroll
    for (int i = 0; i < 28; ++i) tot[i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
    const float tn_raw = sqrtf(tot[18]), tn = fmaxf(tn_raw, 1e-8f);
    float cs[9], sm[9], nr[9], m = -INFINITY;
#pragma unroll
    for (int r = 0; r < 9; ++r) {
      nr[r] = fmaxf(sqrtf(tot[9 + r]), 1e-8f);
      cs[r] = tot[r] / (nr[r] * tn);
      m = fmaxf(m, cs[r]);
    }
    float se = 0.f;
#pragma unroll
    for (int r = 0; r < 9; ++r) {
      sm[r] = expf(cs[r] - m);
      se += sm[r];
    }
    float sds = 0.f, mk[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) {
      mk[r] = p_att > 0.f ? dropout_scale(p_att, seed, 6u, (unsigned long long)pix * 9 + r) : 1.f;
      if (p_att > 0.f) tot[19 + r] *= mk[r];
      sm[r] = sm[r] / se;
      sds = fmaf(sm[r], tot[19 + r], sds);
    }
    float cth = 0.f;
#pragma unroll
    for (int r = 0; r < 9; ++r) {
      const float dcos = sm[r] * (tot[19 + r] - sds);
      const float ca = dcos / (nr[r] * tn);
      const float cphi = sqrtf(tot[9 + r]) > 1e-8f ? dcos * cs[r] / tot[9 + r] : 0.f;
      cth = fmaf(dcos, cs[r], cth);
      cf[r] = ca;
      coef[pix * 27 + r] = ca;
      coef[pix * 27 + 9 + r] = cphi;
      coef[pix * 27 + 18 + r] = p_att > 0.f ? sm[r] * mk[r] : sm[r];
    }
    cf[9] = tn_raw > 1e-8f ? cth / tot[18] : 0.f;
  }
  __syncthreads();
  float dth[CPT];
#pragma unroll
  for (int k = 0; k < CPT; ++k) dth[k] = -cf[9] * th[k];
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    const int yy = min(max(y + r / 3 - 1, 0), h - 1), xx = min(max(x + r % 3 - 1, 0), w - 1);
    const float* q = tpg + (n * P + (long)yy * w + xx) * ld + co;
    const float a = cf[r];
#pragma unroll
    for (int k = 0; k < CPT; ++k)
      if (WA_ON(k)) dth[k] = fmaf(a, q[t + 256 * k] + bp[t + 256 * k], dth[k]);
  }
#pragma unroll
  for (int k = 0; k < CPT; ++k)
    if (WA_ON(k)) dtpg[pix * ld + t + 256 * k] = dth[k];
}

template <int CPT, bool PART = false>
__global__ __launch_bounds__(256) void wa_bwd_nbr_kernel(const float* __restrict__ tpg, int h, int w, int co,
                                                         const float* __restrict__ bt, const float* __restrict__ bp,
                                                         const float* __restrict__ dwavg,
                                                         const float* __restrict__ coef, float* __restrict__ dtpg) {
  const long P = (long)h * w;
  const long pix = blockIdx.x;
  const long n = pix / P;
  const int q = (int)(pix - n * P), yq = q / w, xq = q - yq * w;
  const int t = threadIdx.x;
  if (PART && t >= co) return;  // CPT = 1, no barrier below
  const long ld = 3L * co;
  float ph[CPT], dph[CPT], dg[CPT];
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    ph[k] = tpg[pix * ld + co + t + 256 * k] + bp[t + 256 * k];
    dph[k] = 0.f;
    dg[k] = 0.f;
  }
  for (int dy = -1; dy <= 1; ++dy) {
    const int yp = yq + dy;
    if (yp < 0 || yp >= h) continue;
    for (int dx = -1; dx <= 1; ++dx) {
      const int xp = xq + dx;
      if (xp < 0 || xp >= w) continue;
      const long pp = n * P + (long)yp * w + xp;
      for (int r = 0; r < 9; ++r) {
        const int yy = min(max(yp + r / 3 - 1, 0), h - 1), xx = min(max(xp + r % 3 - 1, 0), w - 1);
        if (yy != yq || xx != xq) continue;
        const float ca = coef[pp * 27 + r], cphi = coef[pp * 27 + 9 + r], s = coef[pp * 27 + 18 + r];
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
          const float thp = tpg[pp * ld + t + 256 * k] + bt[t + 256 * k];
          dph[k] = fmaf(ca, thp, fmaf(-cphi, ph[k], dph[k]));
          dg[k] = fmaf(s, dwavg[pp * co + t + 256 * k], dg[k]);
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < CPT; ++k) {
    dtpg[pix * ld + co + t + 256 * k] = dph[k];
    dtpg[pix * ld + 2 * co + t + 256 * k] = dg[k];
  }
}

int launch_wa_bwd(const float* tpg, int N, int h, int w, int co, const float* bt, const float* bp, const float* bg,
                  const float* dwavg, float* coef, float* dtpg, hipStream_t st, float p_att,
                  unsigned long long seed) {
  const dim3 grid((unsigned)((long)N * h * w));
#define CWT_WAB(...)                                                                                               \
  hipLaunchKernelGGL((wa_bwd_pix_kernel<__VA_ARGS__>), grid, dim3(256), 0, st, tpg, h, w, co, bt, bp, bg, dwavg, coef, \
                     dtpg, p_att, seed);                                                                           \
  CWT_LAUNCH_CHECK();                                                                                              \
  hipLaunchKernelGGL((wa_bwd_nbr_kernel<__VA_ARGS__>), grid, dim3(256), 0, st, tpg, h, w, co, bt, bp, dwavg,         \
                     (const float*)coef, dtpg);                                                                    \
  CWT_LAUNCH_CHECK();
  if (co == 256) {
    CWT_WAB(1)
  } else if (co == 512) {
    CWT_WAB(2)
  } else if (co == 1024) {
    CWT_WAB(4)
  } else if (co >= 32 && co < 256 && co % 32 == 0) {
    CWT_WAB(1, true)
  } else {
    return fail(CWT_EARG, "WeightAverage backward: c_in / 2 must be a multiple of 32 up to 256, or 512 or 1024");
  }
#undef CWT_WAB
#undef WA_ON
  return 0;
}

// ---- small helpers ----
// out[c] (+)= sum_r X[r][c] (row stride ld): the bias gradients.  Two fixed-order stages: chunks
// of CS_ROWS rows summed per (64-column block, chunk) workgroup, 4 row lanes of 64 columns each
// combined in lane order; then the chunk partials summed in chunk order.
constexpr int CS_ROWS = 64;
__global__ __launch_bounds__(256) void colsum_part_kernel(const float* __restrict__ X, long R, int Cc, long ld,
                                                          float* __restrict__ part) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
  const long r0 = (long)blockIdx.y * CS_ROWS;
  __shared__ float red[4][64];
  float s = 0.f;
  if (c < Cc)
    for (int i = rl; i < CS_ROWS && r0 + i < R; i += 4) s += X[(r0 + i) * ld + c];
  red[rl][threadIdx.x & 63] = s;
  __syncthreads();
  if (rl == 0 && c < Cc) {
    const int l = threadIdx.x & 63;
    part[(long)blockIdx.y * Cc + c] = (red[0][l] + red[1][l]) + (red[2][l] + red[3][l]);
  }
}

__global__ void colsum_final_kernel(const float* __restrict__ part, int nch, int Cc, int accum, float* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= Cc) return;
  float s = 0.f;
  for (int k = 0; k < nch; ++k) s += part[(long)k * Cc + c];
  out[c] = accum ? out[c] + s : s;
}

size_t colsum_ws_floats(long R, int Cc) { return (size_t)cdiv(R, CS_ROWS) * Cc; }

int launch_colsum(const float* X, long R, int Cc, long ld, int accum, float* out, float* ws, size_t ws_floats,
                  hipStream_t st) {
  const int nch = cdiv(R, CS_ROWS);
  if (!ws || ws_floats < colsum_ws_floats(R, Cc)) return fail(CWT_ESTATE, "colsum: workspace too small");
  hipLaunchKernelGGL(colsum_part_kernel, dim3(cdiv(Cc, 64), nch), dim3(256), 0, st, X, R, Cc, ld, ws);
  CWT_LAUNCH_CHECK();
  hipLaunchKernelGGL(colsum_final_kernel, dim3(cdiv(Cc, 256)), dim3(256), 0, st, (const float*)ws, nch, Cc, accum, out);
  CWT_LAUNCH_CHECK();
  return 0;
}

// y[b][c][p] = x[b][p][c] (channels-last -> channel-first)
__global__ void to_channels_first_kernel(const float* __restrict__ x, int B, int C, long P, float* __restrict__ y) {
  const long total = (long)B * C * P;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long p = i % P;
    const int c = (int)((i / P) % C);
    const long b = i / ((long)C * P);
    y[i] = x[(b * P + p) * C + c];
  }
}

int launch_to_channels_first(const float* x, int B, int C, long P, float* y, hipStream_t st) {
  const long n = (long)B * C * P;
  hipLaunchKernelGGL(to_channels_first_kernel, dim3((unsigned)std::min<long>(65536, cdiv(n, 256))), dim3(256), 0, st, x,
                     B, C, P, y);
  CWT_LAUNCH_CHECK();
  return 0;
}

// out [R][ld] = X [R][Cc] with the pad columns zero
__global__ void copy_pad_kernel(const float* __restrict__ X, long R, int Cc, int ld, float* __restrict__ out) {
  const long total = R * ld;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / ld;
    const int c = (int)(i - r * ld);
    out[i] = c < Cc ? X[r * Cc + c] : 0.f;
  }
}

int launch_copy_pad(const float* X, long R, int Cc, int ld, float* out, hipStream_t st) {
  const long n = R * ld;
  hipLaunchKernelGGL(copy_pad_kernel, dim3((unsigned)std::min<long>(65536, cdiv(n, 256))), dim3(256), 0, st, X, R, Cc,
                     ld, out);
  CWT_LAUNCH_CHECK();
  return 0;
}

// MMN blend (mmn.py:65-67) backward: d_att[b][i] = (d_mean[i] + att_wt d_fq[i]) / B,
// d_fq_in[i] = (1 - att_wt) d_fq[i]
__global__ void mmn_blend_bwd_kernel(const float* __restrict__ d_fq, const float* __restrict__ d_mean, int B, long n,
                                     float att_wt, float* __restrict__ d_att, float* __restrict__ d_fq_in) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float g = d_fq ? d_fq[i] : 0.f;
    const float dm = ((d_mean ? d_mean[i] : 0.f) + att_wt * g) / (float)B;
    for (int b = 0; b < B; ++b) d_att[(long)b * n + i] = dm;
    if (d_fq_in) d_fq_in[i] = (1.f - att_wt) * g;
  }
}

int launch_mmn_blend_bwd(const float* d_fq, const float* d_mean, int B, long n, float att_wt, float* d_att,
                         float* d_fq_in, hipStream_t st) {
  hipLaunchKernelGGL(mmn_blend_bwd_kernel, dim3((unsigned)std::min<long>(65536, cdiv(n, 256))), dim3(256), 0, st, d_fq,
                     d_mean, B, n, att_wt, d_att, d_fq_in);
  CWT_LAUNCH_CHECK();
  return 0;
}

}  // namespace cwt
