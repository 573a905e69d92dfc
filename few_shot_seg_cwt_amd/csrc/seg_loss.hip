// The MMN / DeTr trainers' loss head (reference src/train_kshot.py:168-183): on the low-resolution
// classifier logits [B][2][h][w] (src/model/pspnet.py:183-187), the bilinear align_corners=True
// upsample to the S x S label, SegLoss (src/model/model_util.py:9-73: weighted_dice_loss,
// weighted_ce_loss, CrossEntropyLoss(ignore_index=255)) and the gradient carried back through the
// upsample and the classifier to the feature map f.
//
// Three launches, every sum in a fixed order (no float atomics), the S x S logits never stored:
//  1. shl_reduce_kernel: per-block double partials of the six sums the loss needs
//       wt_dc: {I_0, I_1, sum p_0^2, sum p_1^2, sum t_0, sum t_1} per image
//       ce:    {n_0, n_1, sum nll | y = 0, sum nll | y = 1, -, -} per image
//  2. shl_final_kernel: the partials summed by a fixed LDS tree, the loss, and the per-(b, k)
//     coefficients of the gradient
//       wt_dc: dz_k = p_k (1 - p_k) (a_k t_k + c_k p_k),  a_k = -2 / (max(D_k, 1e-8) B),
//              c_k = 4 I_k / (D_k^2 B) where D_k >= 1e-8 (the clamp passes no gradient below it)
//       ce:    dz_1 = -dz_0 = w_y (softmax_1 - y) / sum_p w_y
//  3. shl_adjoint_kernel: the bilinear adjoint as a gather -- one workgroup per low-resolution
//     pixel sums, in a fixed order, the hi-resolution pixels whose interpolation reads it, then
//     writes d_f[p][c] = W[0][c] dlogit_0[p] + W[1][c] dlogit_1[p].
#include "common.h"
#include "kernels.h"

namespace cwt {

constexpr int SHL_MAXBLK = 256;  // hi-res blocks per image (the final tree's width)
constexpr int SHL_NQ = 6;        // partial sums per image

size_t seg_head_loss_part_doubles(int B) { return (size_t)B * SHL_MAXBLK * SHL_NQ; }
size_t seg_head_loss_sc_floats(int B) { return (size_t)B * 4 + 4; }

struct HiLogits {
  float z0, z1;
};

// the upsampled logits of hi-res pixel (Y, X), as seg_metrics_kernel forms them
__device__ __forceinline__ HiLogits hi_logits(const float* __restrict__ L0, const float* __restrict__ L1, int w,
                                              const Lerp& ly, const Lerp& lx) {
  HiLogits r;
  r.z0 = ly.l0 * (lx.l0 * L0[ly.i0 * w + lx.i0] + lx.l1 * L0[ly.i0 * w + lx.i1]) +
         ly.l1 * (lx.l0 * L0[ly.i1 * w + lx.i0] + lx.l1 * L0[ly.i1 * w + lx.i1]);
  r.z1 = ly.l0 * (lx.l0 * L1[ly.i0 * w + lx.i0] + lx.l1 * L1[ly.i0 * w + lx.i1]) +
         ly.l1 * (lx.l0 * L1[ly.i1 * w + lx.i0] + lx.l1 * L1[ly.i1 * w + lx.i1]);
  return r;
}

__device__ __forceinline__ float sigmoidf(float z) { return 1.0f / (1.0f + expf(-z)); }

__global__ __launch_bounds__(256) void shl_reduce_kernel(const float* __restrict__ logits,
                                                         const int64_t* __restrict__ target, int h, int w, int S,
                                                         float sy, float sx, int dice, double* __restrict__ part) {
  __shared__ double red[4][SHL_NQ];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int b = blockIdx.y;
  const long npix = (long)S * S;
  const long plane = (long)h * w;
  const float* L0 = logits + (long)b * 2 * plane;
  const float* L1 = L0 + plane;
  double a[SHL_NQ] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (long i = (long)blockIdx.x * 256 + t; i < npix; i += (long)gridDim.x * 256) {
    const int Y = (int)(i / S), X = (int)(i - (long)Y * S);
    const Lerp ly = lerp_coord(Y, h, sy), lx = lerp_coord(X, w, sx);
    const HiLogits z = hi_logits(L0, L1, w, ly, lx);
    const int64_t tg = target[(long)b * npix + i];
    if (dice) {
      const float p0 = sigmoidf(z.z0), p1 = sigmoidf(z.z1);
      a[2] += (double)(p0 * p0);
      a[3] += (double)(p1 * p1);
      if (tg == 0) {
        a[0] += (double)p0;
        a[4] += 1.0;
      } else if (tg == 1) {
        a[1] += (double)p1;
        a[5] += 1.0;
      }
    } else if (tg == 0 || tg == 1) {
      const float m = fmaxf(z.z0, z.z1);
      const float lse = m + logf(expf(z.z0 - m) + expf(z.z1 - m));
      a[(int)tg] += 1.0;
      a[2 + (int)tg] += (double)(lse - (tg == 1 ? z.z1 : z.z0));
    }
  }
#pragma unroll
  for (int q = 0; q < SHL_NQ; ++q) {
    for (int o = 32; o > 0; o >>= 1) a[q] += __shfl_xor(a[q], o, 64);
    if (lane == 0) red[wv][q] = a[q];
  }
  __syncthreads();
  if (t < SHL_NQ) part[((long)b * gridDim.x + blockIdx.x) * SHL_NQ + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
}

// one 256-thread workgroup: thread k takes block k's partials, a fixed-shape LDS tree per image.
// sc[b][0..3]: wt_dc {a_0, a_1, c_0, c_1}; ce: sc[0] = w_fg, sc[1] = 1 / sum_p w_y (all images)
__global__ __launch_bounds__(256) void shl_final_kernel(const double* __restrict__ part, int nblk, int B,
                                                        int loss_type, float* __restrict__ sc,
                                                        float* __restrict__ loss_out) {
  __shared__ double d[SHL_NQ][256];
  __shared__ double tot[8][SHL_NQ];
  const int t = threadIdx.x;
  for (int b = 0; b < B; ++b) {
#pragma unroll
    for (int q = 0; q < SHL_NQ; ++q) d[q][t] = t < nblk ? part[((long)b * nblk + t) * SHL_NQ + q] : 0.0;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (t < o) {
#pragma unroll
        for (int q = 0; q < SHL_NQ; ++q) d[q][t] += d[q][t + o];
      }
      __syncthreads();
    }
    if (t < SHL_NQ) tot[b][t] = d[t][0];
    __syncthreads();
  }
  if (t != 0) return;
  if (loss_type == 1) {  // weighted_dice_loss (model_util.py:40-73), reduction 'sum' / n
    double loss = 0.0;
    for (int b = 0; b < B; ++b)
      for (int k = 0; k < 2; ++k) {
        const double I = tot[b][k], D = tot[b][2 + k] + tot[b][4 + k];
        const double Dc = D > 1e-8 ? D : 1e-8;
        loss += 1.0 - 2.0 * I / Dc;
        sc[b * 4 + k] = (float)(-2.0 / (Dc * B));
        sc[b * 4 + 2 + k] = D >= 1e-8 ? (float)(4.0 * I / (D * D * B)) : 0.f;
      }
    loss_out[0] = (float)(loss / B);
  } else {  // weighted_ce_loss (model_util.py:27-37) / CrossEntropyLoss(ignore_index=255)
    double n0 = 0.0, n1 = 0.0, l0 = 0.0, l1 = 0.0;
    for (int b = 0; b < B; ++b) {
      n0 += tot[b][0];
      n1 += tot[b][1];
      l0 += tot[b][2];
      l1 += tot[b][3];
    }
    // no foreground pixel: its weight multiplies nothing
    const double wfg = (loss_type == 0 && n1 > 0.0) ? n0 / n1 : 1.0;
    const double sumw = n0 + wfg * n1;
    // every pixel ignored: 0 / 0 = NaN and zero gradients, as torch returns them
    loss_out[0] = (float)((l0 + wfg * l1) / sumw);
    sc[0] = (float)wfg;
    sc[1] = sumw > 0.0 ? (float)(1.0 / sumw) : 0.f;
  }
}

// weight of low-res index i in the interpolation of the hi-res coordinate l (both taps may hit
// it: at the far edge i0 == i1)
__device__ __forceinline__ float tap_weight(const Lerp& l, int i) {
  return (l.i0 == i ? l.l0 : 0.f) + (l.i1 == i ? l.l1 : 0.f);
}

// hi-res index range [lo, hi] that can read low-res index i: src = scale * dst in (i - 1, i + 1),
// widened by one on each side (the exact membership is tap_weight's, on lerp_coord's own floats)
__device__ __forceinline__ void support_range(int i, float scale, int S, int* lo, int* hi) {
  const float inv = 1.0f / scale;
  *lo = max(0, (int)floorf((float)(i - 1) * inv) - 1);
  *hi = min(S - 1, (int)ceilf((float)(i + 1) * inv) + 1);
}

__global__ __launch_bounds__(256) void shl_adjoint_kernel(const float* __restrict__ W,
                                                          const float* __restrict__ logits,
                                                          const int64_t* __restrict__ target, int h, int w, int C,
                                                          int S, float sy, float sx, int dice,
                                                          const float* __restrict__ sc, float* __restrict__ d_f) {
  __shared__ float red[2][256];
  const int t = threadIdx.x;
  const long plane = (long)h * w;
  const long pix = blockIdx.x;  // b * h * w + y * w + x
  const int b = (int)(pix / plane);
  const int p = (int)(pix - (long)b * plane), y = p / w, x = p - y * w;
  const float* L0 = logits + (long)b * 2 * plane;
  const float* L1 = L0 + plane;
  const int64_t* tg_b = target + (long)b * S * S;
  int Y0, Y1, X0, X1;
  support_range(y, sy, S, &Y0, &Y1);
  support_range(x, sx, S, &X0, &X1);
  const int nx = X1 - X0 + 1, n = (Y1 - Y0 + 1) * nx;
  float s0, s1, s2, s3;
  if (dice) {
    s0 = sc[b * 4];
    s1 = sc[b * 4 + 1];
    s2 = sc[b * 4 + 2];
    s3 = sc[b * 4 + 3];
  } else {
    s0 = sc[0];
    s1 = sc[1];
    s2 = s3 = 0.f;
  }
  float g0 = 0.f, g1 = 0.f;
  for (int i = t; i < n; i += 256) {
    const int Y = Y0 + i / nx, X = X0 + i % nx;
    const Lerp ly = lerp_coord(Y, h, sy), lx = lerp_coord(X, w, sx);
    const float wt = tap_weight(ly, y) * tap_weight(lx, x);
    if (wt == 0.f) continue;
    const HiLogits z = hi_logits(L0, L1, w, ly, lx);
    const int64_t tg = tg_b[(long)Y * S + X];
    if (dice) {
      const float p0 = sigmoidf(z.z0), p1 = sigmoidf(z.z1);
      const float d0 = p0 * (1.f - p0) * ((tg == 0 ? s0 : 0.f) + s2 * p0);
      const float d1 = p1 * (1.f - p1) * ((tg == 1 ? s1 : 0.f) + s3 * p1);
      g0 = fmaf(wt, d0, g0);
      g1 = fmaf(wt, d1, g1);
    } else if (tg == 0 || tg == 1) {
      const float p1 = sigmoidf(z.z1 - z.z0);  // softmax over the two classes
      const float d1 = (tg == 1 ? s0 * (p1 - 1.f) : p1) * s1;
      g1 = fmaf(wt, d1, g1);
      g0 = fmaf(wt, -d1, g0);
    }
  }
  red[0][t] = g0;
  red[1][t] = g1;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      red[0][t] += red[0][t + o];
      red[1][t] += red[1][t + o];
    }
    __syncthreads();
  }
  const float dl0 = red[0][0], dl1 = red[1][0];
  float* dst = d_f + pix * C;
  for (int c = t; c < C; c += 256) dst[c] = fmaf(W[C + c], dl1, W[c] * dl0);
}

int launch_seg_head_loss(const float* W, const float* logits, int B, int h, int w, int C, const int64_t* target, int S,
                         int loss_type, float* loss_out, float* d_f, double* part, float* sc, hipStream_t st) {
  const long npix = (long)S * S;
  const int nblk = (int)std::min<long>(SHL_MAXBLK, cdiv(npix, 256));
  const float sy = align_corners_scale(h, S), sx = align_corners_scale(w, S);
  const int dice = loss_type == 1;
  hipLaunchKernelGGL(shl_reduce_kernel, dim3(nblk, B), dim3(256), 0, st, logits, target, h, w, S, sy, sx, dice, part);
  CWT_LAUNCH_CHECK();
  hipLaunchKernelGGL(shl_final_kernel, dim3(1), dim3(256), 0, st, (const double*)part, nblk, B, loss_type, sc, loss_out);
  CWT_LAUNCH_CHECK();
  if (d_f) {
    hipLaunchKernelGGL(shl_adjoint_kernel, dim3((unsigned)((long)B * h * w)), dim3(256), 0, st, W, logits, target, h, w,
                       C, S, sy, sx, dice, (const float*)sc, d_f);
    CWT_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace cwt
