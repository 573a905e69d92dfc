// The hi-res pixel pass that nway_pixel.hip, seg_loss.hip and seg_loss_nway.hip share:
// low-resolution logits are upsampled (bilinear, align_corners=True) in registers at every
// pixel of the S x S label, per-pixel terms are summed per block, the per-block partial rows are
// summed by a 256-wide LDS tree, and the loss heads gather the bilinear adjoint per low-res pixel.
// seg.hip's seg_metrics kernels run the same pass in their own text: the NLL's bits and the tie
// of two identical planes hang on how hipcc pairs that kernel's FMAs, which moved with every
// shared piece tried there.
//
// The rules every user of this file keeps ("The hi-res pixel pass"):
//  - every sum has a fixed order: wave shuffle, one LDS row per wave, (r0 + r1) + (r2 + r3), one
//    partial row per block (nothing zeroed first, no atomics), then the tree in block order;
//  - at the far edge i0 == i1 and both taps weigh the same low-res index;
//  - an argmax tie goes to class 0 (callers compare with >);
//  - the dice denominator's clamp at 1e-8 passes no gradient below it.
#pragma once
#include "common.h"

namespace cwt {

constexpr int PIX_MAXBLK = 256;  // hi-res blocks per image: the final tree's width
constexpr int PIX_NQ = 6;        // sums / counters per image

// ---- coordinates and taps ----

struct LerpD {
  int i0, i1;
  double l0, l1;
};
// upsample_bilinear2d(align_corners=True) in float64: src = dst (in - 1) / (out - 1), out >= 2
__device__ __forceinline__ LerpD lerp_coord_d(int dst, int in_size, int out_size) {
  LerpD r;
  const double src = (double)(in_size - 1) / (double)(out_size - 1) * (double)dst;
  r.i0 = min((int)src, in_size - 1);
  r.i1 = r.i0 + (r.i0 < in_size - 1 ? 1 : 0);
  r.l1 = src - (double)r.i0;
  r.l0 = 1.0 - r.l1;
  return r;
}

// the four taps of one hi-res pixel: offsets in floats into an image's logits, whose low-res
// pixels lie `stride` floats apart (1: a class plane [h][w]; N: pixel-major [h*w][N]); the caller
// advances the pointer by class
struct PixelTaps {
  int o00, o01, o10, o11;
  double ly0, ly1, lx0, lx1;
  __device__ __forceinline__ double at(const float* __restrict__ L) const {
    return ly0 * (lx0 * (double)L[o00] + lx1 * (double)L[o01]) + ly1 * (lx0 * (double)L[o10] + lx1 * (double)L[o11]);
  }
};
__device__ __forceinline__ PixelTaps pixel_taps(const LerpD& ly, const LerpD& lx, int w, int stride) {
  return PixelTaps{(ly.i0 * w + lx.i0) * stride, (ly.i0 * w + lx.i1) * stride, (ly.i1 * w + lx.i0) * stride,
                   (ly.i1 * w + lx.i1) * stride, ly.l0, ly.l1, lx.l0, lx.l1};
}

// the two upsampled fp32 logits of a hi-res pixel on common.h's float Lerp (2-way, plane-major)
struct HiLogits {
  float z0, z1;
};
__device__ __forceinline__ HiLogits hi_logits(const float* __restrict__ L0, const float* __restrict__ L1, int w,
                                              const Lerp& ly, const Lerp& lx) {
  HiLogits r;
  r.z0 = ly.l0 * (lx.l0 * L0[ly.i0 * w + lx.i0] + lx.l1 * L0[ly.i0 * w + lx.i1]) +
         ly.l1 * (lx.l0 * L0[ly.i1 * w + lx.i0] + lx.l1 * L0[ly.i1 * w + lx.i1]);
  r.z1 = ly.l0 * (lx.l0 * L1[ly.i0 * w + lx.i0] + lx.l1 * L1[ly.i0 * w + lx.i1]) +
         ly.l1 * (lx.l0 * L1[ly.i1 * w + lx.i0] + lx.l1 * L1[ly.i1 * w + lx.i1]);
  return r;
}

// weight of low-res index i in the interpolation of a hi-res coordinate (Lerp or LerpD); both taps
// may hit it: at the far edge i0 == i1
template <typename L>
__device__ __forceinline__ auto tap_weight(const L& l, int i) -> decltype(l.l0) {
  using T = decltype(l.l0);
  return (l.i0 == i ? l.l0 : T(0)) + (l.i1 == i ? l.l1 : T(0));
}

// hi-res index range [lo, hi] that can read low-res index i: src = dst / inv in (i - 1, i + 1),
// widened by one on each side (the exact membership is tap_weight's); inv = (S - 1) / (in - 1) in
// the caller's own arithmetic, float or double
template <typename T>
__device__ __forceinline__ void support_range(int i, T inv, int S, int* lo, int* hi) {
  *lo = max(0, (int)floor((T)(i - 1) * inv) - 1);
  *hi = min(S - 1, (int)ceil((T)(i + 1) * inv) + 1);
}

// ---- counting ----

// c6 = {inter_0, inter_1, out_0, out_1, tgt_0, tgt_1} of a pixel whose label is not 255 (the
// caller decides what a 255 does; none of them counts it here)
__device__ __forceinline__ void count_pred(unsigned (&c6)[PIX_NQ], int pred, int64_t tg) {
  c6[2 + pred]++;
  if (tg == 0 || tg == 1) {
    c6[4 + (int)tg]++;
    if (pred == (int)tg) c6[pred]++;
  }
}

// ---- block partials ----

// Sums NQ doubles and NC counts per thread over a 256-thread workgroup and writes them as row
// `row` of the partials (a NULL table is not written).  Every thread calls it, once per kernel.
template <int NQ, int NC>
__device__ __forceinline__ void block_partials(double* a, unsigned* c, long row, double* __restrict__ part,
                                               unsigned* __restrict__ counts) {
  __shared__ double red[4][NQ ? NQ : 1];
  __shared__ unsigned cred[4][NC ? NC : 1];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
#pragma unroll
  for (int q = 0; q < NC; ++q) {
    for (int o = 32; o > 0; o >>= 1) c[q] += __shfl_xor(c[q], o, 64);
    if (lane == 0) cred[wv][q] = c[q];
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    for (int o = 32; o > 0; o >>= 1) a[q] += __shfl_xor(a[q], o, 64);
    if (lane == 0) red[wv][q] = a[q];
  }
  __syncthreads();
  if (part && t < NQ) part[row * NQ + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
  if (counts && t < NC) counts[row * NC + t] = cred[0][t] + cred[1][t] + cred[2][t] + cred[3][t];
}

// The 256-wide tree over one image's partial rows (part / counts point at its row 0): thread k
// takes block k's row, rows from nblk on count as zero; afterwards d[q][0] and c[q][0] hold the
// sums.  Every thread of a 256-thread workgroup calls it; it ends on a barrier.
template <int NQ, int NC>
__device__ __forceinline__ void tree_partials(const double* __restrict__ part, const unsigned* __restrict__ counts,
                                              int nblk, double (*d)[PIX_MAXBLK], unsigned (*c)[PIX_MAXBLK]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int q = 0; q < NQ; ++q) d[q][t] = t < nblk ? part[(long)t * NQ + q] : 0.0;
#pragma unroll
  for (int q = 0; q < NC; ++q) c[q][t] = t < nblk ? counts[(long)t * NC + q] : 0u;
  __syncthreads();
  for (int o = PIX_MAXBLK / 2; o > 0; o >>= 1) {
    if (t < o) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) d[q][t] += d[q][t + o];
#pragma unroll
      for (int q = 0; q < NC; ++q) c[q][t] += c[q][t + o];
    }
    __syncthreads();
  }
}

// thread k = 0, 1 writes class k of an image's {intersection, union, target} from the counter sums
__device__ __forceinline__ void write_iut(float* __restrict__ iut, const unsigned (*c)[PIX_MAXBLK], int k) {
  iut[k] = (float)c[k][0];
  iut[2 + k] = (float)(c[2 + k][0] + c[4 + k][0] - c[k][0]);  // union = output + target - intersection
  iut[4 + k] = (float)c[4 + k][0];
}

// The metrics kernels' final step for one image (a 256-thread workgroup; the pointers are the
// image's own): iut from the counter sums and, when ce is asked for, ce = {sum nll, labelled pixels}
// from the per-block NLL sums -- a pixel adds to the NLL exactly when it adds to tgt_0 or tgt_1.
__device__ __forceinline__ void metrics_final(const unsigned* __restrict__ counts, const double* __restrict__ nll_part,
                                              int nblk, float* __restrict__ iut, double* __restrict__ ce,
                                              double (*d)[PIX_MAXBLK], unsigned (*c)[PIX_MAXBLK]) {
  if (ce)
    tree_partials<1, PIX_NQ>(nll_part, counts, nblk, d, c);
  else
    tree_partials<0, PIX_NQ>(nullptr, counts, nblk, d, c);
  const int t = threadIdx.x;
  if (t < 2) write_iut(iut, c, t);
  if (ce && t == 0) {
    ce[0] = d[0][0];
    ce[1] = (double)(c[4][0] + c[5][0]);
  }
}

// ---- the loss heads' arithmetic ----

// From the six totals per image (dice: {I_0, I_1, sum q_0^2, sum q_1^2, sum t_0, sum t_1}; CE:
// {n_0, n_1, sum nll | y = 0, sum nll | y = 1}) the loss and the gradient's coefficients, by one thread:
//   dice: sc[b][0..3] = {a_0, a_1, c_0, c_1}, a_k = -2 / (max(D_k, 1e-8) B), c_k = 4 I_k / (D_k^2 B)
//         where D_k >= 1e-8 (the clamp passes no gradient below it)
//   CE:   sc[0] = w_fg, sc[1] = 1 / sum_p w_y (all images)
__device__ __forceinline__ void head_loss_coef(const double (*tot)[PIX_NQ], int B, int loss_type,
                                               float* __restrict__ sc, float* __restrict__ loss_out) {
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

// One 256-thread workgroup, looping over the B <= 8 images: the tree over each image's partials,
// iut from the counts (COUNTS: the N-way head's), then thread 0 forms the loss and sc.
template <bool COUNTS>
__global__ __launch_bounds__(PIX_MAXBLK) void head_final_kernel(const double* __restrict__ part,
                                                               const unsigned* __restrict__ counts, int nblk, int B,
                                                               int loss_type, float* __restrict__ sc,
                                                               float* __restrict__ loss_out, float* __restrict__ iut) {
  __shared__ double d[PIX_NQ][PIX_MAXBLK];
  __shared__ unsigned cn[COUNTS ? PIX_NQ : 1][PIX_MAXBLK];
  __shared__ double tot[8][PIX_NQ];
  const int t = threadIdx.x;
  for (int b = 0; b < B; ++b) {
    tree_partials<PIX_NQ, COUNTS ? PIX_NQ : 0>(part + (long)b * nblk * PIX_NQ,
                                               COUNTS ? counts + (long)b * nblk * PIX_NQ : nullptr, nblk, d, cn);
    if (t < PIX_NQ) tot[b][t] = d[t][0];
    if (COUNTS && iut && t < 2) write_iut(iut + b * 6, cn, t);
    __syncthreads();
  }
  if (t == 0) head_loss_coef(tot, B, loss_type, sc, loss_out);
}

// the coefficients of image b as the adjoint kernels read them
struct HeadCoef {
  float s0, s1, s2, s3;
};
__device__ __forceinline__ HeadCoef load_coef(const float* __restrict__ sc, int b, int dice) {
  if (dice) return HeadCoef{sc[b * 4], sc[b * 4 + 1], sc[b * 4 + 2], sc[b * 4 + 3]};
  return HeadCoef{sc[0], sc[1], 0.f, 0.f};
}

}  // namespace cwt
