// Per-pixel N-way label operations of a class-incremental episode (reference model_util.py:119-127
// reset_spt_label; model_util.py:158-175 compress_pred / pred2bmask with train_cca.py:348-370).
// Each takes low-resolution logits [B][N][h][w] and upsamples them to S x S (bilinear,
// align_corners=True) in registers, one thread per hi-res pixel, for any h, w, S >= 2.  The
// interpolation and the log-sum-exps run in float64 on the fp32 logits: the labels and the counts
// are then those of the exact upsample wherever two classes are not tied to the last bit, and
// log(1 - p_fg) stays finite where p_fg rounds to 1 in float32.  Two identical logit planes give
// identical values, so the first-index rule of torch.argmax is kept on exact ties.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace cwt {

constexpr int NPX_MAXBLK = 256;

struct LerpD {
  int i0, i1;
  double l0, l1;
};
// upsample_bilinear2d(align_corners=True) in float64: scale = (in - 1) / (out - 1), src = scale * dst
__device__ __forceinline__ LerpD lerp_coord_d(int dst, int in_size, int out_size) {
  LerpD r;
  const double scale = out_size > 1 ? (double)(in_size - 1) / (double)(out_size - 1) : 0.0;
  const double src = scale * (double)dst;
  r.i0 = min((int)src, in_size - 1);
  r.i1 = r.i0 + (r.i0 < in_size - 1 ? 1 : 0);
  r.l1 = src - (double)r.i0;
  r.l0 = 1.0 - r.l1;
  return r;
}

struct PixelTaps {
  int o00, o01, o10, o11;
  double ly0, ly1, lx0, lx1;
  __device__ __forceinline__ double at(const float* __restrict__ plane) const {
    return ly0 * (lx0 * (double)plane[o00] + lx1 * (double)plane[o01]) +
           ly1 * (lx0 * (double)plane[o10] + lx1 * (double)plane[o11]);
  }
};
__device__ __forceinline__ PixelTaps pixel_taps(int Y, int X, int h, int w, int S) {
  const LerpD ly = lerp_coord_d(Y, h, S), lx = lerp_coord_d(X, w, S);
  return PixelTaps{ly.i0 * w + lx.i0, ly.i0 * w + lx.i1, ly.i1 * w + lx.i0, ly.i1 * w + lx.i1,
                   ly.l0, ly.l1, lx.l0, lx.l1};
}

__global__ __launch_bounds__(256) void relabel_support_kernel(const float* __restrict__ logits,
                                                              const int64_t* __restrict__ s_label, int N, int h, int w,
                                                              int S, int idx_cls, int64_t* __restrict__ out) {
  const long npix = (long)S * S, plane = (long)h * w;
  const int b = blockIdx.y;
  const float* L = logits + (long)b * N * plane;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < npix; i += (long)gridDim.x * 256) {
    const int64_t s = s_label[(long)b * npix + i];
    int64_t o = s == 1 ? (int64_t)idx_cls : s;
    if (s == 0) {
      const int Y = (int)(i / S), X = (int)(i - (long)Y * S);
      const PixelTaps tp = pixel_taps(Y, X, h, w, S);
      int am = 0;
      double best = 0.0;
      for (int c = 0; c < N; ++c) {
        const double z = c == idx_cls ? -1000.0 : tp.at(L + c * plane);
        if (c == 0 || z > best) {  // the first maximal index
          best = z;
          am = c;
        }
      }
      o = am == 1 ? idx_cls : am;  // every 1 -- a pseudo-label of base class 1 too -- becomes idx_cls
    }
    out[(long)b * npix + i] = o;
  }
}

int launch_relabel_support(const float* logits, const int64_t* s_label, int B, int N, int h, int w, int S,
                           int idx_cls, int64_t* out, hipStream_t st) {
  const long npix = (long)S * S;
  hipLaunchKernelGGL(relabel_support_kernel, dim3((unsigned)std::min<long>(1024, cdiv(npix, 256)), B), dim3(256), 0,
                     st, logits, s_label, N, h, w, S, idx_cls, out);
  CWT_LAUNCH_CHECK();
  return 0;
}

// counts[b][blk][0..5] = {inter0, inter1, out0, out1, tgt0, tgt1}, cep[b][blk] = {sum nll, count}
__global__ __launch_bounds__(256) void seg_metrics_nway_kernel(const float* __restrict__ logits,
                                                               const int64_t* __restrict__ target, int N, int h,
                                                               int w, int S, int idx_cls,
                                                               unsigned* __restrict__ counts,
                                                               double* __restrict__ cep) {
  __shared__ unsigned cnt[4][6];
  __shared__ double cel[4][2];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int b = blockIdx.y;
  const long npix = (long)S * S, plane = (long)h * w;
  const float* L = logits + (long)b * N * plane;
  unsigned c6[6] = {0, 0, 0, 0, 0, 0};
  double nll = 0.0;
  unsigned nvalid = 0;
  for (long i = (long)blockIdx.x * 256 + t; i < npix; i += (long)gridDim.x * 256) {
    const int64_t tg = target[(long)b * npix + i];
    if (tg == 255) continue;
    const int Y = (int)(i / S), X = (int)(i - (long)Y * S);
    const PixelTaps tp = pixel_taps(Y, X, h, w, S);
    int am = 0;
    double best = 0.0, zf = 0.0, mo = 0.0;  // the argmax, class idx_cls's logit, the other classes' max
    bool have_o = false;
    for (int c = 0; c < N; ++c) {
      const double z = tp.at(L + c * plane);
      if (c == 0 || z > best) {
        best = z;
        am = c;
      }
      if (c == idx_cls) {
        zf = z;
      } else if (!have_o || z > mo) {
        mo = z;
        have_o = true;
      }
    }
    const int pred = am == idx_cls ? 1 : 0;
    c6[2 + pred]++;
    if (tg == 0 || tg == 1) {
      c6[4 + (int)tg]++;
      if (pred == tg) c6[pred]++;
      double so = 0.0;
      for (int c = 0; c < N; ++c)
        if (c != idx_cls) so += exp(tp.at(L + c * plane) - mo);
      // a = lse(other classes) - z_fg: -log p_fg = softplus(a), -log(1 - p_fg) = softplus(-a)
      const double a = mo + log(so) - zf, x = tg == 1 ? a : -a;
      nll += fmax(x, 0.0) + log1p(exp(-fabs(x)));
      nvalid++;
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k)
    for (int o = 32; o > 0; o >>= 1) c6[k] += __shfl_xor(c6[k], o, 64);
  for (int o = 32; o > 0; o >>= 1) {
    nll += __shfl_xor(nll, o, 64);
    nvalid += __shfl_xor(nvalid, o, 64);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) cnt[wv][k] = c6[k];
    cel[wv][0] = nll;
    cel[wv][1] = (double)nvalid;
  }
  __syncthreads();
  // per-block partials, summed in block order by the final kernel: no atomics, fixed order
  const long pb = (long)b * gridDim.x + blockIdx.x;
  if (t < 6) counts[pb * 6 + t] = cnt[0][t] + cnt[1][t] + cnt[2][t] + cnt[3][t];
  if (t < 2) cep[pb * 2 + t] = (cel[0][t] + cel[1][t]) + (cel[2][t] + cel[3][t]);
}

__global__ __launch_bounds__(NPX_MAXBLK) void seg_metrics_nway_final_kernel(const unsigned* __restrict__ counts,
                                                                            const double* __restrict__ cep, int nblk,
                                                                            float* __restrict__ iut,
                                                                            double* __restrict__ ce) {
  __shared__ unsigned c[6][NPX_MAXBLK];
  __shared__ double d[2][NPX_MAXBLK];
  const int b = blockIdx.x, t = threadIdx.x;
  const bool have = t < nblk;
#pragma unroll
  for (int q = 0; q < 6; ++q) c[q][t] = have ? counts[((long)b * nblk + t) * 6 + q] : 0u;
  d[0][t] = have ? cep[((long)b * nblk + t) * 2] : 0.0;
  d[1][t] = have ? cep[((long)b * nblk + t) * 2 + 1] : 0.0;
  __syncthreads();
  for (int o = NPX_MAXBLK / 2; o > 0; o >>= 1) {
    if (t < o) {
#pragma unroll
      for (int q = 0; q < 6; ++q) c[q][t] += c[q][t + o];
      d[0][t] += d[0][t + o];
      d[1][t] += d[1][t + o];
    }
    __syncthreads();
  }
  if (t < 2) {
    iut[b * 6 + t] = (float)c[t][0];
    iut[b * 6 + 2 + t] = (float)(c[2 + t][0] + c[4 + t][0] - c[t][0]);  // union = output + target - intersection
    iut[b * 6 + 4 + t] = (float)c[4 + t][0];
    if (ce) ce[b * 2 + t] = d[t][0];
  }
}

size_t nway_metrics_ws_bytes(int B) { return (size_t)B * NPX_MAXBLK * (6 * sizeof(unsigned) + 2 * sizeof(double)) + 16; }

int launch_seg_metrics_nway(const float* logits, const int64_t* target, int B, int N, int h, int w, int S,
                            int idx_cls, float* iut, double* ce, void* ws, hipStream_t st) {
  const long npix = (long)S * S;
  const int nblk = (int)std::min<long>(NPX_MAXBLK, cdiv(npix, 256));
  double* cep = (double*)ws;  // [B][nblk][2], then the counts [B][nblk][6]
  unsigned* counts = (unsigned*)(cep + (long)B * NPX_MAXBLK * 2);
  hipLaunchKernelGGL(seg_metrics_nway_kernel, dim3(nblk, B), dim3(256), 0, st, logits, target, N, h, w, S, idx_cls,
                     counts, cep);
  CWT_LAUNCH_CHECK();
  hipLaunchKernelGGL(seg_metrics_nway_final_kernel, dim3(B), dim3(NPX_MAXBLK), 0, st, (const unsigned*)counts,
                     (const double*)cep, nblk, iut, ce);
  CWT_LAUNCH_CHECK();
  return 0;
}

// pred_q2 (train_cca.py:347, 353): m = softmax(z0) (1 - att_wt) + softmax(z1) att_wt on the two
// upsampled logit tensors, the mask argmax_c m == idx_cls (the first maximal index).  Three sweeps
// over the classes per pixel (the maxima, the exponential sums, the mix), nothing kept per class.
// Writes seg_metrics_nway_kernel's per-block counts (and zero NLL partials) for the same final kernel.
__global__ __launch_bounds__(256) void seg_metrics_nway_mix_kernel(const float* __restrict__ logits0,
                                                                   const float* __restrict__ logits1, double att_wt,
                                                                   const int64_t* __restrict__ target, int N, int h,
                                                                   int w, int S, int idx_cls,
                                                                   unsigned* __restrict__ counts,
                                                                   double* __restrict__ cep) {
  __shared__ unsigned cnt[4][6];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int b = blockIdx.y;
  const long npix = (long)S * S, plane = (long)h * w;
  const float* L0 = logits0 + (long)b * N * plane;
  const float* L1 = logits1 + (long)b * N * plane;
  const double w0 = 1.0 - att_wt, w1 = att_wt;
  unsigned c6[6] = {0, 0, 0, 0, 0, 0};
  for (long i = (long)blockIdx.x * 256 + t; i < npix; i += (long)gridDim.x * 256) {
    const int64_t tg = target[(long)b * npix + i];
    if (tg == 255) continue;
    const int Y = (int)(i / S), X = (int)(i - (long)Y * S);
    const PixelTaps tp = pixel_taps(Y, X, h, w, S);
    double m0 = tp.at(L0), m1 = tp.at(L1);
    for (int c = 1; c < N; ++c) {
      m0 = fmax(m0, tp.at(L0 + c * plane));
      m1 = fmax(m1, tp.at(L1 + c * plane));
    }
    double s0 = 0.0, s1 = 0.0;
    for (int c = 0; c < N; ++c) {
      s0 += exp(tp.at(L0 + c * plane) - m0);
      s1 += exp(tp.at(L1 + c * plane) - m1);
    }
    int am = 0;
    double best = 0.0;
    for (int c = 0; c < N; ++c) {
      const double v = exp(tp.at(L0 + c * plane) - m0) / s0 * w0 + exp(tp.at(L1 + c * plane) - m1) / s1 * w1;
      if (c == 0 || v > best) {  // the first maximal index
        best = v;
        am = c;
      }
    }
    const int pred = am == idx_cls ? 1 : 0;
    c6[2 + pred]++;
    if (tg == 0 || tg == 1) {
      c6[4 + (int)tg]++;
      if (pred == tg) c6[pred]++;
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k)
    for (int o = 32; o > 0; o >>= 1) c6[k] += __shfl_xor(c6[k], o, 64);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) cnt[wv][k] = c6[k];
  }
  __syncthreads();
  const long pb = (long)b * gridDim.x + blockIdx.x;
  if (t < 6) counts[pb * 6 + t] = cnt[0][t] + cnt[1][t] + cnt[2][t] + cnt[3][t];
  if (t < 2) cep[pb * 2 + t] = 0.0;
}

int launch_seg_metrics_nway_mix(const float* logits0, const float* logits1, double att_wt, const int64_t* target, int B,
                                int N, int h, int w, int S, int idx_cls, float* iut, void* ws, hipStream_t st) {
  const long npix = (long)S * S;
  const int nblk = (int)std::min<long>(NPX_MAXBLK, cdiv(npix, 256));
  double* cep = (double*)ws;  // the layout of launch_seg_metrics_nway
  unsigned* counts = (unsigned*)(cep + (long)B * NPX_MAXBLK * 2);
  hipLaunchKernelGGL(seg_metrics_nway_mix_kernel, dim3(nblk, B), dim3(256), 0, st, logits0, logits1, att_wt, target, N,
                     h, w, S, idx_cls, counts, cep);
  CWT_LAUNCH_CHECK();
  hipLaunchKernelGGL(seg_metrics_nway_final_kernel, dim3(B), dim3(NPX_MAXBLK), 0, st, (const unsigned*)counts,
                     (const double*)cep, nblk, iut, (double*)nullptr);
  CWT_LAUNCH_CHECK();
  return 0;
}

}  // namespace cwt
