// Per-pixel N-way label operations of a class-incremental episode (reference model_util.py:119-127
// reset_spt_label; model_util.py:158-175 compress_pred / pred2bmask with train_cca.py:348-370).
// Each takes low-resolution logits [B][N][h][w] and upsamples them to S x S (bilinear,
// align_corners=True) in registers, one thread per hi-res pixel, for any h, w, S >= 2.  The
// interpolation and the log-sum-exps run in float64 on the fp32 logits: the labels and the counts
// are then those of the exact upsample wherever two classes are not tied to the last bit, and
// log(1 - p_fg) stays finite where p_fg rounds to 1 in float32.  Two identical logit planes give
// identical values, so the first-index rule of torch.argmax is kept on exact ties.
#include <algorithm>

#include "kernels.h"
#include "pixel_pass.h"

namespace cwt {

// the taps of hi-res pixel (Y, X) into a class plane [h][w]
__device__ __forceinline__ PixelTaps plane_taps(int Y, int X, int h, int w, int S) {
  return pixel_taps(lerp_coord_d(Y, h, S), lerp_coord_d(X, w, S), w, 1);
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
      const PixelTaps tp = plane_taps(Y, X, h, w, S);
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

// counts[b][blk][0..5] = {inter0, inter1, out0, out1, tgt0, tgt1}, cep[b][blk] = sum nll
__global__ __launch_bounds__(256) void seg_metrics_nway_kernel(const float* __restrict__ logits,
                                                               const int64_t* __restrict__ target, int N, int h,
                                                               int w, int S, int idx_cls,
                                                               unsigned* __restrict__ counts,
                                                               double* __restrict__ cep) {
  const int t = threadIdx.x;
  const int b = blockIdx.y;
  const long npix = (long)S * S, plane = (long)h * w;
  const float* L = logits + (long)b * N * plane;
  unsigned c6[PIX_NQ] = {0, 0, 0, 0, 0, 0};
  double nll = 0.0;
  for (long i = (long)blockIdx.x * 256 + t; i < npix; i += (long)gridDim.x * 256) {
    const int64_t tg = target[(long)b * npix + i];
    if (tg == 255) continue;
    const int Y = (int)(i / S), X = (int)(i - (long)Y * S);
    const PixelTaps tp = plane_taps(Y, X, h, w, S);
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
    count_pred(c6, am == idx_cls ? 1 : 0, tg);
    if (tg == 0 || tg == 1) {
      double so = 0.0;
      for (int c = 0; c < N; ++c)
        if (c != idx_cls) so += exp(tp.at(L + c * plane) - mo);
      // a = lse(other classes) - z_fg: -log p_fg = softplus(a), -log(1 - p_fg) = softplus(-a)
      const double a = mo + log(so) - zf, x = tg == 1 ? a : -a;
      nll += fmax(x, 0.0) + log1p(exp(-fabs(x)));
    }
  }
  block_partials<1, PIX_NQ>(&nll, c6, (long)b * gridDim.x + blockIdx.x, cep, counts);
}

// one 256-thread block per image: iut from the counts, {sum nll, count} from cep when ce is asked for
__global__ __launch_bounds__(PIX_MAXBLK) void seg_metrics_nway_final_kernel(const unsigned* __restrict__ counts,
                                                                            const double* __restrict__ cep, int nblk,
                                                                            float* __restrict__ iut,
                                                                            double* __restrict__ ce) {
  __shared__ unsigned c[PIX_NQ][PIX_MAXBLK];
  __shared__ double d[1][PIX_MAXBLK];
  const int b = blockIdx.x;
  metrics_final(counts + (long)b * nblk * PIX_NQ, cep + (long)b * nblk, nblk, iut + b * 6, ce ? ce + b * 2 : nullptr, d,
                c);
}

size_t nway_metrics_ws_bytes(int B) { return (size_t)B * PIX_MAXBLK * (6 * sizeof(unsigned) + 2 * sizeof(double)) + 16; }

int launch_seg_metrics_nway(const float* logits, const int64_t* target, int B, int N, int h, int w, int S,
                            int idx_cls, float* iut, double* ce, void* ws, hipStream_t st) {
  const long npix = (long)S * S;
  const int nblk = (int)std::min<long>(PIX_MAXBLK, cdiv(npix, 256));
  double* cep = (double*)ws;  // [B][nblk] (2 x PIX_MAXBLK doubles an image kept), then the counts [B][nblk][6]
  unsigned* counts = (unsigned*)(cep + (long)B * PIX_MAXBLK * 2);
  hipLaunchKernelGGL(seg_metrics_nway_kernel, dim3(nblk, B), dim3(256), 0, st, logits, target, N, h, w, S, idx_cls,
                     counts, cep);
  CWT_LAUNCH_CHECK();
  hipLaunchKernelGGL(seg_metrics_nway_final_kernel, dim3(B), dim3(PIX_MAXBLK), 0, st, (const unsigned*)counts,
                     (const double*)cep, nblk, iut, ce);
  CWT_LAUNCH_CHECK();
  return 0;
}

// pred_q2 (train_cca.py:347, 353): m = softmax(z0) (1 - att_wt) + softmax(z1) att_wt on the two
// upsampled logit tensors, the mask argmax_c m == idx_cls (the first maximal index).  Three sweeps
// over the classes per pixel (the maxima, the exponential sums, the mix), nothing kept per class.
// Writes seg_metrics_nway_kernel's per-block counts for the same final kernel (no NLL: ce is NULL there).
__global__ __launch_bounds__(256) void seg_metrics_nway_mix_kernel(const float* __restrict__ logits0,
                                                                   const float* __restrict__ logits1, double att_wt,
                                                                   const int64_t* __restrict__ target, int N, int h,
                                                                   int w, int S, int idx_cls,
                                                                   unsigned* __restrict__ counts) {
  const int t = threadIdx.x;
  const int b = blockIdx.y;
  const long npix = (long)S * S, plane = (long)h * w;
  const float* L0 = logits0 + (long)b * N * plane;
  const float* L1 = logits1 + (long)b * N * plane;
  const double w0 = 1.0 - att_wt, w1 = att_wt;
  unsigned c6[PIX_NQ] = {0, 0, 0, 0, 0, 0};
  for (long i = (long)blockIdx.x * 256 + t; i < npix; i += (long)gridDim.x * 256) {
    const int64_t tg = target[(long)b * npix + i];
    if (tg == 255) continue;
    const int Y = (int)(i / S), X = (int)(i - (long)Y * S);
    const PixelTaps tp = plane_taps(Y, X, h, w, S);
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
    count_pred(c6, am == idx_cls ? 1 : 0, tg);
  }
  block_partials<0, PIX_NQ>(nullptr, c6, (long)b * gridDim.x + blockIdx.x, nullptr, counts);
}

int launch_seg_metrics_nway_mix(const float* logits0, const float* logits1, double att_wt, const int64_t* target, int B,
                                int N, int h, int w, int S, int idx_cls, float* iut, void* ws, hipStream_t st) {
  const long npix = (long)S * S;
  const int nblk = (int)std::min<long>(PIX_MAXBLK, cdiv(npix, 256));
  unsigned* counts = (unsigned*)((double*)ws + (long)B * PIX_MAXBLK * 2);  // the layout of launch_seg_metrics_nway
  hipLaunchKernelGGL(seg_metrics_nway_mix_kernel, dim3(nblk, B), dim3(256), 0, st, logits0, logits1, att_wt, target, N,
                     h, w, S, idx_cls, counts);
  CWT_LAUNCH_CHECK();
  hipLaunchKernelGGL(seg_metrics_nway_final_kernel, dim3(B), dim3(PIX_MAXBLK), 0, st, (const unsigned*)counts,
                     (const double*)nullptr, nblk, iut, (double*)nullptr);
  CWT_LAUNCH_CHECK();
  return 0;
}

}  // namespace cwt
