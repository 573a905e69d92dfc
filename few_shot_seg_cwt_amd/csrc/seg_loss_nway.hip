// The class-incremental trainer's loss head (reference src/train_cca.py:177-198): on the low-resolution
// N-way classifier logits [B][h][w][N] (cwt_linear's, pixel-major), the bilinear align_corners=True
// upsample to the S x S label, p = softmax_N(z)[idx_cls], q = [1 - p, p] (compress_pred(., idx_cls,
// 'lg'), src/model/model_util.py:158-166; F.softmax without dim on a 4-D tensor is dim = 1),
// SegLoss(loss_type)(q, target, 'pb') (model_util.py:9-73) and the gradient carried back through the
// softmax, the upsample and the classifier to the feature map f.
//
// The reference's arithmetic, kept as it is:
//   wt_dc / dc: weighted_dice_loss on q without the sigmoid ('pb'); t_k = [label == k], pixels
//               labelled 255 have t = 0 in both channels and still count in sum q^2; clamp at 1e-8; / B.
//   ce, wt_ce:  SegLoss.forward ignores input_type on these branches, so the two-channel
//               probabilities q go into CrossEntropyLoss(ignore_index=255) as if they were logits:
//               nll = log(exp(q_0) + exp(q_1)) - q_y.  wt_ce weights class 1 by #bg / #fg of the
//               target.  This is what train_cca.py computes; it is restated, not corrected.
//
// Four launches on pixel_pass.h's pieces, the S x S x N logits never stored; the reduce pass keeps
// (lse, p, 1 - p) per hi-res pixel in the workspace (3 floats a pixel) so that the adjoint's gather
// does not redo an N-way log-sum-exp for each low-res pixel that a hi-res pixel feeds:
//  1. shn_reduce_kernel: one thread per hi-res pixel; the interpolation and the softmax's max run in
//     float64 on the fp32 logits (as nway_pixel.hip), 1 - p is the other classes' share of the
//     exponential sum (no cancellation where p rounds to 1); per-block double partials of
//       wt_dc: {I_0, I_1, sum q_0^2, sum q_1^2, sum t_0, sum t_1} per image
//       ce:    {n_0, n_1, sum nll | y = 0, sum nll | y = 1, -, -} per image
//     and integer counts of the mask p > 1 - p against the target (train_cca.py:211-213: argmax of
//     the compressed prediction, a tie goes to class 0, 255 ignored).
//  2. head_final_kernel<true>: the loss, iut, and the coefficients
//       wt_dc: dL/dq_k = a_k t_k + c_k q_k
//       ce:    dL/dq_k = w_y (softmax2(q)_k - [k == y]) / sum_p w_y
//  3. shn_adjoint_kernel: dL/dp = dL/dq_1 - dL/dq_0, dz_c = (dL/dp) p ([c == idx_cls] - softmax_c);
//     the bilinear adjoint as a gather -- one workgroup per low-res pixel over the hi-res pixels
//     whose interpolation reads it, lanes over the classes -- then
//     d_f[pix][:] = sum_c W[c][:] dlogit_c[pix] in plain fp32 FMAs (N x C per pixel: small).
//  4. shn_logits_out_kernel (when logits_out is given): the pixel-major logits copied to [B][N][h][w].
#include <algorithm>

#include "kernels.h"
#include "pixel_pass.h"

namespace cwt {

size_t seg_head_loss_nway_part_bytes(int B) {
  return (size_t)B * PIX_MAXBLK * PIX_NQ * (sizeof(double) + sizeof(unsigned));
}
size_t seg_head_loss_nway_pix_floats(int B, int S) { return (size_t)3 * B * S * S; }

// pix: [3][B * S * S] planes {lse, p, 1 - p}, or NULL (no gradient asked for)
__global__ __launch_bounds__(256) void shn_reduce_kernel(const float* __restrict__ logits,
                                                         const int64_t* __restrict__ target, int N, int h, int w,
                                                         int S, int idx_cls, int dice, double* __restrict__ part,
                                                         unsigned* __restrict__ counts, float* __restrict__ pix,
                                                         long pix_plane) {
  const int t = threadIdx.x;
  const int b = blockIdx.y;
  const long npix = (long)S * S;
  const float* L = logits + (long)b * h * w * N;
  double a[PIX_NQ] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  unsigned c6[PIX_NQ] = {0, 0, 0, 0, 0, 0};
  for (long i = (long)blockIdx.x * 256 + t; i < npix; i += (long)gridDim.x * 256) {
    const int Y = (int)(i / S), X = (int)(i - (long)Y * S);
    const PixelTaps tp = pixel_taps(lerp_coord_d(Y, h, S), lerp_coord_d(X, w, S), w, N);
    double m = tp.at(L);
    for (int c = 1; c < N; ++c) m = fmax(m, tp.at(L + c));
    double s = 0.0, so = 0.0;
    float ef = 0.f;
    for (int c = 0; c < N; ++c) {
      const float e = expf((float)(tp.at(L + c) - m));
      s += (double)e;
      if (c == idx_cls)
        ef = e;
      else
        so += (double)e;
    }
    const float p = (float)((double)ef / s), q0 = (float)(so / s);
    if (pix) {
      const long o = (long)b * npix + i;
      pix[o] = (float)(m + log(s));
      pix[pix_plane + o] = p;
      pix[2 * pix_plane + o] = q0;
    }
    const int64_t tg = target[(long)b * npix + i];
    if (tg != 255) count_pred(c6, p > q0 ? 1 : 0, tg);
    if (dice) {
      a[2] += (double)(q0 * q0);
      a[3] += (double)(p * p);
      if (tg == 0) {
        a[0] += (double)q0;
        a[4] += 1.0;
      } else if (tg == 1) {
        a[1] += (double)p;
        a[5] += 1.0;
      }
    } else if (tg == 0 || tg == 1) {
      // the probabilities as logits: nll = log(exp(q_0) + exp(q_1)) - q_y = log1p(exp(q_other - q_y))
      const float d = tg == 1 ? q0 - p : p - q0;
      a[(int)tg] += 1.0;
      a[2 + (int)tg] += (double)log1pf(expf(d));
    }
  }
  block_partials<PIX_NQ, PIX_NQ>(a, c6, (long)b * gridDim.x + blockIdx.x, part, counts);
}

// One workgroup per low-res pixel.  Per chunk of 256 hi-res pixels of its support: thread i forms
// pixel i's taps and coef = tap weight x (dL/dp) p; then the threads turn to (class, group) pairs --
// cs = the power of two >= N lanes over the classes, 256 / cs groups striding the chunk -- and
// accumulate coef ([c == idx_cls] - softmax_c); the groups are summed in order, and the workgroup
// writes d_f[pix][:].
__global__ __launch_bounds__(256) void shn_adjoint_kernel(const float* __restrict__ W,
                                                          const float* __restrict__ logits,
                                                          const int64_t* __restrict__ target, int N, int h, int w,
                                                          int C, int S, int idx_cls, int dice, int cs,
                                                          const float* __restrict__ sc, const float* __restrict__ pix,
                                                          long pix_plane, float* __restrict__ d_f) {
  __shared__ PixelTaps taps[256];
  __shared__ float coef[256], lse_s[256], q0_s[256];
  __shared__ double red[256];
  __shared__ float dl[64];
  const int t = threadIdx.x;
  const long plane = (long)h * w;
  const long gp = blockIdx.x;  // b * h * w + y * w + x
  const int b = (int)(gp / plane);
  const int pp = (int)(gp - (long)b * plane), y = pp / w, x = pp - y * w;
  const float* L = logits + (long)b * plane * N;
  const long npix = (long)S * S;
  const int64_t* tg_b = target + (long)b * npix;
  const float* px = pix + (long)b * npix;
  int Y0, Y1, X0, X1;
  support_range(y, (double)(S - 1) / (double)(h - 1), S, &Y0, &Y1);
  support_range(x, (double)(S - 1) / (double)(w - 1), S, &X0, &X1);
  const int nx = X1 - X0 + 1, n = (Y1 - Y0 + 1) * nx;
  const HeadCoef k4 = load_coef(sc, b, dice);
  const int c = t & (cs - 1), g = t / cs, G = 256 / cs;
  double acc = 0.0;
  for (int base = 0; base < n; base += 256) {
    const int i = base + t;
    float cf = 0.f;
    if (i < n) {
      const int Y = Y0 + i / nx, X = X0 + i % nx;
      const LerpD ly = lerp_coord_d(Y, h, S), lx = lerp_coord_d(X, w, S);
      const double wt = tap_weight(ly, y) * tap_weight(lx, x);
      if (wt != 0.0) {
        const long o = (long)Y * S + X;
        const float p = px[pix_plane + o], q0 = px[2 * pix_plane + o];
        const int64_t tg = tg_b[o];
        float dp = 0.f;  // dL/dp = dL/dq_1 - dL/dq_0
        if (dice) {
          dp = ((tg == 1 ? k4.s1 : 0.f) + k4.s3 * p) - ((tg == 0 ? k4.s0 : 0.f) + k4.s2 * q0);
        } else if (tg == 0 || tg == 1) {
          const float sg1 = 1.0f / (1.0f + expf(q0 - p));  // softmax2(q)_1
          dp = (tg == 1 ? k4.s0 * -2.0f * (1.0f - sg1) : 2.0f * sg1) * k4.s1;
        }
        cf = (float)wt * dp * p;
        taps[t] = pixel_taps(ly, lx, w, N);
        lse_s[t] = px[o];
        q0_s[t] = q0;
      }
    }
    coef[t] = cf;
    __syncthreads();
    const int cnt = min(256, n - base);
    if (c < N) {
      for (int k = g; k < cnt; k += G) {
        const float cfk = coef[k];
        if (cfk == 0.f) continue;
        // class idx_cls: 1 - softmax = the kept 1 - p, exact where p rounds to 1
        const float term = c == idx_cls ? q0_s[k] : -expf((float)(taps[k].at(L + c) - (double)lse_s[k]));
        acc += (double)(cfk * term);
      }
    }
    __syncthreads();
  }
  red[t] = acc;
  __syncthreads();
  if (t < N) {
    double v = 0.0;
    for (int k = 0; k < G; ++k) v += red[k * cs + t];
    dl[t] = (float)v;
  }
  __syncthreads();
  float* dst = d_f + gp * C;
  for (int ch = t; ch < C; ch += 256) {
    float v = 0.f;
    for (int k = 0; k < N; ++k) v = fmaf(W[(long)k * C + ch], dl[k], v);
    dst[ch] = v;
  }
}

// [B][h*w][N] -> [B][N][h*w]
__global__ __launch_bounds__(256) void shn_logits_out_kernel(const float* __restrict__ lg, long plane, int N,
                                                             long total, float* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;  // over the output
  if (i >= total) return;
  const long b = i / (plane * N), r = i - b * plane * N;
  const long c = r / plane, p = r - c * plane;
  out[i] = lg[(b * plane + p) * N + c];
}

int launch_seg_head_loss_nway(const float* W, const float* logits, int B, int N, int h, int w, int C,
                              const int64_t* target, int S, int idx_cls, int loss_type, float* loss_out,
                              float* logits_out, float* d_f, float* iut_out, void* part_ws, float* sc, float* pix,
                              hipStream_t st) {
  const long npix = (long)S * S;
  const int nblk = (int)std::min<long>(PIX_MAXBLK, cdiv(npix, 256));
  const int dice = loss_type == 1;
  double* part = (double*)part_ws;
  unsigned* counts = (unsigned*)(part + (size_t)B * PIX_MAXBLK * PIX_NQ);
  const long pix_plane = (long)B * npix;
  hipLaunchKernelGGL(shn_reduce_kernel, dim3(nblk, B), dim3(256), 0, st, logits, target, N, h, w, S, idx_cls, dice, part,
                     counts, d_f ? pix : (float*)nullptr, pix_plane);
  CWT_LAUNCH_CHECK();
  hipLaunchKernelGGL(head_final_kernel<true>, dim3(1), dim3(PIX_MAXBLK), 0, st, (const double*)part,
                     (const unsigned*)counts, nblk, B, loss_type, sc, loss_out, iut_out);
  CWT_LAUNCH_CHECK();
  if (d_f) {
    int cs = 2;
    while (cs < N) cs <<= 1;
    hipLaunchKernelGGL(shn_adjoint_kernel, dim3((unsigned)((long)B * h * w)), dim3(256), 0, st, W, logits, target, N, h,
                       w, C, S, idx_cls, dice, cs, (const float*)sc, (const float*)pix, pix_plane, d_f);
    CWT_LAUNCH_CHECK();
  }
  if (logits_out) {
    const long total = (long)B * N * h * w;
    hipLaunchKernelGGL(shn_logits_out_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, st, logits, (long)h * w, N,
                       total, logits_out);
    CWT_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace cwt
