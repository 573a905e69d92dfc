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
// Four launches, every float sum in a fixed order (no float atomics), the S x S x N logits never
// stored; the reduce pass keeps (lse, p, 1 - p) per hi-res pixel in the workspace (3 floats a pixel)
// so that the adjoint's gather does not redo an N-way log-sum-exp for each low-res pixel that a
// hi-res pixel feeds:
//  1. shn_reduce_kernel: one thread per hi-res pixel; the interpolation and the softmax's max run in
//     float64 on the fp32 logits (as nway_pixel.hip), 1 - p is the other classes' share of the
//     exponential sum (no cancellation where p rounds to 1); per-block double partials of
//       wt_dc: {I_0, I_1, sum q_0^2, sum q_1^2, sum t_0, sum t_1} per image
//       ce:    {n_0, n_1, sum nll | y = 0, sum nll | y = 1, -, -} per image
//     and integer counts of the mask p > 1 - p against the target (train_cca.py:211-213: argmax of
//     the compressed prediction, a tie goes to class 0, 255 ignored).
//  2. shn_final_kernel: the partials summed by a fixed LDS tree, the loss, iut, and the coefficients
//       wt_dc: dL/dq_k = a_k t_k + c_k q_k, a_k = -2 / (max(D_k, 1e-8) B), c_k = 4 I_k / (D_k^2 B)
//              where D_k >= 1e-8 (the clamp passes no gradient below it)
//       ce:    dL/dq_k = w_y (softmax2(q)_k - [k == y]) / sum_p w_y
//  3. shn_adjoint_kernel: dL/dp = dL/dq_1 - dL/dq_0, dz_c = (dL/dp) p ([c == idx_cls] - softmax_c);
//     the bilinear adjoint as a gather -- one workgroup per low-res pixel over the hi-res pixels
//     whose interpolation reads it, lanes over the classes -- then
//     d_f[pix][:] = sum_c W[c][:] dlogit_c[pix] in plain fp32 FMAs (N x C per pixel: small).
//  4. shn_logits_out_kernel (when logits_out is given): the pixel-major logits copied to [B][N][h][w].
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace cwt {

constexpr int SHN_MAXBLK = 256;  // hi-res blocks per image (the final tree's width)
constexpr int SHN_NQ = 6;        // partial sums / counts per image

size_t seg_head_loss_nway_part_bytes(int B) {
  return (size_t)B * SHN_MAXBLK * SHN_NQ * (sizeof(double) + sizeof(unsigned));
}
size_t seg_head_loss_nway_sc_floats(int B) { return (size_t)B * 4 + 4; }
size_t seg_head_loss_nway_pix_floats(int B, int S) { return (size_t)3 * B * S * S; }

struct LerpN {
  int i0, i1;
  double l0, l1;
};
// upsample_bilinear2d(align_corners=True) in float64: src = dst (in - 1) / (out - 1)
__device__ __forceinline__ LerpN shn_lerp(int dst, int in_size, int out_size) {
  LerpN r;
  const double src = (double)(in_size - 1) / (double)(out_size - 1) * (double)dst;
  r.i0 = min((int)src, in_size - 1);
  r.i1 = r.i0 + (r.i0 < in_size - 1 ? 1 : 0);
  r.l1 = src - (double)r.i0;
  r.l0 = 1.0 - r.l1;
  return r;
}

// the four taps of one hi-res pixel: offsets in floats into an image's [h*w][N] logits
struct TapsN {
  int o00, o01, o10, o11;
  double ly0, ly1, lx0, lx1;
  __device__ __forceinline__ double at(const float* __restrict__ L) const {
    return ly0 * (lx0 * (double)L[o00] + lx1 * (double)L[o01]) + ly1 * (lx0 * (double)L[o10] + lx1 * (double)L[o11]);
  }
};
__device__ __forceinline__ TapsN shn_taps(const LerpN& ly, const LerpN& lx, int w, int N) {
  return TapsN{(ly.i0 * w + lx.i0) * N, (ly.i0 * w + lx.i1) * N, (ly.i1 * w + lx.i0) * N, (ly.i1 * w + lx.i1) * N,
               ly.l0, ly.l1, lx.l0, lx.l1};
}

// pix: [3][B * S * S] planes {lse, p, 1 - p}, or NULL (no gradient asked for)
__global__ __launch_bounds__(256) void shn_reduce_kernel(const float* __restrict__ logits,
                                                         const int64_t* __restrict__ target, int N, int h, int w,
                                                         int S, int idx_cls, int dice, double* __restrict__ part,
                                                         unsigned* __restrict__ counts, float* __restrict__ pix,
                                                         long pix_plane) {
  __shared__ double red[4][SHN_NQ];
  __shared__ unsigned cred[4][SHN_NQ];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int b = blockIdx.y;
  const long npix = (long)S * S;
  const float* L = logits + (long)b * h * w * N;
  double a[SHN_NQ] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  unsigned c6[SHN_NQ] = {0, 0, 0, 0, 0, 0};  // inter_0, inter_1, out_0, out_1, tgt_0, tgt_1
  for (long i = (long)blockIdx.x * 256 + t; i < npix; i += (long)gridDim.x * 256) {
    const int Y = (int)(i / S), X = (int)(i - (long)Y * S);
    const TapsN tp = shn_taps(shn_lerp(Y, h, S), shn_lerp(X, w, S), w, N);
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
    if (tg != 255) {
      const int pred = p > q0 ? 1 : 0;
      c6[2 + pred]++;
      if (tg == 0 || tg == 1) {
        c6[4 + (int)tg]++;
        if (pred == (int)tg) c6[pred]++;
      }
    }
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
#pragma unroll
  for (int q = 0; q < SHN_NQ; ++q) {
    for (int o = 32; o > 0; o >>= 1) {
      a[q] += __shfl_xor(a[q], o, 64);
      c6[q] += __shfl_xor(c6[q], o, 64);
    }
    if (lane == 0) {
      red[wv][q] = a[q];
      cred[wv][q] = c6[q];
    }
  }
  __syncthreads();
  if (t < SHN_NQ) {
    const long pb = ((long)b * gridDim.x + blockIdx.x) * SHN_NQ + t;
    part[pb] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
    counts[pb] = cred[0][t] + cred[1][t] + cred[2][t] + cred[3][t];
  }
}

// one 256-thread workgroup: thread k takes block k's partials, a fixed-shape LDS tree per image.
// sc[b][0..3]: wt_dc {a_0, a_1, c_0, c_1}; ce: sc[0] = w_fg, sc[1] = 1 / sum_p w_y (all images)
__global__ __launch_bounds__(256) void shn_final_kernel(const double* __restrict__ part,
                                                        const unsigned* __restrict__ counts, int nblk, int B,
                                                        int loss_type, float* __restrict__ sc,
                                                        float* __restrict__ loss_out, float* __restrict__ iut) {
  __shared__ double d[SHN_NQ][256];
  __shared__ unsigned cn[SHN_NQ][256];
  __shared__ double tot[8][SHN_NQ];
  const int t = threadIdx.x;
  for (int b = 0; b < B; ++b) {
#pragma unroll
    for (int q = 0; q < SHN_NQ; ++q) {
      d[q][t] = t < nblk ? part[((long)b * nblk + t) * SHN_NQ + q] : 0.0;
      cn[q][t] = t < nblk ? counts[((long)b * nblk + t) * SHN_NQ + q] : 0u;
    }
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (t < o) {
#pragma unroll
        for (int q = 0; q < SHN_NQ; ++q) {
          d[q][t] += d[q][t + o];
          cn[q][t] += cn[q][t + o];
        }
      }
      __syncthreads();
    }
    if (t < SHN_NQ) tot[b][t] = d[t][0];
    if (iut && t < 2) {
      iut[b * 6 + t] = (float)cn[t][0];
      iut[b * 6 + 2 + t] = (float)(cn[2 + t][0] + cn[4 + t][0] - cn[t][0]);  // union = output + target - intersection
      iut[b * 6 + 4 + t] = (float)cn[4 + t][0];
    }
    __syncthreads();
  }
  if (t != 0) return;
  if (loss_type == 1) {  // weighted_dice_loss (model_util.py:40-73) on probabilities, reduction 'sum' / n
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

// weight of low-res index i in the interpolation of a hi-res coordinate (both taps may hit it: at
// the far edge i0 == i1)
__device__ __forceinline__ double shn_tap_weight(const LerpN& l, int i) {
  return (l.i0 == i ? l.l0 : 0.0) + (l.i1 == i ? l.l1 : 0.0);
}

// hi-res index range [lo, hi] that can read low-res index i: src = dst (in - 1) / (S - 1) in
// (i - 1, i + 1), widened by one on each side (the exact membership is shn_tap_weight's)
__device__ __forceinline__ void shn_support_range(int i, int in_size, int S, int* lo, int* hi) {
  const double inv = (double)(S - 1) / (double)(in_size - 1);
  *lo = max(0, (int)floor((double)(i - 1) * inv) - 1);
  *hi = min(S - 1, (int)ceil((double)(i + 1) * inv) + 1);
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
  __shared__ TapsN taps[256];
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
  shn_support_range(y, h, S, &Y0, &Y1);
  shn_support_range(x, w, S, &X0, &X1);
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
  const int c = t & (cs - 1), g = t / cs, G = 256 / cs;
  double acc = 0.0;
  for (int base = 0; base < n; base += 256) {
    const int i = base + t;
    float cf = 0.f;
    if (i < n) {
      const int Y = Y0 + i / nx, X = X0 + i % nx;
      const LerpN ly = shn_lerp(Y, h, S), lx = shn_lerp(X, w, S);
      const double wt = shn_tap_weight(ly, y) * shn_tap_weight(lx, x);
      if (wt != 0.0) {
        const long o = (long)Y * S + X;
        const float p = px[pix_plane + o], q0 = px[2 * pix_plane + o];
        const int64_t tg = tg_b[o];
        float dp = 0.f;  // dL/dp = dL/dq_1 - dL/dq_0
        if (dice) {
          dp = ((tg == 1 ? s1 : 0.f) + s3 * p) - ((tg == 0 ? s0 : 0.f) + s2 * q0);
        } else if (tg == 0 || tg == 1) {
          const float sg1 = 1.0f / (1.0f + expf(q0 - p));  // softmax2(q)_1
          dp = (tg == 1 ? s0 * -2.0f * (1.0f - sg1) : 2.0f * sg1) * s1;
        }
        cf = (float)wt * dp * p;
        taps[t] = shn_taps(ly, lx, w, N);
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
  const int nblk = (int)std::min<long>(SHN_MAXBLK, cdiv(npix, 256));
  const int dice = loss_type == 1;
  double* part = (double*)part_ws;
  unsigned* counts = (unsigned*)(part + (size_t)B * SHN_MAXBLK * SHN_NQ);
  const long pix_plane = (long)B * npix;
  hipLaunchKernelGGL(shn_reduce_kernel, dim3(nblk, B), dim3(256), 0, st, logits, target, N, h, w, S, idx_cls, dice, part,
                     counts, d_f ? pix : (float*)nullptr, pix_plane);
  CWT_LAUNCH_CHECK();
  hipLaunchKernelGGL(shn_final_kernel, dim3(1), dim3(256), 0, st, (const double*)part, (const unsigned*)counts, nblk, B,
                     loss_type, sc, loss_out, iut_out);
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
