// The MMN / DeTr trainers' loss head (reference src/train_kshot.py:168-183): on the low-resolution
// classifier logits [B][2][h][w] (src/model/pspnet.py:183-187), the bilinear align_corners=True
// upsample to the S x S label, SegLoss (src/model/model_util.py:9-73: weighted_dice_loss,
// weighted_ce_loss, CrossEntropyLoss(ignore_index=255)) and the gradient carried back through the
// upsample and the classifier to the feature map f.
//
// Three launches on pixel_pass.h's pieces, the S x S logits never stored:
//  1. shl_reduce_kernel: per-block double partials of the six sums the loss needs
//       wt_dc: {I_0, I_1, sum p_0^2, sum p_1^2, sum t_0, sum t_1} per image, p_k = sigmoid(z_k)
//       ce:    {n_0, n_1, sum nll | y = 0, sum nll | y = 1, -, -} per image
//  2. head_final_kernel<false>: the loss and the per-(b, k) coefficients of the gradient
//       wt_dc: dz_k = p_k (1 - p_k) (a_k t_k + c_k p_k)
//       ce:    dz_1 = -dz_0 = w_y (softmax_1 - y) / sum_p w_y
//  3. shl_adjoint_kernel: the bilinear adjoint as a gather -- one workgroup per low-resolution
//     pixel sums, in a fixed order, the hi-resolution pixels whose interpolation reads it, then
//     writes d_f[p][c] = W[0][c] dlogit_0[p] + W[1][c] dlogit_1[p].
#include "kernels.h"
#include "pixel_pass.h"

namespace cwt {

size_t seg_head_loss_part_doubles(int B) { return (size_t)B * PIX_MAXBLK * PIX_NQ; }
size_t seg_head_loss_sc_floats(int B) { return (size_t)B * 4 + 4; }

__device__ __forceinline__ float sigmoidf(float z) { return 1.0f / (1.0f + expf(-z)); }

__global__ __launch_bounds__(256) void shl_reduce_kernel(const float* __restrict__ logits,
                                                         const int64_t* __restrict__ target, int h, int w, int S,
                                                         float sy, float sx, int dice, double* __restrict__ part) {
  const int t = threadIdx.x;
  const int b = blockIdx.y;
  const long npix = (long)S * S;
  const long plane = (long)h * w;
  const float* L0 = logits + (long)b * 2 * plane;
  const float* L1 = L0 + plane;
  double a[PIX_NQ] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
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
  block_partials<PIX_NQ, 0>(a, nullptr, (long)b * gridDim.x + blockIdx.x, part, nullptr);
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
  support_range(y, 1.0f / sy, S, &Y0, &Y1);
  support_range(x, 1.0f / sx, S, &X0, &X1);
  const int nx = X1 - X0 + 1, n = (Y1 - Y0 + 1) * nx;
  const HeadCoef k = load_coef(sc, b, dice);
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
      const float d0 = p0 * (1.f - p0) * ((tg == 0 ? k.s0 : 0.f) + k.s2 * p0);
      const float d1 = p1 * (1.f - p1) * ((tg == 1 ? k.s1 : 0.f) + k.s3 * p1);
      g0 = fmaf(wt, d0, g0);
      g1 = fmaf(wt, d1, g1);
    } else if (tg == 0 || tg == 1) {
      const float p1 = sigmoidf(z.z1 - z.z0);  // softmax over the two classes
      const float d1 = (tg == 1 ? k.s0 * (p1 - 1.f) : p1) * k.s1;
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
  const int nblk = (int)std::min<long>(PIX_MAXBLK, cdiv(npix, 256));
  const float sy = align_corners_scale(h, S), sx = align_corners_scale(w, S);
  const int dice = loss_type == 1;
  hipLaunchKernelGGL(shl_reduce_kernel, dim3(nblk, B), dim3(256), 0, st, logits, target, h, w, S, sy, sx, dice, part);
  CWT_LAUNCH_CHECK();
  hipLaunchKernelGGL(head_final_kernel<false>, dim3(1), dim3(PIX_MAXBLK), 0, st, (const double*)part,
                     (const unsigned*)nullptr, nblk, B, loss_type, sc, loss_out, (float*)nullptr);
  CWT_LAUNCH_CHECK();
  if (d_f) {
    hipLaunchKernelGGL(shl_adjoint_kernel, dim3((unsigned)((long)B * h * w)), dim3(256), 0, st, W, logits, target, h, w,
                       C, S, sy, sx, dice, (const float*)sc, d_f);
    CWT_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace cwt
