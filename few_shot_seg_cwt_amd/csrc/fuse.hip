// The fusion trainer's kernels (reference src/train_fuse.py:121-229, FuseNet1 of
// src/model/transformer.py:286-330 over CenterPivotConv4d, src/model/conv4d.py:27-62).
//
// The 4-D stack.  x [B][NA][NB] is one correlation (query position a = (ya, xa), support position
// b = (yb, xb)); b' = (yb', xb') runs over the strided support plane mB x nB = ceil(hB/2) x ceil(wB/2).
//   pre1[o][a][b'] = b1a[o] + b1b[o] + sum_da w1a[o][da] x[a + da][2 b'] + sum_db w1b[o][db] x[a][2 b' + db]
//   y1 = relu(pre1)         (prune samples support rows 0, 2, 4, ...; the strided conv pads with one zero)
//   pre2[a][b']    = b2a + b2b + sum_o sum_da w2a[o][da] y1[o][a + da][b'] + sum_o sum_db w2b[o][db] y1[o][a][b' + db]
//   y2 = relu(pre2)         (da, db in {-1, 0, 1}^2, zero padding on both planes)
// A y2 needs y1 on a cross: the nine (a + da, b') and the nine (a, b' + db), the centre shared.  The
// fused forward recomputes layer 1 on those 17 positions per output in registers (plain fp32 FMA)
// and never stores y1; the training forward stores y1 [B][NA][NB2][16] once and layer 2 reads it.
// Both run the same two device functions in the same order, so they give the same bits.
//
// The backward carries no gradient to x (nothing upstream of the correlations trains).  Every term is
// keyed on a y1 position p = (a, b'): with G_da = g2[a - da][b'], H_db = g2[a][b' - db] (g2 = dy2 [y2 > 0]),
//   dw2a[o][da] += y1[o][p] G_da, dw2b[o][db] += y1[o][p] H_db, db2 += g2[p]
//   g1[o][p] = [y1 > 0] (sum_da w2a[o][da] G_da + sum_db w2b[o][db] H_db)
//   dw1a[o][da] += g1 x[a + da][2 b'], dw1b[o][db] += g1 x[a][2 b' + db], db1[o] += g1
// A workgroup is 16 channels x 16 positions; each thread keeps its channel's 38 sums over the
// workgroup's positions (a grid stride), the 16 position slots are added in slot order, one row of
// partials per workgroup, and a second kernel adds the rows: per thread in row order, then a 256-wide
// tree.  No float atomics; two calls give the same bits.
#include "fuse.h"
#include "pixel_pass.h"

namespace cwt {

// ---- the stack ----

struct FuseW {  // in LDS: the 16-channel weights of both layers and the summed biases
  float w1a[FUSE_C * 9], w1b[FUSE_C * 9], w2a[FUSE_C * 9], w2b[FUSE_C * 9], b1[FUSE_C], b2;
};
__device__ __forceinline__ void fuse_load_w(FuseW& s, const FuseParams& p) {
  for (int i = threadIdx.x; i < FUSE_C * 9; i += blockDim.x) {
    s.w1a[i] = p.w1a[i];
    s.w1b[i] = p.w1b[i];
    s.w2a[i] = p.w2a[i];
    s.w2b[i] = p.w2b[i];
  }
  if (threadIdx.x < FUSE_C) s.b1[threadIdx.x] = p.b1a[threadIdx.x] + p.b1b[threadIdx.x];
  if (threadIdx.x == 0) s.b2 = p.b2a[0] + p.b2b[0];
  __syncthreads();
}

struct FusePos {
  int b, ya, xa, yb, xb;
};
__device__ __forceinline__ FusePos fuse_pos(long u, const FuseGeom& g) {
  FusePos r;
  const long nb2 = (long)g.mB * g.nB;
  const long q = u / nb2;
  const int bp = (int)(u - q * nb2);
  r.yb = bp / g.nB;
  r.xb = bp - r.yb * g.nB;
  const long na = (long)g.hA * g.wA;
  r.b = (int)(q / na);
  const int a = (int)(q - (long)r.b * na);
  r.ya = a / g.wA;
  r.xa = a - r.ya * g.wA;
  return r;
}

// the 18 inputs of layer 1 at (ya, xa, yb', xb'): xq[k] = x[a + da][2 b'], xs[k] = x[a][2 b' + db]
__device__ __forceinline__ void fuse_l1_taps(const float* __restrict__ xb_, const FuseGeom& g, int ya, int xa, int yb,
                                             int xb, float (&xq)[9], float (&xs)[9]) {
  const long NB = (long)g.hB * g.wB;
  const int sb = 2 * yb * g.wB + 2 * xb;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int qy = ya + dy - 1, qx = xa + dx - 1;
      const bool okq = qy >= 0 && qy < g.hA && qx >= 0 && qx < g.wA;
      xq[dy * 3 + dx] = okq ? xb_[((long)qy * g.wA + qx) * NB + sb] : 0.f;
      const int sy = 2 * yb + dy - 1, sx = 2 * xb + dx - 1;
      const bool oks = sy >= 0 && sy < g.hB && sx >= 0 && sx < g.wB;
      xs[dy * 3 + dx] = oks ? xb_[((long)ya * g.wA + xa) * NB + (long)sy * g.wB + sx] : 0.f;
    }
}

__device__ __forceinline__ void fuse_l1(const float* __restrict__ xb_, const FuseGeom& g, int ya, int xa, int yb,
                                        int xb, const FuseW& s, float (&y)[FUSE_C]) {
  float xq[9], xs[9];
  fuse_l1_taps(xb_, g, ya, xa, yb, xb, xq, xs);
#pragma unroll
  for (int o = 0; o < FUSE_C; ++o) {
    float acc = s.b1[o];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc = fmaf(s.w1a[o * 9 + k], xq[k], acc);
#pragma unroll
    for (int k = 0; k < 9; ++k) acc = fmaf(s.w1b[o * 9 + k], xs[k], acc);
    y[o] = fmaxf(acc, 0.f);
  }
}

// one tap of layer 2: acc += sum_o w[o][k] y[o]
__device__ __forceinline__ float fuse_l2_tap(const float* w, int k, const float (&y)[FUSE_C], float acc) {
#pragma unroll
  for (int o = 0; o < FUSE_C; ++o) acc = fmaf(w[o * 9 + k], y[o], acc);
  return acc;
}

// Layer 2 at unit P over a y1 source: src(ya, xa, yb, xb, y) fills the 16 channels of an in-range position.
// Order: the nine query taps, then the nine support taps (the centre's y1 fetched once).
template <class Src>
__device__ __forceinline__ float fuse_l2(const FuseGeom& g, const FusePos& P, const FuseW& s, Src src) {
  float acc = s.b2;
  float yc[FUSE_C], y[FUSE_C];
  src(P.ya, P.xa, P.yb, P.xb, yc);
  for (int k = 0; k < 9; ++k) {
    const int qy = P.ya + k / 3 - 1, qx = P.xa + k % 3 - 1;
    if (k == 4) {
      acc = fuse_l2_tap(s.w2a, k, yc, acc);
    } else if (qy >= 0 && qy < g.hA && qx >= 0 && qx < g.wA) {
      src(qy, qx, P.yb, P.xb, y);
      acc = fuse_l2_tap(s.w2a, k, y, acc);
    }
  }
  for (int k = 0; k < 9; ++k) {
    const int sy = P.yb + k / 3 - 1, sx = P.xb + k % 3 - 1;
    if (k == 4) {
      acc = fuse_l2_tap(s.w2b, k, yc, acc);
    } else if (sy >= 0 && sy < g.mB && sx >= 0 && sx < g.nB) {
      src(P.ya, P.xa, sy, sx, y);
      acc = fuse_l2_tap(s.w2b, k, y, acc);
    }
  }
  return fmaxf(acc, 0.f);
}

__device__ __forceinline__ long fuse_x_index(const FuseGeom& g, const FusePos& P, long ldx, int col) {
  return ((long)P.b * g.hA * g.wA + (long)P.ya * g.wA + P.xa) * ldx + col + (long)P.yb * g.nB + P.xb;
}

__global__ __launch_bounds__(256) void fuse_stack_fused_kernel(const float* __restrict__ x, FuseGeom g, FuseParams p,
                                                               float* __restrict__ X, long ldx, int col) {
  __shared__ FuseW s;
  fuse_load_w(s, p);
  const long u = (long)blockIdx.x * 256 + threadIdx.x;
  if (u >= g.units()) return;
  const FusePos P = fuse_pos(u, g);
  const float* xb_ = x + (long)P.b * g.NA() * g.NB();
  X[fuse_x_index(g, P, ldx, col)] =
      fuse_l2(g, P, s, [&](int ya, int xa, int yb, int xb, float (&y)[FUSE_C]) { fuse_l1(xb_, g, ya, xa, yb, xb, s, y); });
}

__global__ __launch_bounds__(256) void fuse_stack_l1_kernel(const float* __restrict__ x, FuseGeom g, FuseParams p,
                                                            float* __restrict__ y1) {
  __shared__ FuseW s;
  fuse_load_w(s, p);
  const long u = (long)blockIdx.x * 256 + threadIdx.x;
  if (u >= g.units()) return;
  const FusePos P = fuse_pos(u, g);
  float y[FUSE_C];
  fuse_l1(x + (long)P.b * g.NA() * g.NB(), g, P.ya, P.xa, P.yb, P.xb, s, y);
  float4* dst = (float4*)(y1 + u * FUSE_C);
#pragma unroll
  for (int i = 0; i < FUSE_C / 4; ++i) dst[i] = make_float4(y[4 * i], y[4 * i + 1], y[4 * i + 2], y[4 * i + 3]);
}

__global__ __launch_bounds__(256) void fuse_stack_l2_kernel(const float* __restrict__ y1, FuseGeom g, FuseParams p,
                                                            float* __restrict__ X, long ldx, int col) {
  __shared__ FuseW s;
  fuse_load_w(s, p);
  const long u = (long)blockIdx.x * 256 + threadIdx.x;
  if (u >= g.units()) return;
  const FusePos P = fuse_pos(u, g);
  const float* yb_ = y1 + (long)P.b * g.NA() * g.NB2() * FUSE_C;
  X[fuse_x_index(g, P, ldx, col)] = fuse_l2(g, P, s, [&](int ya, int xa, int yb, int xb, float (&y)[FUSE_C]) {
    const float4* src = (const float4*)(yb_ + (((long)ya * g.wA + xa) * g.NB2() + (long)yb * g.nB + xb) * FUSE_C);
#pragma unroll
    for (int i = 0; i < FUSE_C / 4; ++i) {
      const float4 v = src[i];
      y[4 * i] = v.x;
      y[4 * i + 1] = v.y;
      y[4 * i + 2] = v.z;
      y[4 * i + 3] = v.w;
    }
  });
}

int launch_fuse_stack(const float* x, const FuseGeom& g, const FuseParams& p, float* y1, float* X, long ldx, int col,
                      hipStream_t st) {
  const unsigned nblk = (unsigned)cdiv(g.units(), 256);
  if (!y1) {
    hipLaunchKernelGGL(fuse_stack_fused_kernel, dim3(nblk), dim3(256), 0, st, x, g, p, X, ldx, col);
    CWT_LAUNCH_CHECK();
    return 0;
  }
  hipLaunchKernelGGL(fuse_stack_l1_kernel, dim3(nblk), dim3(256), 0, st, x, g, p, y1);
  CWT_LAUNCH_CHECK();
  hipLaunchKernelGGL(fuse_stack_l2_kernel, dim3(nblk), dim3(256), 0, st, (const float*)y1, g, p, X, ldx, col);
  CWT_LAUNCH_CHECK();
  return 0;
}

// ---- the stack's backward ----

int fuse_bwd_blocks(const FuseGeom& g) { return (int)std::min<long>(FUSE_MAXBLK, cdiv(g.units(), 16)); }
size_t fuse_bwd_part_doubles(const FuseGeom& g) { return (size_t)fuse_bwd_blocks(g) * FUSE_C * FUSE_NACC; }

// g2 at (a, b') of batch b: dX [y2 > 0]
__device__ __forceinline__ float fuse_g2(const float* __restrict__ X, const float* __restrict__ dX, const FuseGeom& g,
                                         int b, int ya, int xa, int yb, int xb, long ldx, int col) {
  const long i = ((long)b * g.hA * g.wA + (long)ya * g.wA + xa) * ldx + col + (long)yb * g.nB + xb;
  return X[i] > 0.f ? dX[i] : 0.f;
}

// acc: [0, 9) dw1a, [9, 18) dw1b, 18 db1, [19, 28) dw2a, [28, 37) dw2b, 37 db2 (channel 0's threads only)
__global__ __launch_bounds__(256) void fuse_stack_bwd_kernel(const float* __restrict__ x, FuseGeom g, FuseParams p,
                                                             const float* __restrict__ y1,
                                                             const float* __restrict__ X,
                                                             const float* __restrict__ dX, long ldx, int col,
                                                             double* __restrict__ part) {
  __shared__ float w2a[FUSE_C * 9], w2b[FUSE_C * 9];
  __shared__ double red[16][FUSE_C];
  const int t = threadIdx.x, o = t & 15, slot = t >> 4;
  if (t < FUSE_C * 9) {
    w2a[t] = p.w2a[t];
    w2b[t] = p.w2b[t];
  }
  __syncthreads();
  float acc[FUSE_NACC];
#pragma unroll
  for (int q = 0; q < FUSE_NACC; ++q) acc[q] = 0.f;
  const long n = g.units();
  for (long u = (long)blockIdx.x * 16 + slot; u < n; u += (long)gridDim.x * 16) {
    const FusePos P = fuse_pos(u, g);
    float G[9], H[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int qy = P.ya - (k / 3 - 1), qx = P.xa - (k % 3 - 1);
      G[k] = (qy >= 0 && qy < g.hA && qx >= 0 && qx < g.wA) ? fuse_g2(X, dX, g, P.b, qy, qx, P.yb, P.xb, ldx, col) : 0.f;
      const int sy = P.yb - (k / 3 - 1), sx = P.xb - (k % 3 - 1);
      H[k] = (sy >= 0 && sy < g.mB && sx >= 0 && sx < g.nB) ? fuse_g2(X, dX, g, P.b, P.ya, P.xa, sy, sx, ldx, col) : 0.f;
    }
    const float yv = y1[u * FUSE_C + o];
    float d = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      acc[19 + k] = fmaf(yv, G[k], acc[19 + k]);
      d = fmaf(w2a[o * 9 + k], G[k], d);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      acc[28 + k] = fmaf(yv, H[k], acc[28 + k]);
      d = fmaf(w2b[o * 9 + k], H[k], d);
    }
    if (o == 0) acc[37] += G[4];
    const float g1 = yv > 0.f ? d : 0.f;
    float xq[9], xs[9];
    fuse_l1_taps(x + (long)P.b * g.NA() * g.NB(), g, P.ya, P.xa, P.yb, P.xb, xq, xs);
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      acc[k] = fmaf(g1, xq[k], acc[k]);
      acc[9 + k] = fmaf(g1, xs[k], acc[9 + k]);
    }
    acc[18] += g1;
  }
#pragma unroll
  for (int q = 0; q < FUSE_NACC; ++q) {
    red[slot][o] = (double)acc[q];
    __syncthreads();
    if (slot == 0) {
      double sum = 0.0;
      for (int r = 0; r < 16; ++r) sum += red[r][o];
      part[((long)blockIdx.x * FUSE_C + o) * FUSE_NACC + q] = sum;
    }
    __syncthreads();
  }
}

// one workgroup per (channel, sum): the rows in order per thread, the 256-wide tree, the destination
__global__ __launch_bounds__(256) void fuse_stack_bwd_final_kernel(const double* __restrict__ part, int nblk,
                                                                   int accumulate, FuseGrads d) {
  __shared__ double red[256];
  const int t = threadIdx.x, o = blockIdx.x / FUSE_NACC, q = blockIdx.x - o * FUSE_NACC;
  double sum = 0.0;
  for (int r = t; r < nblk; r += 256) sum += part[((long)r * FUSE_C + o) * FUSE_NACC + q];
  red[t] = sum;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (t < k) red[t] += red[t + k];
    __syncthreads();
  }
  if (t != 0) return;
  const double v = red[0];
  float* dst[2] = {nullptr, nullptr};
  if (q < 9) {
    dst[0] = d.w1a + o * 9 + q;
  } else if (q < 18) {
    dst[0] = d.w1b + o * 9 + (q - 9);
  } else if (q == 18) {
    dst[0] = d.b1a + o;
    dst[1] = d.b1b + o;
  } else if (q < 28) {
    dst[0] = d.w2a + o * 9 + (q - 19);
  } else if (q < 37) {
    dst[0] = d.w2b + o * 9 + (q - 28);
  } else if (o == 0) {
    dst[0] = d.b2a;
    dst[1] = d.b2b;
  }
  for (int i = 0; i < 2; ++i)
    if (dst[i]) *dst[i] = (float)((accumulate ? (double)*dst[i] : 0.0) + v);
}

int launch_fuse_stack_bwd(const float* x, const FuseGeom& g, const FuseParams& p, const float* y1, const float* X,
                          const float* dX, long ldx, int col, int accumulate, const FuseGrads& d, double* part,
                          hipStream_t st) {
  const int nblk = fuse_bwd_blocks(g);
  hipLaunchKernelGGL(fuse_stack_bwd_kernel, dim3(nblk), dim3(256), 0, st, x, g, p, y1, X, dX, ldx, col, part);
  CWT_LAUNCH_CHECK();
  hipLaunchKernelGGL(fuse_stack_bwd_final_kernel, dim3(FUSE_C * FUSE_NACC), dim3(256), 0, st, (const double*)part, nblk,
                     accumulate, d);
  CWT_LAUNCH_CHECK();
  return 0;
}

// ---- the support mask (train_fuse.py:173-175, :319-321; transformer.py:318-319) ----

// upsample_bilinear2d's source coordinate in float64: align_corners dst (in - 1) / (out - 1), else
// max(0, (dst + 0.5) in / out - 0.5)
__device__ __forceinline__ LerpD fuse_mask_coord(int dst, int in_size, int out_size, int align) {
  double src;
  if (align)
    src = out_size > 1 ? (double)(in_size - 1) / (double)(out_size - 1) * (double)dst : 0.0;
  else
    src = fmax(0.0, ((double)dst + 0.5) * ((double)in_size / (double)out_size) - 0.5);
  LerpD r;
  r.i0 = min((int)src, in_size - 1);
  r.i1 = r.i0 + (r.i0 < in_size - 1 ? 1 : 0);
  r.l1 = src - (double)r.i0;
  r.l0 = 1.0 - r.l1;
  return r;
}
__device__ __forceinline__ double fuse_mask_label(const int64_t* __restrict__ label, long i) {
  const int64_t v = label[i];
  return v == 255 ? 0.0 : (double)v;
}
__device__ __forceinline__ double fuse_mask_at(const int64_t* __restrict__ label, int H, int W, int Y, int X, int oh,
                                               int ow, int align) {
  const LerpD ly = fuse_mask_coord(Y, H, oh, align), lx = fuse_mask_coord(X, W, ow, align);
  return ly.l0 * (lx.l0 * fuse_mask_label(label, (long)ly.i0 * W + lx.i0) +
                  lx.l1 * fuse_mask_label(label, (long)ly.i0 * W + lx.i1)) +
         ly.l1 * (lx.l0 * fuse_mask_label(label, (long)ly.i1 * W + lx.i0) +
                  lx.l1 * fuse_mask_label(label, (long)ly.i1 * W + lx.i1));
}
__global__ __launch_bounds__(256) void fuse_support_mask_kernel(const int64_t* __restrict__ label, int H, int W, int m,
                                                                int align, int pool, float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m * m) return;
  const int Y = i / m, X = i - Y * m;
  if (!pool) {
    out[i] = (float)fuse_mask_at(label, H, W, Y, X, m, m, align);
    return;
  }
  // the resize to [2m][2m] stored in fp32, as the reference holds it, then AvgPool2d(2, 2)
  const float a = (float)fuse_mask_at(label, H, W, 2 * Y, 2 * X, 2 * m, 2 * m, align);
  const float b = (float)fuse_mask_at(label, H, W, 2 * Y, 2 * X + 1, 2 * m, 2 * m, align);
  const float c = (float)fuse_mask_at(label, H, W, 2 * Y + 1, 2 * X, 2 * m, 2 * m, align);
  const float d = (float)fuse_mask_at(label, H, W, 2 * Y + 1, 2 * X + 1, 2 * m, 2 * m, align);
  out[i] = (float)((((double)a + (double)b) + ((double)c + (double)d)) * 0.25);
}
int launch_fuse_support_mask(const int64_t* label, int H, int W, int m, int align_corners, int pool, float* out,
                             hipStream_t st) {
  hipLaunchKernelGGL(fuse_support_mask_kernel, dim3(cdiv((long)m * m, 256)), dim3(256), 0, st, label, H, W, m,
                     align_corners, pool, out);
  CWT_LAUNCH_CHECK();
  return 0;
}

// ---- the broadcast mask folded into the bias: b_eff[j] = b[j] + sum_i W[j][col + i] s_mask[i] ----

__global__ __launch_bounds__(256) void fuse_mask_bias_kernel(const float* __restrict__ W, long ldw, int col,
                                                             const float* __restrict__ s_mask, int n,
                                                             const float* __restrict__ b, float* __restrict__ b_eff) {
  __shared__ double red[256];
  const int t = threadIdx.x, j = blockIdx.x;
  const float* row = W + (long)j * ldw + col;
  double sum = 0.0;
  for (int i = t; i < n; i += 256) sum += (double)row[i] * (double)s_mask[i];
  red[t] = sum;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (t < k) red[t] += red[t + k];
    __syncthreads();
  }
  if (t == 0) b_eff[j] = (float)((double)b[j] + red[0]);
}
int launch_fuse_mask_bias(const float* W, long ldw, int col, const float* s_mask, int n, const float* b, int mid,
                          float* b_eff, hipStream_t st) {
  hipLaunchKernelGGL(fuse_mask_bias_kernel, dim3(mid), dim3(256), 0, st, W, ldw, col, s_mask, n, b, b_eff);
  CWT_LAUNCH_CHECK();
  return 0;
}
// its weight gradient: d_W[j][col + i] = d_b[j] s_mask[i]
__global__ __launch_bounds__(256) void fuse_mask_bias_bwd_kernel(const float* __restrict__ d_b,
                                                                 const float* __restrict__ s_mask, int n,
                                                                 float* __restrict__ d_W, long ldw, int col) {
  const int j = blockIdx.x;
  const float g = d_b[j];
  for (int i = threadIdx.x; i < n; i += 256) d_W[(long)j * ldw + col + i] = g * s_mask[i];
}
int launch_fuse_mask_bias_bwd(const float* d_b, const float* s_mask, int mid, int n, float* d_W, long ldw, int col,
                              hipStream_t st) {
  hipLaunchKernelGGL(fuse_mask_bias_bwd_kernel, dim3(mid), dim3(256), 0, st, d_b, s_mask, n, d_W, ldw, col);
  CWT_LAUNCH_CHECK();
  return 0;
}

// ---- softmax over the two attention logits: z [B][P][2] tokens -> wt [B][2][P] planes ----

__global__ __launch_bounds__(256) void fuse_softmax2_kernel(const float* __restrict__ z, int B, long P,
                                                            float* __restrict__ wt) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * P) return;
  const long b = i / P, p = i - b * P;
  const float z0 = z[2 * i], z1 = z[2 * i + 1];
  wt[(2 * b) * P + p] = 1.0f / (1.0f + expf(z1 - z0));
  wt[(2 * b + 1) * P + p] = 1.0f / (1.0f + expf(z0 - z1));
}
// d_z0 = wt0 wt1 (d_wt0 - d_wt1) = -d_z1
__global__ __launch_bounds__(256) void fuse_softmax2_bwd_kernel(const float* __restrict__ wt,
                                                                const float* __restrict__ d_wt, int B, long P,
                                                                float* __restrict__ d_z) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * P) return;
  const long b = i / P, p = i - b * P;
  const long i0 = (2 * b) * P + p, i1 = i0 + P;
  const float d0 = wt[i0] * wt[i1] * (d_wt[i0] - d_wt[i1]);
  d_z[2 * i] = d0;
  d_z[2 * i + 1] = -d0;
}
int launch_fuse_softmax2(const float* z, int B, long P, float* wt, hipStream_t st) {
  hipLaunchKernelGGL(fuse_softmax2_kernel, dim3(cdiv((long)B * P, 256)), dim3(256), 0, st, z, B, P, wt);
  CWT_LAUNCH_CHECK();
  return 0;
}
int launch_fuse_softmax2_bwd(const float* wt, const float* d_wt, int B, long P, float* d_z, hipStream_t st) {
  hipLaunchKernelGGL(fuse_softmax2_bwd_kernel, dim3(cdiv((long)B * P, 256)), dim3(256), 0, st, wt, d_wt, B, P, d_z);
  CWT_LAUNCH_CHECK();
  return 0;
}

// ---- the blend on NHWC tokens: out[p][c] = wv[p][c] wt0[p] + fq[p][c] wt1[p] (train_fuse.py:178) ----

__global__ __launch_bounds__(256) void fuse_blend_kernel(const float* __restrict__ wv, const float* __restrict__ fq,
                                                         const float* __restrict__ wt, int B, long P, int C,
                                                         float* __restrict__ out) {
  const long n = (long)B * P * C;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long tok = i / C, b = tok / P, p = tok - b * P;
    out[i] = fmaf(fq[i], wt[(2 * b + 1) * P + p], wv[i] * wt[(2 * b) * P + p]);
  }
}
// one wave per token: d_wt0 = sum_c d_out wv, d_wt1 = sum_c d_out fq (lane-strided, then the wave's butterfly)
__global__ __launch_bounds__(256) void fuse_blend_bwd_kernel(const float* __restrict__ wv,
                                                             const float* __restrict__ fq,
                                                             const float* __restrict__ d_out, int B, long P, int C,
                                                             float* __restrict__ d_wt) {
  const int lane = threadIdx.x & 63;
  const long tok = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tok >= (long)B * P) return;
  const long b = tok / P, p = tok - b * P;
  float s0 = 0.f, s1 = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float d = d_out[tok * C + c];
    s0 = fmaf(d, wv[tok * C + c], s0);
    s1 = fmaf(d, fq[tok * C + c], s1);
  }
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  if (lane == 0) {
    d_wt[(2 * b) * P + p] = s0;
    d_wt[(2 * b + 1) * P + p] = s1;
  }
}
int launch_fuse_blend(const float* wv, const float* fq, const float* wt, int B, long P, int C, float* out,
                      hipStream_t st) {
  const int nblk = (int)std::min<long>(4096, cdiv((long)B * P * C, 256));
  hipLaunchKernelGGL(fuse_blend_kernel, dim3(nblk), dim3(256), 0, st, wv, fq, wt, B, P, C, out);
  CWT_LAUNCH_CHECK();
  return 0;
}
int launch_fuse_blend_bwd(const float* wv, const float* fq, const float* d_out, int B, long P, int C, float* d_wt,
                          hipStream_t st) {
  hipLaunchKernelGGL(fuse_blend_bwd_kernel, dim3(cdiv((long)B * P, 4)), dim3(256), 0, st, wv, fq, d_out, B, P, C, d_wt);
  CWT_LAUNCH_CHECK();
  return 0;
}

// ---- the loss head (train_fuse.py:182-186, :195-205) on pixel_pass.h's rules ----
// Per pixel of the S x S label, the three low-resolution logit pairs upsampled in float64:
//   m_i = 1 where argmax(pred_q0) != argmax(pred_q1) and the label is not 255, else 0.001 (ignored
//   pixels included: CrossEntropyLoss(reduction='none') gives them 0 and sum(wt_mask) counts them)
//   loss = sum ce_i m_i / sum m_i;   d pd_q = the bilinear adjoint of m_i (softmax - onehot) / sum m_i
// counts per block: 3 x {inter_0, inter_1, out_0, out_1, tgt_0, tgt_1} (pred_q, pred_q0, pred_q1), then
// the disagreeing pixels

constexpr int FUSE_LNC = 3 * PIX_NQ + 1;
size_t fuse_loss_part_doubles() { return (size_t)PIX_MAXBLK * 2; }
size_t fuse_loss_count_words() { return (size_t)PIX_MAXBLK * FUSE_LNC; }

struct FusePix {
  double z0, z1, m;
  int p, p0, p1;
};
__device__ __forceinline__ FusePix fuse_pixel(const float* __restrict__ q, const float* __restrict__ q0,
                                              const float* __restrict__ q1, int h, int w, int S, int Y, int X,
                                              int64_t tg) {
  const LerpD ly = lerp_coord_d(Y, h, S), lx = lerp_coord_d(X, w, S);
  const PixelTaps tp = pixel_taps(ly, lx, w, 1);
  const long plane = (long)h * w;
  FusePix r;
  r.z0 = tp.at(q);
  r.z1 = tp.at(q + plane);
  r.p = r.z1 > r.z0;  // a tie goes to class 0
  r.p0 = tp.at(q0 + plane) > tp.at(q0);
  r.p1 = tp.at(q1 + plane) > tp.at(q1);
  r.m = (r.p0 != r.p1 && tg != 255) ? 1.0 : 0.001;
  return r;
}

__global__ __launch_bounds__(256) void fuse_loss_reduce_kernel(const float* __restrict__ q, const float* __restrict__ q0,
                                                               const float* __restrict__ q1, int h, int w,
                                                               const int64_t* __restrict__ label, int S,
                                                               double* __restrict__ part, unsigned* __restrict__ counts) {
  double a[2] = {0.0, 0.0};
  unsigned c[FUSE_LNC];
#pragma unroll
  for (int k = 0; k < FUSE_LNC; ++k) c[k] = 0u;
  const long npix = (long)S * S;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < npix; i += (long)gridDim.x * 256) {
    const int Y = (int)(i / S), X = (int)(i - (long)Y * S);
    const int64_t tg = label[i];
    const FusePix r = fuse_pixel(q, q0, q1, h, w, S, Y, X, tg);
    a[1] += r.m;
    if (tg == 0 || tg == 1) {
      const double mx = fmax(r.z0, r.z1);
      const double lse = mx + log(exp(r.z0 - mx) + exp(r.z1 - mx));
      a[0] += (lse - (tg == 1 ? r.z1 : r.z0)) * r.m;
    }
    if (tg != 255) {
      unsigned(&c0)[PIX_NQ] = *(unsigned(*)[PIX_NQ])(c);
      unsigned(&c1)[PIX_NQ] = *(unsigned(*)[PIX_NQ])(c + PIX_NQ);
      unsigned(&c2)[PIX_NQ] = *(unsigned(*)[PIX_NQ])(c + 2 * PIX_NQ);
      count_pred(c0, r.p, tg);
      count_pred(c1, r.p0, tg);
      count_pred(c2, r.p1, tg);
      if (r.p0 != r.p1) c[3 * PIX_NQ]++;
    }
  }
  block_partials<2, FUSE_LNC>(a, c, blockIdx.x, part, counts);
}

__global__ __launch_bounds__(PIX_MAXBLK) void fuse_loss_final_kernel(const double* __restrict__ part,
                                                                    const unsigned* __restrict__ counts, int nblk,
                                                                    float* __restrict__ loss_out,
                                                                    float* __restrict__ iut_out,
                                                                    float* __restrict__ disagree_out,
                                                                    double* __restrict__ sc) {
  __shared__ double d[2][PIX_MAXBLK];
  __shared__ unsigned c[FUSE_LNC][PIX_MAXBLK];
  tree_partials<2, FUSE_LNC>(part, counts, nblk, d, c);
  const int t = threadIdx.x;
  if (t < 6) write_iut(iut_out + (t >> 1) * 6, c + (t >> 1) * PIX_NQ, t & 1);
  if (t == 0) {
    loss_out[0] = (float)(d[0][0] / d[1][0]);
    disagree_out[0] = (float)c[3 * PIX_NQ][0];
    sc[0] = 1.0 / d[1][0];  // sum m_i >= 0.001 S^2 > 0
  }
}

// one workgroup per low-resolution pixel: the hi-res pixels whose interpolation reads it, in a fixed order
__global__ __launch_bounds__(256) void fuse_loss_adjoint_kernel(const float* __restrict__ q, const float* __restrict__ q0,
                                                                const float* __restrict__ q1, int h, int w,
                                                                const int64_t* __restrict__ label, int S,
                                                                const double* __restrict__ sc,
                                                                float* __restrict__ d_pd_q) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  const int y = blockIdx.x / w, x = blockIdx.x - y * w;
  int Y0, Y1, X0, X1;
  support_range(y, (double)(S - 1) / (double)(h - 1), S, &Y0, &Y1);
  support_range(x, (double)(S - 1) / (double)(w - 1), S, &X0, &X1);
  const int nx = X1 - X0 + 1, n = (Y1 - Y0 + 1) * nx;
  double g1 = 0.0;
  for (int i = t; i < n; i += 256) {
    const int Y = Y0 + i / nx, X = X0 + i % nx;
    const int64_t tg = label[(long)Y * S + X];
    if (tg != 0 && tg != 1) continue;
    const LerpD ly = lerp_coord_d(Y, h, S), lx = lerp_coord_d(X, w, S);
    const double wgt = tap_weight(ly, y) * tap_weight(lx, x);
    if (wgt == 0.0) continue;
    const FusePix r = fuse_pixel(q, q0, q1, h, w, S, Y, X, tg);
    const double p1 = 1.0 / (1.0 + exp(r.z0 - r.z1));
    g1 += wgt * r.m * (p1 - (tg == 1 ? 1.0 : 0.0));
  }
  red[t] = g1;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (t < k) red[t] += red[t + k];
    __syncthreads();
  }
  if (t == 0) {
    const double v = red[0] * sc[0];
    d_pd_q[(long)h * w + blockIdx.x] = (float)v;
    d_pd_q[blockIdx.x] = (float)(-v);
  }
}

int launch_fuse_loss_head(const float* pd_q, const float* pd_q0, const float* pd_q1, int h, int w,
                          const int64_t* label, int S, float* loss_out, float* d_pd_q, float* iut_out,
                          float* disagree_out, double* part, unsigned* counts, double* sc, hipStream_t st) {
  const int nblk = (int)std::min<long>(PIX_MAXBLK, cdiv((long)S * S, 256));
  hipLaunchKernelGGL(fuse_loss_reduce_kernel, dim3(nblk), dim3(256), 0, st, pd_q, pd_q0, pd_q1, h, w, label, S, part,
                     counts);
  CWT_LAUNCH_CHECK();
  hipLaunchKernelGGL(fuse_loss_final_kernel, dim3(1), dim3(PIX_MAXBLK), 0, st, (const double*)part,
                     (const unsigned*)counts, nblk, loss_out, iut_out, disagree_out, sc);
  CWT_LAUNCH_CHECK();
  if (d_pd_q) {
    hipLaunchKernelGGL(fuse_loss_adjoint_kernel, dim3(h * w), dim3(256), 0, st, pd_q, pd_q0, pd_q1, h, w, label, S,
                       (const double*)sc, d_pd_q);
    CWT_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace cwt
