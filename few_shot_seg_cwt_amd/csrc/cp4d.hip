// The CenterPivotConv4d consensus layer of MatchNet / MMN (reference src/model/conv4d.py:11-62,
// src/model/match.py:55-86): every kernel form of its forward, input gradient and weight gradient,
// and their launchers.  Which form a shape takes, with which template arguments and grid, is
// decided in cp4d_plan.h alone (cp4d_plan_fwd / _dgrad / _wgrad); a launcher here takes that plan
// and instantiates the kernel it names.  Layout and arithmetic as match.hip describes them:
// channels-last x[B][a][b][C], exact fp32.
#include <algorithm>

#include "../../include/cwt.h"
#include "common.h"
#include "kernels.h"

namespace cwt {

// ---- one CenterPivotConv4d layer (+ ReLU) on x[B][NA][NB][CIN] -> y[B][NA][NB][COUT] ----
// y[a][b][o] = relu( sum_{c,ky,kx} Wa[o][c][ky][kx] x[(ha+ky-1, wa+kx-1)][b][c] + ba[o]
//                  + sum_{c,ky,kx} Wb[o][c][ky][kx] x[a][(hb+ky-1, wb+kx-1)][c] + bb[o] )
// (zero padding).  Workgroup tile: an a patch of TAH x TAW positions by a b patch of TBH x TBW;
// its cross-shaped input (a patch + halo at the tile's b positions, b patch + halo at its a
// positions) is staged in LDS; thread = one (a, b) pair, all COUT outputs.
constexpr int CP_NA = CP_TAH * CP_TAW, CP_NB = CP_TBH * CP_TBW;             // 16 x 16 = 256 pairs
constexpr int CP_HA = (CP_TAH + 2) * (CP_TAW + 2), CP_HB = (CP_TBH + 2) * (CP_TBW + 2);  // 40 halo positions
// MODE 1 (backward, match_bwd.hip): the input gradient of a layer -- the same cross-shaped
// convolution of the output gradient with each filter transposed (in / out channels exchanged)
// and flipped (tap 8 - t), no bias, no ReLU; accum adds into y (the symmetric branches' sum).
template <int CIN, int COUT, int MODE>
__global__ __launch_bounds__(256) void cp4d_layer_kernel(const float* __restrict__ x, int hA, int wA, int hB, int wB,
                                                         const float* __restrict__ Wa, const float* __restrict__ ba,
                                                         const float* __restrict__ Wb, const float* __restrict__ bb,
                                                         float* __restrict__ y, int accum) {
  // a halo box x b tile, one float of padding per a-halo position (the wave's two a rows of a
  // 32-lane group then fall on disjoint banks); b halo box at the tile's a positions
  __shared__ float xa[CP_HA][CP_NB * CIN + 1];
  __shared__ float xb[CP_NA][CP_HB][CIN];
  // weights tap-major with the outputs innermost ([side][tap][c][o], o padded to a multiple of
  // 4): one broadcast ds_read_b128 gives four outputs' weights for an input value
  constexpr int CO4 = (COUT + 3) & ~3;
  __shared__ __attribute__((aligned(16))) float wl[2][9][CIN][CO4];
  const int NA = hA * wA, NB = hB * wB;
  const int ntb = (wB + CP_TBW - 1) / CP_TBW;
  const int ta = blockIdx.y, tb = blockIdx.x;  // a tile, b tile
  const int ntaw = (wA + CP_TAW - 1) / CP_TAW;
  const int ha0 = (ta / ntaw) * CP_TAH, wa0 = (ta % ntaw) * CP_TAW;
  const int hb0 = (tb / ntb) * CP_TBH, wb0 = (tb % ntb) * CP_TBW;
  const long xoff = (long)blockIdx.z * NA * NB * CIN;
  const int t = threadIdx.x;
  for (int i = threadIdx.x; i < 2 * 9 * CIN * CO4; i += 256) {
    const int o = i % CO4, r = i / CO4;
    const int c = r % CIN, r2 = r / CIN;
    const int tap = r2 % 9, side = r2 / 9;
    const float* W = side ? Wb : Wa;
    (&wl[0][0][0][0])[i] = o >= COUT ? 0.f : MODE == 0 ? W[(o * CIN + c) * 9 + tap] : W[(c * COUT + o) * 9 + 8 - tap];
  }
  // both boxes: every load of the thread issued before the first LDS store (one round of
  // memory latency per workgroup instead of one per element)
  constexpr int EA = CP_HA * CP_NB * CIN, EB = CP_NA * CP_HB * CIN;
  constexpr int IA = (EA + 255) / 256, IB = (EB + 255) / 256;
  float ra[IA], rb[IB];
#pragma unroll
  for (int k = 0; k < IA; ++k) {  // a halo box at the tile's b positions
    const int i = t + 256 * k;
    const int c = i % CIN, p = i / CIN;
    const int bi = p % CP_NB, ai = p / CP_NB;
    const int ha = ha0 - 1 + ai / (CP_TAW + 2), wa = wa0 - 1 + ai % (CP_TAW + 2);
    const int hb = hb0 + bi / CP_TBW, wb = wb0 + bi % CP_TBW;
    const bool in = i < EA && (unsigned)ha < (unsigned)hA && (unsigned)wa < (unsigned)wA && hb < hB && wb < wB;
    ra[k] = in ? x[xoff + (((long)(ha * wA + wa) * NB) + hb * wB + wb) * CIN + c] : 0.f;
  }
#pragma unroll
  for (int k = 0; k < IB; ++k) {  // b halo box at the tile's a positions
    const int i = t + 256 * k;
    const int c = i % CIN, p = i / CIN;
    const int bi = p % CP_HB, ai = p / CP_HB;
    const int ha = ha0 + ai / CP_TAW, wa = wa0 + ai % CP_TAW;
    const int hb = hb0 - 1 + bi / (CP_TBW + 2), wb = wb0 - 1 + bi % (CP_TBW + 2);
    const bool in = i < EB && ha < hA && wa < wA && (unsigned)hb < (unsigned)hB && (unsigned)wb < (unsigned)wB;
    rb[k] = in ? x[xoff + (((long)(ha * wA + wa) * NB) + hb * wB + wb) * CIN + c] : 0.f;
  }
#pragma unroll
  for (int k = 0; k < IA; ++k) {
    const int i = t + 256 * k;
    if (i < EA) {
      const int c = i % CIN, p = i / CIN;
      xa[p / CP_NB][(p % CP_NB) * CIN + c] = ra[k];
    }
  }
#pragma unroll
  for (int k = 0; k < IB; ++k) {
    const int i = t + 256 * k;
    if (i < EB) (&xb[0][0][0])[i] = rb[k];
  }
  __syncthreads();
  const int ai = t / CP_NB, bi = t % CP_NB;  // this thread's pair within the tile
  const int ha = ha0 + ai / CP_TAW, wa = wa0 + ai % CP_TAW;
  const int hb = hb0 + bi / CP_TBW, wb = wb0 + bi % CP_TBW;
  float acc[COUT];
#pragma unroll
  for (int o = 0; o < COUT; ++o) acc[o] = MODE == 0 ? ba[o] + bb[o] : 0.f;
  const int aiy = ai / CP_TAW, aix = ai % CP_TAW, biy = bi / CP_TBW, bix = bi % CP_TBW;
#pragma unroll 1
  for (int tap = 0; tap < 9; ++tap) {  // one tap's inputs and weights live at a time
      const int ky = tap / 3, kx = tap - 3 * (tap / 3);
      const float* pa = &xa[(aiy + ky) * (CP_TAW + 2) + aix + kx][bi * CIN];
      const float* pb = xb[ai][(biy + ky) * (CP_TBW + 2) + bix + kx];
      float va[CIN], vb[CIN];
#pragma unroll
      for (int c = 0; c < CIN; ++c) {
        va[c] = pa[c];
        vb[c] = pb[c];
      }
#pragma unroll
      for (int c = 0; c < CIN; ++c) {
        const float* w0 = wl[0][tap][c];
        const float* w1 = wl[1][tap][c];
#pragma unroll
        for (int o4 = 0; o4 < CO4; o4 += 4) {
          const f32x4 a4 = *(const f32x4*)(w0 + o4), b4 = *(const f32x4*)(w1 + o4);
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (o4 + q < COUT) {
              acc[o4 + q] = fmaf(a4[q], va[c], acc[o4 + q]);
              acc[o4 + q] = fmaf(b4[q], vb[c], acc[o4 + q]);
            }
        }
        if (c & 1) __builtin_amdgcn_sched_barrier(0);  // bounds the weight reads in flight (registers)
      }
    }
  if (ha < hA && wa < wA && hb < hB && wb < wB) {
    float* yp = y + (long)blockIdx.z * NA * NB * COUT + ((long)(ha * wA + wa) * NB + hb * wB + wb) * COUT;
#pragma unroll
    for (int o = 0; o < COUT; ++o) yp[o] = MODE == 0 ? fmaxf(acc[o], 0.f) : accum ? yp[o] + acc[o] : acc[o];
  }
}

// ---- the same layer on the f32 matrix cores (COUT = 10) and a register-blocked VALU form for
// COUT = 1 (round 4; the scalar kernel above measured 16 % of the fp32 VALU peak at 60^2: bound
// by its broadcast LDS weight reads, one per two FMAs, and by 4-B staging loads) ----
// Tile: a 4 x 4 patch of a positions by a 4 x 4 patch of b positions (256 pairs); staged in LDS
// as the a halo box (6 x 6) at the tile's 16 b positions and the tile's 16 a positions at the b
// halo box, CIN floats per position (dense; 2 floats of padding at the end).
constexpr int CM_H = CM_T + 2, CM_NH = CM_H * CM_H, CM_NT = CM_T * CM_T;  // 6 x 6 halo, 16 tile
template <int CIN>
struct CmLds {
  static constexpr int EA = CM_NH * CM_NT * CIN, EB = CM_NT * CM_NH * CIN;  // floats
};

// xa[ah][bt][c]: a halo position ah (6 x 6 around the a tile), tile b position bt; xb[at][bh][c]:
// tile a position at, b halo position bh.  CIN even: 8-B loads (a position is CIN / 2 of them,
// 8-B aligned); every load of the thread is issued before the first LDS store; positions off the
// map read 0.
template <int CIN>
__device__ __forceinline__ void cm_stage(const float* __restrict__ x, int hA, int wA, int hB, int wB, int ha0, int wa0,
                                         int hb0, int wb0, long xoff, float* xa, float* xb) {
  const int NB = hB * wB;
  constexpr int V = (CIN % 2 == 0) ? 2 : 1;  // floats per load
  constexpr int VP = CIN / V;                // loads per position
  constexpr int LA = CM_NH * CM_NT * VP, LB = CM_NT * CM_NH * VP;
  constexpr int IA = (LA + 255) / 256, IB = (LB + 255) / 256;
  typedef float vec_t __attribute__((ext_vector_type(V)));
  const int t = threadIdx.x;
  vec_t ra[IA], rb[IB];
#pragma unroll
  for (int k = 0; k < IA; ++k) {
    const int i = t + 256 * k;
    const int q = i % VP, p = i / VP;
    const int bt = p % CM_NT, ah = p / CM_NT;
    const int ha = ha0 - 1 + ah / CM_H, wa = wa0 - 1 + ah % CM_H;
    const int hb = hb0 + bt / CM_T, wb = wb0 + bt % CM_T;
    const bool in = i < LA && (unsigned)ha < (unsigned)hA && (unsigned)wa < (unsigned)wA && hb < hB && wb < wB;
    ra[k] = in ? *(const vec_t*)(x + xoff + (((long)(ha * wA + wa) * NB) + hb * wB + wb) * CIN + q * V) : vec_t(0.f);
  }
#pragma unroll
  for (int k = 0; k < IB; ++k) {
    const int i = t + 256 * k;
    const int q = i % VP, p = i / VP;
    const int bh = p % CM_NH, at = p / CM_NH;
    const int ha = ha0 + at / CM_T, wa = wa0 + at % CM_T;
    const int hb = hb0 - 1 + bh / CM_H, wb = wb0 - 1 + bh % CM_H;
    const bool in = i < LB && ha < hA && wa < wA && (unsigned)hb < (unsigned)hB && (unsigned)wb < (unsigned)wB;
    rb[k] = in ? *(const vec_t*)(x + xoff + (((long)(ha * wA + wa) * NB) + hb * wB + wb) * CIN + q * V) : vec_t(0.f);
  }
#pragma unroll
  for (int k = 0; k < IA; ++k) {
    const int i = t + 256 * k;
    if (i < LA) *(vec_t*)(xa + i * V) = ra[k];
  }
#pragma unroll
  for (int k = 0; k < IB; ++k) {
    const int i = t + 256 * k;
    if (i < LB) *(vec_t*)(xb + i * V) = rb[k];
  }
}

// COUT = 10 on v_mfma_f32_16x16x4_f32 (fp32 products, fp32 sums: an fmaf chain per output).
// Output rows of one MFMA group: the 16 tile b positions of ONE tile a position (group G = the a
// position); columns: the 10 output channels (16 wide, 6 unused).  K = (tap, channel) dense,
// 9 CIN rows padded to a multiple of 4 (zero weights): MFMA m, lane group g = lane / 16 takes
// k = 4 m + g, read at the lane's per-k LDS offset.  Both 2-D convolutions (a plane, b plane)
// accumulate into the same accumulators.  4 waves x 4 groups = the tile's 256 pairs.
// MODE 1: the input gradient of a layer with 10 input channels (the backward, launch_cp4d_dgrad):
// transposed, flipped filters (W[(c COUT + o) 9 + 8 - tap]), no bias, no ReLU, y accumulated when
// accum != 0.
template <int CIN, int MODE = 0>
__global__ __launch_bounds__(256) void cp4d_mfma_kernel(const float* __restrict__ x, int hA, int wA, int hB, int wB,
                                                        const float* __restrict__ Wa, const float* __restrict__ ba,
                                                        const float* __restrict__ Wb, const float* __restrict__ bb,
                                                        float* __restrict__ y, int accum = 0) {
  constexpr int COUT = 10;
  constexpr int KT = 9 * CIN;        // K rows per branch
  constexpr int NM = (KT + 3) / 4;   // MFMAs per branch and group
  __shared__ __attribute__((aligned(16))) float xa[CmLds<CIN>::EA + 2];
  __shared__ __attribute__((aligned(16))) float xb[CmLds<CIN>::EB + 2];
  const int NA = hA * wA, NB = hB * wB;
  const int ntb = (wB + CM_T - 1) / CM_T, nta = (wA + CM_T - 1) / CM_T;
  const int ta = blockIdx.y, tb = blockIdx.x;
  const int ha0 = (ta / nta) * CM_T, wa0 = (ta % nta) * CM_T;
  const int hb0 = (tb / ntb) * CM_T, wb0 = (tb % ntb) * CM_T;
  const long xoff = (long)blockIdx.z * NA * NB * CIN;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int r = lane & 15, g4 = lane >> 4;
  cm_stage<CIN>(x, hA, wA, hB, wB, ha0, wa0, hb0, wb0, xoff, xa, xb);
  // this lane's weights (B operand: column r = output channel, k = 4 m + g4) and the LDS offsets
  // of its k's (tap, channel) in the two staged boxes
  float wra[NM], wrb[NM];
  int offa[NM], offb[NM];
#pragma unroll
  for (int m = 0; m < NM; ++m) {
    const int k = 4 * m + g4;
    const bool kin = k < KT;
    const int tap = kin ? k / CIN : 0, c = kin ? k % CIN : 0;
    const int ky = tap / 3, kx = tap - 3 * (tap / 3);
    const bool live = kin && r < COUT;
    const int wi = MODE == 0 ? (r * CIN + c) * 9 + tap : (c * COUT + r) * 9 + 8 - tap;
    wra[m] = live ? Wa[wi] : 0.f;
    wrb[m] = live ? Wb[wi] : 0.f;
    offa[m] = (ky * CM_H + kx) * CM_NT * CIN + c;
    offb[m] = (ky * CM_H + kx) * CIN + c;
  }
  // row r of group G: a tile position G (ay, ax), b tile position r (by, bx)
  const int by = r / CM_T, bx = r % CM_T;
  const int base_b = (by * CM_H + bx) * CIN;
  __syncthreads();
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int m = 0; m < NM; ++m) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int G = wv * 4 + j, ay = G / CM_T, ax = G % CM_T;
      const float va = xa[((ay * CM_H + ax) * CM_NT + r) * CIN + offa[m]];
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(va, wra[m], acc[j], 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int G = wv * 4 + j;
      const float vb = xb[G * CM_NH * CIN + base_b + offb[m]];
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(vb, wrb[m], acc[j], 0, 0, 0);
    }
  }
  // D: lane (col o = r, rows 4 g4 + i) -> pair (a = G, b = 4 g4 + i), channel o
  if (r < COUT) {
    const float bias = MODE == 0 ? ba[r] + bb[r] : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int G = wv * 4 + j;
      const int ha = ha0 + G / CM_T, wa = wa0 + G % CM_T;
      if (ha >= hA || wa >= wA) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int bt = 4 * g4 + i;
        const int hb = hb0 + bt / CM_T, wb = wb0 + bt % CM_T;
        if (hb < hB && wb < wB) {
          float* yp = y + (long)blockIdx.z * NA * NB * COUT + ((long)(ha * wA + wa) * NB + hb * wB + wb) * COUT + r;
          *yp = MODE == 0 ? fmaxf(acc[j][i] + bias, 0.f) : accum ? *yp + acc[j][i] : acc[j][i];
        }
      }
    }
  }
}

// Weight and bias gradients of one CenterPivotConv4d layer (the backward, match_bwd.hip) on the
// same matrix cores: dW[(side, tap, c)][o] = sum over pairs p of X_side,tap[p][c] G[p][o] is the
// transpose of the forward GEMM -- rows the 18 CIN (side, tap, channel) entries plus one row of
// ones (whose result is the bias gradient sum_p G[p][o]), columns the COUT output channels, K the
// pairs.  Workgroups stride over the forward's 4x4 (a) by 4x4 (b) tiles, staged as cm_stage does,
// with the tile's (ReLU-masked) output gradient beside them; MFMA k-step s takes pairs 4 s .. 4 s
// + 3 (lane group g4 = pair within the step), wave w the row blocks w, w + 4, ...; the sums stay
// in the accumulators across tiles and land in part[workgroup] ([(side, tap, o)][c], then the
// bias), summed in workgroup order by cp4d_wgrad_reduce_kernel.
template <int CIN, int COUT>
__global__ __launch_bounds__(256) void cp4d_wgrad_mfma_kernel(const float* __restrict__ x, const float* __restrict__ gm,
                                                              int B, int hA, int wA, int hB, int wB,
                                                              float* __restrict__ part) {
  constexpr int KE = 18 * CIN;              // (side, tap, c) rows; row KE = ones (the bias)
  constexpr int MB = (KE + 1 + 15) / 16;    // 16-row blocks
  constexpr int MW = (MB + 3) / 4;          // blocks per wave
  constexpr int EA = CmLds<CIN>::EA, EB = CmLds<CIN>::EB;
  constexpr int NE = 18 * COUT;
  __shared__ __attribute__((aligned(16))) float xs[EA + EB + 2];
  __shared__ float gl[CM_NT * CM_NT][COUT];
  float* xa = xs;
  float* xb = xs + EA;
  const int NA = hA * wA, NB = hB * wB;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int i16 = lane & 15, g4 = lane >> 4;
  // this lane's A rows: kind 0 data (LDS offset off[], box b[]), 1 the ones row, 2 padding
  int off[MW], kind[MW];
  bool inb[MW];
#pragma unroll
  for (int mw = 0; mw < MW; ++mw) {
    const int kk = 16 * (wv + 4 * mw) + i16;
    kind[mw] = kk < KE ? 0 : kk == KE ? 1 : 2;
    const int k2 = kk < KE ? kk : 0;
    const int side = k2 / (9 * CIN), tap = (k2 / CIN) % 9, c = k2 % CIN;
    const int ky = tap / 3, kx = tap - 3 * (tap / 3);
    inb[mw] = side != 0;
    off[mw] = side == 0 ? (ky * CM_H + kx) * CM_NT * CIN + c : EA + (ky * CM_H + kx) * CIN + c;
  }
  f32x4 acc[MW];
#pragma unroll
  for (int mw = 0; mw < MW; ++mw) acc[mw] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int ntbw = (wB + CM_T - 1) / CM_T, ntaw = (wA + CM_T - 1) / CM_T;
  const long ntb = (long)((hB + CM_T - 1) / CM_T) * ntbw, nta = (long)((hA + CM_T - 1) / CM_T) * ntaw;
  const long ntiles = (long)B * nta * ntb;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long tb = tile % ntb, rest = tile / ntb;
    const long ta = rest % nta, bz = rest / nta;
    const int ha0 = (int)(ta / ntaw) * CM_T, wa0 = (int)(ta % ntaw) * CM_T;
    const int hb0 = (int)(tb / ntbw) * CM_T, wb0 = (int)(tb % ntbw) * CM_T;
    __syncthreads();  // the previous tile's LDS reads are done
    cm_stage<CIN>(x, hA, wA, hB, wB, ha0, wa0, hb0, wb0, bz * NA * NB * CIN, xa, xb);
    for (int e = t; e < CM_NT * CM_NT * COUT; e += 256) {
      const int o = e % COUT, p = e / COUT;
      const int at = p / CM_NT, bt = p % CM_NT;
      const int ha = ha0 + at / CM_T, wa = wa0 + at % CM_T, hb = hb0 + bt / CM_T, wb = wb0 + bt % CM_T;
      const bool in = ha < hA && wa < wA && hb < hB && wb < wB;
      (&gl[0][0])[e] = in ? gm[(bz * NA * NB + (long)(ha * wA + wa) * NB + hb * wB + wb) * COUT + o] : 0.f;
    }
    __syncthreads();
#pragma unroll 4
    for (int st = 0; st < CM_NT * CM_NT / 4; ++st) {
      const int p = 4 * st + g4, at = p / CM_NT, bt = p % CM_NT;
      const int terma = (((at / CM_T) * CM_H + at % CM_T) * CM_NT + bt) * CIN;
      const int termb = (at * CM_NH + (bt / CM_T) * CM_H + bt % CM_T) * CIN;
      const float bv = i16 < COUT ? gl[p][i16 < COUT ? i16 : 0] : 0.f;
#pragma unroll
      for (int mw = 0; mw < MW; ++mw) {
        if (wv + 4 * mw >= MB) continue;
        const float av = kind[mw] == 0 ? xs[(inb[mw] ? termb : terma) + off[mw]] : kind[mw] == 1 ? 1.f : 0.f;
        acc[mw] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[mw], 0, 0, 0);
      }
    }
  }
  // D: lane (column o = i16, rows 4 g4 + r of block m)
  float* pw = part + (long)blockIdx.x * (NE * CIN + COUT);
  if (i16 < COUT) {
#pragma unroll
    for (int mw = 0; mw < MW; ++mw) {
      const int m = wv + 4 * mw;
      if (m >= MB) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kk = 16 * m + 4 * g4 + r;
        if (kk < KE) {
          const int side = kk / (9 * CIN), tap = (kk / CIN) % 9, c = kk % CIN;
          pw[((side * 9 + tap) * COUT + i16) * CIN + c] = acc[mw][r];
        } else if (kk == KE) {
          pw[NE * CIN + i16] = acc[mw][r];
        }
      }
    }
  }
}

// ---- the first consensus layer L -> 10 for any L up to CWT_MATCH_MAX_L (MMN with every
// bottleneck's correlation as a channel: 9, 13, 26, 30), forward, input gradient and weight
// gradient.  The kernels above stage all CIN channels of a tile (CmLds<CIN>: 46 KB at 10, 147 KB
// at 32), so these walk the channels in chunks of NC_CK = 8: 9 taps x 8 channels = 72 K rows, 18
// MFMAs per branch with no K padding, and two staged boxes of 8 x 592 floats = 37,888 B per
// workgroup (four workgroups per CU by LDS).  A box is held channel-major, xa[c][ah][bt] and
// xb[c][at][bh], planes NC_PL = 576 + 16 floats apart: the lane (row r, k group g4) of an MFMA
// operand reads plane g4 at r, bank 16 g4 + r (no conflict on the a box).  Channels at or past L
// and positions off the map are staged as 0, every global access guarded, so odd L and the last
// partial chunk need no other form.  4-B staging loads: a position's run of L floats is 8-B
// aligned only for even L.
constexpr int NC_PL = CM_NH * CM_NT + 16;
constexpr int NC_BOX = NC_CK * NC_PL;

// A lane value the optimiser must take as new at this point.  The kernels below loop over chunks,
// column groups or tiles around fully unrolled bodies; without it every address of the body that does
// not depend on the loop variable is hoisted out of the loop and kept in registers (256 VGPRs, one
// workgroup per CU; or spills at a higher occupancy).
__device__ __forceinline__ int nc_opaque(int v) {
  asm volatile("" : "+v"(v));
  return v;
}

// stage channels c0 .. c0 + CS - 1 (CS = 1, 2, 4 or 8: the chunk's live channels rounded up, so the
// short last chunk of L = 9 or 10 stages one or two planes, not eight)
template <int CS>
__device__ __forceinline__ void nc_stage_cs(const float* __restrict__ x, int C, int c0, int hA, int wA, int hB, int wB,
                                            int ha0, int wa0, int hb0, int wb0, long xoff, float* xa, float* xb) {
  const int NB = hB * wB;
  constexpr int NE = CM_NH * CM_NT * CS, IT = (NE + 255) / 256;  // loads per thread and box: 18 at CS = 8
  const int t = nc_opaque(threadIdx.x);
  float ra[IT], rb[IT];
#pragma unroll
  for (int k = 0; k < IT; ++k) {
    const int i = t + 256 * k;
    const int c = i % CS, p = i / CS;
    const int bt = p % CM_NT, ah = p / CM_NT;
    const int ha = ha0 - 1 + ah / CM_H, wa = wa0 - 1 + ah % CM_H;
    const int hb = hb0 + bt / CM_T, wb = wb0 + bt % CM_T;
    const bool in = i < NE && c0 + c < C && (unsigned)ha < (unsigned)hA && (unsigned)wa < (unsigned)wA && hb < hB &&
                    wb < wB;
    ra[k] = in ? x[xoff + (((long)(ha * wA + wa) * NB) + hb * wB + wb) * C + c0 + c] : 0.f;
  }
#pragma unroll
  for (int k = 0; k < IT; ++k) {
    const int i = t + 256 * k;
    const int c = i % CS, p = i / CS;
    const int bh = p % CM_NH, at = p / CM_NH;
    const int ha = ha0 + at / CM_T, wa = wa0 + at % CM_T;
    const int hb = hb0 - 1 + bh / CM_H, wb = wb0 - 1 + bh % CM_H;
    const bool in = i < NE && c0 + c < C && ha < hA && wa < wA && (unsigned)hb < (unsigned)hB &&
                    (unsigned)wb < (unsigned)wB;
    rb[k] = in ? x[xoff + (((long)(ha * wA + wa) * NB) + hb * wB + wb) * C + c0 + c] : 0.f;
  }
#pragma unroll
  for (int k = 0; k < IT; ++k) {
    const int i = t + 256 * k;
    if (i < NE) {
      xa[(i % CS) * NC_PL + i / CS] = ra[k];
      xb[(i % CS) * NC_PL + i / CS] = rb[k];
    }
  }
}
// nc live channels (workgroup-uniform): planes 0 .. nc - 1 are staged, the others are not read
__device__ __forceinline__ void nc_stage(const float* __restrict__ x, int C, int c0, int nc, int hA, int wA, int hB,
                                         int wB, int ha0, int wa0, int hb0, int wb0, long xoff, float* xa, float* xb) {
  if (nc > 4)
    nc_stage_cs<8>(x, C, c0, hA, wA, hB, wB, ha0, wa0, hb0, wb0, xoff, xa, xb);
  else if (nc > 2)
    nc_stage_cs<4>(x, C, c0, hA, wA, hB, wB, ha0, wa0, hb0, wb0, xoff, xa, xb);
  else if (nc > 1)
    nc_stage_cs<2>(x, C, c0, hA, wA, hB, wB, ha0, wa0, hb0, wb0, xoff, xa, xb);
  else
    nc_stage_cs<1>(x, C, c0, hA, wA, hB, wB, ha0, wa0, hb0, wb0, xoff, xa, xb);
}
// K row k of a chunk of nc channels -> (tap, channel): rows (tap, channel) dense, 9 nc of them
__device__ __forceinline__ void nc_row(int k, int nc, int& tap, int& c) {
  if (nc == NC_CK) {
    tap = k >> 3, c = k & 7;
  } else {
    tap = k / nc, c = k - tap * nc;
  }
}

// forward L -> 10: cp4d_mfma_kernel's groups (rows the 16 tile b positions of one tile a position,
// columns the output channels), the accumulators carried over the chunks, bias + ReLU once at the
// end.  K row k = 4 m + g4 of a chunk of nc live channels is (tap k / nc, channel k % nc), dense as
// cp4d_mfma_kernel's: ceil(9 nc / 4) MFMA steps per branch, 18 for a full chunk (tap m / 2, channel
// 4 (m & 1) + g4: the four lane groups read four planes, no bank conflict), 3 for one channel.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void cp4d_nc_fwd_kernel(const float* __restrict__ x, int L, int hA, int wA, int hB,
                                                          int wB, const float* __restrict__ Wa,
                                                          const float* __restrict__ ba, const float* __restrict__ Wb,
                                                          const float* __restrict__ bb, float* __restrict__ y) {
  constexpr int COUT = 10, NM = 9 * NC_CK / 4;
  __shared__ float xa[NC_BOX];
  __shared__ float xb[NC_BOX];
  const int NA = hA * wA, NB = hB * wB;
  const int ntb = (wB + CM_T - 1) / CM_T, nta = (wA + CM_T - 1) / CM_T;
  const int ta = blockIdx.y, tb = blockIdx.x;
  const int ha0 = (ta / nta) * CM_T, wa0 = (ta % nta) * CM_T;
  const int hb0 = (tb / ntb) * CM_T, wb0 = (tb % ntb) * CM_T;
  const long xoff = (long)blockIdx.z * NA * NB * L;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int r = lane & 15, g4 = lane >> 4;
  const int by = r / CM_T, bx = r % CM_T;
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int c0 = 0; c0 < L; c0 += NC_CK) {
    const int nc = min(NC_CK, L - c0);  // the chunk's live channels
    const int nm = (9 * nc + 3) >> 2;   // its MFMA steps per branch
    if (c0) __syncthreads();  // the previous chunk's LDS reads are done
    nc_stage(x, L, c0, nc, hA, wA, hB, wB, ha0, wa0, hb0, wb0, xoff, xa, xb);
    float wra[NM], wrb[NM];
    int offa[NM], offb[NM];
    const int g4 = nc_opaque(lane >> 4);
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      int tap, c;
      nc_row(4 * m + g4, nc, tap, c);
      const bool kin = tap < 9;  // rows past 9 nc: zero weights, a staged address
      tap = kin ? tap : 0, c = kin ? c : 0;
      const int ky = tap / 3, kx = tap - 3 * ky;
      const bool live = kin && r < COUT;
      const int wi = (r * L + c0 + c) * 9 + tap;
      wra[m] = live ? Wa[wi] : 0.f;
      wrb[m] = live ? Wb[wi] : 0.f;
      offa[m] = c * NC_PL + (ky * CM_H + kx) * CM_NT + r;
      offb[m] = c * NC_PL + (by + ky) * CM_H + bx + kx;
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      if (m < nm) {  // workgroup-uniform
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int G = wv * 4 + j, ay = G / CM_T, ax = G % CM_T;
          const float va = xa[offa[m] + (ay * CM_H + ax) * CM_NT];
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(va, wra[m], acc[j], 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int G = wv * 4 + j;
          const float vb = xb[offb[m] + G * CM_NH];
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(vb, wrb[m], acc[j], 0, 0, 0);
        }
      }
    }
  }
  // D: lane (col o = r, rows 4 g4 + i) -> pair (a = G, b = 4 g4 + i), channel o
  if (r < COUT) {
    const float bias = ba[r] + bb[r];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int G = wv * 4 + j;
      const int ha = ha0 + G / CM_T, wa = wa0 + G % CM_T;
      if (ha >= hA || wa >= wA) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int bt = 4 * g4 + i;
        const int hb = hb0 + bt / CM_T, wb = wb0 + bt % CM_T;
        if (hb < hB && wb < wB)
          y[(long)blockIdx.z * NA * NB * COUT + ((long)(ha * wA + wa) * NB + hb * wB + wb) * COUT + r] =
              fmaxf(acc[j][i] + bias, 0.f);
      }
    }
  }
}

// input gradient 10 -> L: cp4d_mfma_kernel<10, 1>'s tile (the 10-channel output gradient staged
// once by cm_stage<10>, 46 KB), the L output channels walked in groups of 16 MFMA columns with the
// group's transposed, flipped filters reloaded per group; dx accumulated when accum != 0.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void cp4d_nc_dgrad_kernel(const float* __restrict__ g, int L, int hA, int wA, int hB,
                                                            int wB, const float* __restrict__ Wa,
                                                            const float* __restrict__ Wb, float* __restrict__ dx,
                                                            int accum) {
  constexpr int CIN = 10, KT = 9 * CIN, NM = (KT + 3) / 4;
  __shared__ __attribute__((aligned(16))) float xa[CmLds<CIN>::EA + 2];
  __shared__ __attribute__((aligned(16))) float xb[CmLds<CIN>::EB + 2];
  const int NA = hA * wA, NB = hB * wB;
  const int ntb = (wB + CM_T - 1) / CM_T, nta = (wA + CM_T - 1) / CM_T;
  const int ta = blockIdx.y, tb = blockIdx.x;
  const int ha0 = (ta / nta) * CM_T, wa0 = (ta % nta) * CM_T;
  const int hb0 = (tb / ntb) * CM_T, wb0 = (tb % ntb) * CM_T;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int r = lane & 15, g4 = lane >> 4;
  cm_stage<CIN>(g, hA, wA, hB, wB, ha0, wa0, hb0, wb0, (long)blockIdx.z * NA * NB * CIN, xa, xb);
  __syncthreads();
  for (int o0 = 0; o0 < L; o0 += 16) {
    const int r = nc_opaque(lane & 15), g4 = nc_opaque(lane >> 4);
    const int base_b = ((r / CM_T) * CM_H + r % CM_T) * CIN;
    const int o = o0 + r;
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      const int k = 4 * m + g4;
      const bool kin = k < KT;
      const int tap = kin ? k / CIN : 0, c = kin ? k % CIN : 0;
      const int ky = tap / 3, kx = tap - 3 * (tap / 3);
      const bool live = kin && o < L;
      const int wi = live ? (c * L + o) * 9 + 8 - tap : 0;
      const float wra = live ? Wa[wi] : 0.f, wrb = live ? Wb[wi] : 0.f;
      const int offa = (ky * CM_H + kx) * CM_NT * CIN + c, offb = (ky * CM_H + kx) * CIN + c;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int G = wv * 4 + j, ay = G / CM_T, ax = G % CM_T;
        const float va = xa[((ay * CM_H + ax) * CM_NT + r) * CIN + offa];
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(va, wra, acc[j], 0, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int G = wv * 4 + j;
        const float vb = xb[G * CM_NH * CIN + base_b + offb];
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(vb, wrb, acc[j], 0, 0, 0);
      }
    }
    if (o < L) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int G = wv * 4 + j;
        const int ha = ha0 + G / CM_T, wa = wa0 + G % CM_T;
        if (ha >= hA || wa >= wA) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int bt = 4 * g4 + i;
          const int hb = hb0 + bt / CM_T, wb = wb0 + bt % CM_T;
          if (hb < hB && wb < wB) {
            float* yp = dx + (long)blockIdx.z * NA * NB * L + ((long)(ha * wA + wa) * NB + hb * wB + wb) * L + o;
            *yp = accum ? *yp + acc[j][i] : acc[j][i];
          }
        }
      }
    }
  }
}

// weight gradient of the L -> 10 layer: cp4d_wgrad_mfma_kernel with the (side, tap, channel) rows
// chunked -- workgroup (g, q) keeps the 18 nc rows (nc = 8 live channels, fewer in the last chunk; rows
// (side, tap, channel) dense: ceil(18 nc / 16) blocks of 16, 9 for a full chunk, three per wave at most)
// of channels 8 q .. 8 q + nc - 1 in its accumulators over tiles g, g + G, ... and writes them into
// part[g] in the same [(side, tap, o)][c] order, stride 180 L + 10, so the fixed-order
// cp4d_wgrad_reduce_kernel sums them unchanged.  No ones row: the bias gradients are summed in
// double by launch_cp4d_wgrad.  LDS: the two boxes and the tile's output gradient, 48,128 B.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void cp4d_nc_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ gm,
                                                            int B, int L, int hA, int wA, int hB, int wB,
                                                            float* __restrict__ part) {
  constexpr int COUT = 10, MB = 18 * NC_CK / 16, MW = (MB + 3) / 4, NE = 18 * COUT;
  __shared__ float xs[2 * NC_BOX];
  __shared__ float gl[CM_NT * CM_NT][COUT];
  float* xa = xs;
  float* xb = xs + NC_BOX;
  const int NA = hA * wA, NB = hB * wB;
  const int c0 = blockIdx.y * NC_CK;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int i16 = lane & 15, g4 = lane >> 4;
  const int nc = min(NC_CK, L - c0);   // live channels of this chunk
  const int nrow = 18 * nc, mbl = (nrow + 15) >> 4;  // its rows and 16-row blocks
  int off[MW];
  bool inb[MW];
#pragma unroll
  for (int mw = 0; mw < MW; ++mw) {
    const int kk = min(16 * (wv + 4 * mw) + i16, nrow - 1);  // rows past the last: a staged address, never written
    int st, c;
    nc_row(kk, nc, st, c);  // st = side * 9 + tap
    const int side = st / 9, tap = st - 9 * side;
    const int ky = tap / 3, kx = tap - 3 * (tap / 3);
    inb[mw] = side != 0;
    off[mw] = c * NC_PL + (side == 0 ? (ky * CM_H + kx) * CM_NT : NC_BOX + ky * CM_H + kx);
  }
  f32x4 acc[MW];
#pragma unroll
  for (int mw = 0; mw < MW; ++mw) acc[mw] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int ntbw = (wB + CM_T - 1) / CM_T, ntaw = (wA + CM_T - 1) / CM_T;
  const long ntb = (long)((hB + CM_T - 1) / CM_T) * ntbw, nta = (long)((hA + CM_T - 1) / CM_T) * ntaw;
  const long ntiles = (long)B * nta * ntb;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long tb = tile % ntb, rest = tile / ntb;
    const long ta = rest % nta, bz = rest / nta;
    const int ha0 = (int)(ta / ntaw) * CM_T, wa0 = (int)(ta % ntaw) * CM_T;
    const int hb0 = (int)(tb / ntbw) * CM_T, wb0 = (int)(tb % ntbw) * CM_T;
    __syncthreads();  // the previous tile's LDS reads are done
    nc_stage(x, L, c0, nc, hA, wA, hB, wB, ha0, wa0, hb0, wb0, bz * NA * NB * L, xa, xb);
    for (int e = nc_opaque(t); e < CM_NT * CM_NT * COUT; e += 256) {
      const int o = e % COUT, p = e / COUT;
      const int at = p / CM_NT, bt = p % CM_NT;
      const int ha = ha0 + at / CM_T, wa = wa0 + at % CM_T, hb = hb0 + bt / CM_T, wb = wb0 + bt % CM_T;
      const bool in = ha < hA && wa < wA && hb < hB && wb < wB;
      (&gl[0][0])[e] = in ? gm[(bz * NA * NB + (long)(ha * wA + wa) * NB + hb * wB + wb) * COUT + o] : 0.f;
    }
    __syncthreads();
#pragma unroll 4
    for (int st = 0; st < CM_NT * CM_NT / 4; ++st) {
      const int p = 4 * st + g4, at = p / CM_NT, bt = p % CM_NT;
      const int terma = ((at / CM_T) * CM_H + at % CM_T) * CM_NT + bt;
      const int termb = at * CM_NH + (bt / CM_T) * CM_H + bt % CM_T;
      const float bv = i16 < COUT ? gl[p][i16] : 0.f;
#pragma unroll
      for (int mw = 0; mw < MW; ++mw) {
        if (wv + 4 * mw >= mbl) continue;  // wave-uniform
        const float av = xs[(inb[mw] ? termb : terma) + off[mw]];
        acc[mw] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[mw], 0, 0, 0);
      }
    }
  }
  // D: lane (column o = i16, rows 4 g4 + r of block m)
  float* pw = part + (long)blockIdx.x * (NE * L + COUT);
  if (i16 < COUT) {
#pragma unroll
    for (int mw = 0; mw < MW; ++mw) {
      const int m = wv + 4 * mw;
      if (m >= mbl) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kk = 16 * m + 4 * g4 + r;
        int st, c;
        nc_row(kk, nc, st, c);
        if (kk < nrow) pw[(st * COUT + i16) * L + c0 + c] = acc[mw][r];
      }
    }
  }
}

// COUT = 1 (the consensus stack's last layer, CIN = 10): a thread per (a, b) pair of the same
// staged tile, its channels read 2 at a time (ds_read_b64), the 2 x 9 x CIN weights in LDS read
// as wave-uniform broadcasts, two independent partial sums per thread.
template <int CIN>
__global__ __launch_bounds__(256) void cp4d_c1_kernel(const float* __restrict__ x, int hA, int wA, int hB, int wB,
                                                      const float* __restrict__ Wa, const float* __restrict__ ba,
                                                      const float* __restrict__ Wb, const float* __restrict__ bb,
                                                      float* __restrict__ y) {
  static_assert(CIN % 2 == 0, "pairs of channels");
  __shared__ __attribute__((aligned(16))) float xa[CmLds<CIN>::EA + 2];
  __shared__ __attribute__((aligned(16))) float xb[CmLds<CIN>::EB + 2];
  __shared__ __attribute__((aligned(16))) float wl[2][9][CIN];
  const int NA = hA * wA, NB = hB * wB;
  const int ntb = (wB + CM_T - 1) / CM_T, nta = (wA + CM_T - 1) / CM_T;
  const int ta = blockIdx.y, tb = blockIdx.x;
  const int ha0 = (ta / nta) * CM_T, wa0 = (ta % nta) * CM_T;
  const int hb0 = (tb / ntb) * CM_T, wb0 = (tb % ntb) * CM_T;
  const long xoff = (long)blockIdx.z * NA * NB * CIN;
  const int t = threadIdx.x;
  if (t < 2 * 9 * CIN) {
    const int c = t % CIN, tap = (t / CIN) % 9, side = t / (9 * CIN);
    (&wl[0][0][0])[t] = (side ? Wb : Wa)[c * 9 + tap];
  }
  cm_stage<CIN>(x, hA, wA, hB, wB, ha0, wa0, hb0, wb0, xoff, xa, xb);
  __syncthreads();
  const int at = t / CM_NT, bt = t % CM_NT;
  const int ay = at / CM_T, ax = at % CM_T, by = bt / CM_T, bx = bt % CM_T;
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  float s0 = 0.f, s1 = 0.f;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int ky = tap / 3, kx = tap % 3;
    const float* pa = &xa[(((ay + ky) * CM_H + ax + kx) * CM_NT + bt) * CIN];
    const float* pb = &xb[(at * CM_NH + (by + ky) * CM_H + bx + kx) * CIN];
#pragma unroll
    for (int c2 = 0; c2 < CIN / 2; ++c2) {
      const f32x2 va = *(const f32x2*)(pa + 2 * c2), vb = *(const f32x2*)(pb + 2 * c2);
      const f32x2 wa = *(const f32x2*)&wl[0][tap][2 * c2], wb = *(const f32x2*)&wl[1][tap][2 * c2];
      s0 = fmaf(wa[0], va[0], s0);
      s1 = fmaf(wa[1], va[1], s1);
      s0 = fmaf(wb[0], vb[0], s0);
      s1 = fmaf(wb[1], vb[1], s1);
    }
  }
  const int ha = ha0 + ay, wa = wa0 + ax, hb = hb0 + by, wb = wb0 + bx;
  if (ha < hA && wa < wA && hb < hB && wb < wB)
    y[(long)blockIdx.z * NA * NB + (long)(ha * wA + wa) * NB + hb * wB + wb] = fmaxf((s0 + s1) + (ba[0] + bb[0]), 0.f);
}

// ---- persistent forms (round 4, second pass): the tile kernels above spent ~85 % of a wave's
// life outside the matrix pipe (PMC: SQ_VALU_MFMA_BUSY 40 % of the 10 -> 10 layer's time, a wave
// living 41 k cycles for 5.9 k of MFMA) -- each workgroup staged its tile, then loaded its weights
// (46 scattered loads per lane), then computed, with nothing to overlap the loads but the two
// other workgroups on the CU.  Here a workgroup stays resident over tiles t, t + G, t + 2G, ...:
// weights and per-lane LDS offsets are formed once, and the next tile's staging loads are issued
// into registers right after the current tile is stored to LDS, so they fly under its MFMAs.
// Same staged layout, same per-output fmaf chains (the K order below only changes which MFMA
// carries which (tap, channel) row: the f32 MFMA accumulates one product at a time, in K order,
// so the sums differ from the tile kernels' only in that order).
template <int CIN>
struct CmRegs {
  static constexpr int V = (CIN % 2 == 0) ? 2 : 1, VP = CIN / V;
  static constexpr int LA = CM_NH * CM_NT * VP, LB = CM_NT * CM_NH * VP;
  static constexpr int IA = (LA + 255) / 256, IB = (LB + 255) / 256;
  typedef float vec_t __attribute__((ext_vector_type(V)));
  vec_t ra[IA], rb[IB];
};

// tile t of the grid of (a tile, b tile, batch) -> its origin and input offset
struct CmTile {
  int ha0, wa0, hb0, wb0, z;
};
__device__ __forceinline__ CmTile cm_tile(int t, int nta, int ntb, int NTA, int NTB) {
  const int per = NTA * NTB;
  const int z = t / per, r = t - z * per;
  const int ta = r / NTB, tb = r - ta * NTB;
  return CmTile{(ta / nta) * CM_T, (ta % nta) * CM_T, (tb / ntb) * CM_T, (tb % ntb) * CM_T, z};
}

// Tile schedule of the persistent kernels.  order 0: workgroup w takes tiles w, w + G, ... of
// the (batch, a tile, b tile) order, b fastest.  order 1: the same order cut into 8 contiguous
// ranges, one per XCD (workgroup w runs on XCD w % 8 when G % 8 == 0), so the tiles that share
// staged data share an L2.  order 2: as 1, with the tiles visited by rows of b tiles, a tiles
// fastest within a row (the b-halo strip of a row is then streamed once per a tile, the a halo
// slides along wa inside one L2).
struct CmSched {
  int cur, end, step;
};
__device__ __forceinline__ CmSched cm_sched(int ntiles, int order) {
  if (order == 0 || (gridDim.x & 7)) return CmSched{(int)blockIdx.x, ntiles, (int)gridDim.x};
  const int xcd = blockIdx.x & 7, per = (ntiles + 7) / 8;
  return CmSched{xcd * per + (int)(blockIdx.x >> 3), min(ntiles, (xcd + 1) * per), (int)(gridDim.x >> 3)};
}
__device__ __forceinline__ int cm_order(int l, int order, int NTA, int NTB, int nbb) {
  if (order < 2) return l;
  const int per = NTA * NTB, z = l / per, r = l - z * per;
  const int full = (NTB / nbb) * nbb;
  int ta, tb;
  if (r < NTA * full) {
    const int blk = r / (NTA * nbb), rem = r - blk * NTA * nbb;
    ta = rem / nbb;
    tb = blk * nbb + rem % nbb;
  } else {
    const int r2 = r - NTA * full, nl = NTB - full;
    ta = r2 / nl;
    tb = full + r2 % nl;
  }
  return z * per + ta * NTB + tb;
}

template <int CIN>
__device__ __forceinline__ void cm_load(CmRegs<CIN>& R, const float* __restrict__ x, int hA, int wA, int hB, int wB,
                                        const CmTile& T) {
  using Rg = CmRegs<CIN>;
  typedef typename Rg::vec_t vec_t;
  constexpr int V = Rg::V, VP = Rg::VP;
  const int NB = hB * wB;
  const float* xz = x + (long)T.z * hA * wA * NB * CIN;
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < Rg::IA; ++k) {
    int i = t + 256 * k;
    asm volatile("" : "+v"(i));  // re-derive the indices per tile: hoisted, 24 loads' worth held ~120 VGPRs
    const int q = i % VP, p = i / VP;
    const int bt = p % CM_NT, ah = p / CM_NT;
    const int ha = T.ha0 - 1 + ah / CM_H, wa = T.wa0 - 1 + ah % CM_H;
    const int hb = T.hb0 + bt / CM_T, wb = T.wb0 + bt % CM_T;
    const bool in = i < Rg::LA && (unsigned)ha < (unsigned)hA && (unsigned)wa < (unsigned)wA && hb < hB && wb < wB;
    R.ra[k] = in ? *(const vec_t*)(xz + (((long)(ha * wA + wa) * NB) + hb * wB + wb) * CIN + q * V) : vec_t(0.f);
  }
#pragma unroll
  for (int k = 0; k < Rg::IB; ++k) {
    int i = t + 256 * k;
    asm volatile("" : "+v"(i));
    const int q = i % VP, p = i / VP;
    const int bh = p % CM_NH, at = p / CM_NH;
    const int ha = T.ha0 + at / CM_T, wa = T.wa0 + at % CM_T;
    const int hb = T.hb0 - 1 + bh / CM_H, wb = T.wb0 - 1 + bh % CM_H;
    const bool in = i < Rg::LB && ha < hA && wa < wA && (unsigned)hb < (unsigned)hB && (unsigned)wb < (unsigned)wB;
    R.rb[k] = in ? *(const vec_t*)(xz + (((long)(ha * wA + wa) * NB) + hb * wB + wb) * CIN + q * V) : vec_t(0.f);
  }
}

template <int CIN>
__device__ __forceinline__ void cm_store(const CmRegs<CIN>& R, float* xa, float* xb) {
  using Rg = CmRegs<CIN>;
  typedef typename Rg::vec_t vec_t;
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < Rg::IA; ++k) {
    const int i = t + 256 * k;
    if (i < Rg::LA) *(vec_t*)(xa + i * Rg::V) = R.ra[k];
  }
#pragma unroll
  for (int k = 0; k < Rg::IB; ++k) {
    const int i = t + 256 * k;
    if (i < Rg::LB) *(vec_t*)(xb + i * Rg::V) = R.rb[k];
  }
}

// K order of the persistent MFMA kernel (per branch): first the F = CIN / 4 full channel quads
// of every tap (MFMA m < 9 F: tap m / F, channels 4 (m % F) + g4 -- the four lane groups share the
// tap, so the LDS offset is the lane's base + an immediate), then the R = CIN % 4 leftover
// channels of PER = 4 / R taps per MFMA (lane group g4: tap i PER + g4 / R, channel 4F + g4 % R;
// offsets formed once into registers).  CIN = 10: 18 + 5 = 23 MFMAs (92 rows, as before).
template <int CIN>
struct CmK {
  static constexpr int F = CIN / 4, R = CIN % 4;
  static constexpr int PER = R ? 4 / R : 1;
  static constexpr int NFULL = 9 * F;
  // F even: the full quads of a tap go in MFMA pairs (2p, 2p + 1) whose lane group g4 takes the
  // ADJACENT channels 8 q + 2 g4 and 8 q + 2 g4 + 1 -- one ds_read_b64 feeds both MFMAs
  static constexpr bool PAIR = F % 2 == 0 && F > 0;
  static constexpr int NMIX = R ? (9 + PER - 1) / PER : 0;
  static constexpr int NM = NFULL + NMIX;
};
__device__ __forceinline__ constexpr int cm_toff(int tap) { return (tap / 3) * CM_H + tap % 3; }  // halo position

template <int CIN>
__global__ __launch_bounds__(256) void cp4d_mfma_persist_kernel(const float* __restrict__ x, int hA, int wA, int hB,
                                                                int wB, int ntiles, const float* __restrict__ Wa,
                                                                const float* __restrict__ ba,
                                                                const float* __restrict__ Wb,
                                                                const float* __restrict__ bb, float* __restrict__ y,
                                                                int dbg, int order) {
  constexpr int COUT = 10;
  using K = CmK<CIN>;
  constexpr int NM = K::NM, NMIX = K::NMIX;
  __shared__ __attribute__((aligned(16))) float xa[CmLds<CIN>::EA + 2];
  __shared__ __attribute__((aligned(16))) float xb[CmLds<CIN>::EB + 2];
  const int NA = hA * wA, NB = hB * wB;
  const int ntb = (wB + CM_T - 1) / CM_T, nta = (wA + CM_T - 1) / CM_T;
  const int NTB = ntb * ((hB + CM_T - 1) / CM_T), NTA = nta * ((hA + CM_T - 1) / CM_T);
  const int t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const int r = lane & 15, g4 = lane >> 4;
  CmSched sc = cm_sched(ntiles, order);
  if (sc.cur >= sc.end) return;
  int tile = cm_order(sc.cur, order, NTA, NTB, ntb);
  CmRegs<CIN> R;
  cm_load<CIN>(R, x, hA, wA, hB, wB, cm_tile(tile, nta, ntb, NTA, NTB));
  // weights (B operand: column r = output channel) in this K order, and the mixed MFMAs' offsets
  float wra[NM], wrb[NM];
  int mixa[NMIX > 0 ? NMIX : 1], mixb[NMIX > 0 ? NMIX : 1];
#pragma unroll
  for (int m = 0; m < NM; ++m) {
    int tap, c;
    bool kin;
    if (m < K::NFULL && K::PAIR) {
      const int pp = m / 2, h = m % 2;
      tap = pp / (K::F / 2);
      c = 8 * (pp % (K::F / 2)) + 2 * g4 + h;
      kin = true;
    } else if (m < K::NFULL) {
      tap = m / K::F;
      c = 4 * (m % K::F) + g4;
      kin = true;
    } else {
      const int i = m - K::NFULL;
      tap = i * K::PER + g4 / (K::R ? K::R : 1);
      c = 4 * K::F + g4 % (K::R ? K::R : 1);
      kin = g4 / (K::R ? K::R : 1) < K::PER && tap < 9;
      if (!kin) tap = c = 0;
      mixa[i] = cm_toff(tap) * CM_NT * CIN + c;
      mixb[i] = cm_toff(tap) * CIN + c;
    }
    const bool live = kin && r < COUT;
    wra[m] = live ? Wa[(r * CIN + c) * 9 + tap] : 0.f;
    wrb[m] = live ? Wb[(r * CIN + c) * 9 + tap] : 0.f;
  }
  const float bias = r < COUT ? ba[r] + bb[r] : 0.f;
  // row r of group j: a tile position (wv, j), b tile position r = (by, bx)
  const int by = r / CM_T, bx = r % CM_T;
  const float* pa = xa + (wv * CM_H * CM_NT + r) * CIN;                // + j CM_NT CIN + offsets
  const float* pb = xb + (wv * CM_T * CM_NH + by * CM_H + bx) * CIN;   // + j CM_NH CIN + offsets
  for (;;) {
    const CmTile T = cm_tile(tile, nta, ntb, NTA, NTB);
    sc.cur += sc.step;
    const bool more = sc.cur < sc.end;
    tile = cm_order(more ? sc.cur : 0, order, NTA, NTB, ntb);
    __syncthreads();  // the previous tile's LDS reads are done
    cm_store<CIN>(R, xa, xb);
    __syncthreads();
    if (more && !(dbg & 2)) cm_load<CIN>(R, x, hA, wA, hB, wB, cm_tile(tile, nta, ntb, NTA, NTB));
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    typedef float f32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int m = 0; m < (K::PAIR ? K::NFULL : 0); m += 2) {
      if (dbg & 1) break;
      const int pp = m / 2, tap = pp / (K::F / 2), q8 = 8 * (pp % (K::F / 2)) + 2 * g4;
      const int oa = cm_toff(tap) * CM_NT * CIN + q8, ob = cm_toff(tap) * CIN + q8;
      f32x2 va[4], vb[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        va[j] = *(const f32x2*)(pa + j * CM_NT * CIN + oa);
        vb[j] = *(const f32x2*)(pb + j * CM_NH * CIN + ob);
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[j][h], wra[m + h], acc[j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(vb[j][h], wrb[m + h], acc[j], 0, 0, 0);
      }
    }
#pragma unroll
    for (int m = K::PAIR ? K::NFULL : 0; m < NM; ++m) {
      if (dbg & 1) break;  // timing study: staging only (CWT_CP4D_DBG=1); 2: compute only
      int oa, ob;
      if (m < K::NFULL) {
        oa = cm_toff(m / K::F) * CM_NT * CIN + 4 * (m % K::F) + g4;
        ob = cm_toff(m / K::F) * CIN + 4 * (m % K::F) + g4;
      } else {
        oa = mixa[m - K::NFULL];
        ob = mixb[m - K::NFULL];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[j * CM_NT * CIN + oa], wra[m], acc[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(pb[j * CM_NH * CIN + ob], wrb[m], acc[j], 0, 0, 0);
    }
    // D: lane (col o = r, rows 4 g4 + i) -> pair (a = (wv, j), b = 4 g4 + i), channel o
    if (r < COUT) {
      float* yz = y + (long)T.z * NA * NB * COUT;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ha = T.ha0 + wv, wa = T.wa0 + j;
        if (ha >= hA || wa >= wA) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int hb = T.hb0 + g4, wb = T.wb0 + i;
          if (hb < hB && wb < wB) yz[((long)(ha * wA + wa) * NB + hb * wB + wb) * COUT + r] = fmaxf(acc[j][i] + bias, 0.f);
        }
      }
    }
    if (!more) break;
  }
}

// COUT = 1, persistent: cp4d_c1_kernel's per-pair arithmetic over the same staged tiles
template <int CIN>
__global__ __launch_bounds__(256) void cp4d_c1_persist_kernel(const float* __restrict__ x, int hA, int wA, int hB,
                                                              int wB, int ntiles, const float* __restrict__ Wa,
                                                              const float* __restrict__ ba,
                                                              const float* __restrict__ Wb,
                                                              const float* __restrict__ bb, float* __restrict__ y,
                                                              int dbg, int order) {
  static_assert(CIN % 2 == 0, "pairs of channels");
  __shared__ __attribute__((aligned(16))) float xa[CmLds<CIN>::EA + 2];
  __shared__ __attribute__((aligned(16))) float xb[CmLds<CIN>::EB + 2];
  __shared__ __attribute__((aligned(16))) float wl[2][9][CIN];
  const int NA = hA * wA, NB = hB * wB;
  const int ntb = (wB + CM_T - 1) / CM_T, nta = (wA + CM_T - 1) / CM_T;
  const int NTB = ntb * ((hB + CM_T - 1) / CM_T), NTA = nta * ((hA + CM_T - 1) / CM_T);
  const int t = threadIdx.x;
  CmSched sc = cm_sched(ntiles, order);
  if (sc.cur >= sc.end) return;
  int tile = cm_order(sc.cur, order, NTA, NTB, ntb);
  CmRegs<CIN> R;
  cm_load<CIN>(R, x, hA, wA, hB, wB, cm_tile(tile, nta, ntb, NTA, NTB));
  if (t < 2 * 9 * CIN) {
    const int c = t % CIN, tap = (t / CIN) % 9, side = t / (9 * CIN);
    (&wl[0][0][0])[t] = (side ? Wb : Wa)[c * 9 + tap];
  }
  const float bias = ba[0] + bb[0];
  const int at = t / CM_NT, bt = t % CM_NT;
  const int ay = at / CM_T, ax = at % CM_T, by = bt / CM_T, bx = bt % CM_T;
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  for (;;) {
    const CmTile T = cm_tile(tile, nta, ntb, NTA, NTB);
    sc.cur += sc.step;
    const bool more = sc.cur < sc.end;
    tile = cm_order(more ? sc.cur : 0, order, NTA, NTB, ntb);
    __syncthreads();
    cm_store<CIN>(R, xa, xb);
    __syncthreads();
    if (more && !(dbg & 2)) cm_load<CIN>(R, x, hA, wA, hB, wB, cm_tile(tile, nta, ntb, NTA, NTB));
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      if (dbg & 1) break;
      const int ky = tap / 3, kx = tap % 3;
      const float* pa = &xa[(((ay + ky) * CM_H + ax + kx) * CM_NT + bt) * CIN];
      const float* pb = &xb[(at * CM_NH + (by + ky) * CM_H + bx + kx) * CIN];
#pragma unroll
      for (int c2 = 0; c2 < CIN / 2; ++c2) {
        const f32x2 va = *(const f32x2*)(pa + 2 * c2), vb = *(const f32x2*)(pb + 2 * c2);
        const f32x2 wa = *(const f32x2*)&wl[0][tap][2 * c2], wb = *(const f32x2*)&wl[1][tap][2 * c2];
        s0 = fmaf(wa[0], va[0], s0);
        s1 = fmaf(wa[1], va[1], s1);
        s0 = fmaf(wb[0], vb[0], s0);
        s1 = fmaf(wb[1], vb[1], s1);
      }
    }
    const int ha = T.ha0 + ay, wa = T.wa0 + ax, hb = T.hb0 + by, wb = T.wb0 + bx;
    if (ha < hA && wa < wA && hb < hB && wb < wB)
      y[(long)T.z * NA * NB + (long)(ha * wA + wa) * NB + hb * wB + wb] = fmaxf((s0 + s1) + bias, 0.f);
    if (!more) break;
  }
}

// ---- rolling-window form (round 4, third pass): the tile kernels above stage a cross-shaped
// box per 4x4-by-4x4 tile and so read every input 4.5 times (2.33 GB per 10 -> 10 layer at 60^2,
// 2.0 GB of it past the L2s: staging-bound).  Here a workgroup owns a 4 x 12 tile of
// b positions and a strip of 4 a rows, and walks the strip's a columns left to right: the window
// holds the 6 a rows (strip + halo) x 3 a columns of the b box (the tile + its 1-position ring,
// 6 x 14), so each step loads ONE new a column -- the a-plane convolution reads an input
// (4 + 2) / 4 times, the b-plane convolution only the ring around the tile (the tile itself is
// already in the window): ~2.2 reads per input.  The new column's loads are issued into
// registers before the current column's MFMAs and stored after them.  MFMA layout and K order
// as cp4d_mfma_persist_kernel (rows: 16 b positions of one a position; columns: the 10 outputs;
// CmK's K order); wave w takes a row w of the strip, its three groups the tile's 48 b positions.
// MODE 1: the input gradient (launch_cp4d_dgrad), as cp4d_mfma_kernel's MODE 1.
constexpr int RL_XH = RL_BH + 2, RL_XW = RL_BW + 2;
constexpr int RL_NT = RL_BH * RL_BW, RL_NX = RL_XH * RL_XW, RL_ROWS = RL_RA + 2;
static_assert(RL_NT == 48, "three 16-row MFMA groups per a position");

// four column slots per a row (one barrier per step: the column stored in step wa is read from
// step wa + 1 on, into the slot last read in step wa - 1; three slots need a second barrier and
// measured 3 % slower)
template <int CIN>
struct RlWin {
  static constexpr int NS = 4;
  static constexpr int V = (CIN % 2 == 0) ? 2 : 1, VP = CIN / V;
  static constexpr int SLOT = RL_NX * CIN;        // floats of one (a row, column slot): the b box
  static constexpr int ROW = NS * SLOT;           // NS column slots per a row
  static constexpr int FLOATS = RL_ROWS * ROW;
  static constexpr int L = RL_ROWS * RL_NX * VP;  // loads per window column
  static constexpr int IL = (L + 255) / 256;
  static constexpr int LDS = FLOATS + (IL * 256 - L) * V + 4;  // + a dummy tail for the spare lanes
  typedef float vec_t __attribute__((ext_vector_type(V)));
};

// The window column's loads, branch-free: a buffer resource based at the column (num_records 0
// off the map), per-lane byte offsets out of range where the position is off the map or unused.
template <int CIN, int V, int IL, typename vec_t>
__device__ __forceinline__ void rl_load(vec_t (&rg)[IL], const int (&goff)[IL], const float* xz, int col, int wA,
                                        int NA, int NB) {
  const bool colin = (unsigned)col < (unsigned)wA;
  const float* base = xz + (colin ? (long)col * NB * CIN : 0L);
  const int nrec = colin ? (int)((long)(NA - col) * NB * CIN * 4) : 0;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, (short)0, nrec, 0x00020000);
#pragma unroll
  for (int k = 0; k < IL; ++k) {
    if constexpr (V == 2) {
      typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
      const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, goff[k], 0, 0);
      rg[k] = __builtin_bit_cast(vec_t, v);
    } else {
      rg[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, goff[k], 0, 0));
    }
  }
}

template <int CIN, int MODE, int PF>
__global__ __launch_bounds__(256) void cp4d_roll_kernel(const float* __restrict__ x, int hA, int wA, int hB, int wB,
                                                        int nsa, int wc, const float* __restrict__ Wa,
                                                        const float* __restrict__ ba, const float* __restrict__ Wb,
                                                        const float* __restrict__ bb, float* __restrict__ y,
                                                        int accum, int dbg) {
  constexpr int COUT = 10;
  using K = CmK<CIN>;
  using Wn = RlWin<CIN>;
  typedef typename Wn::vec_t vec_t;
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  constexpr int NM = K::NM, NMIX = K::NMIX, V = Wn::V, VP = Wn::VP;
  __shared__ __attribute__((aligned(16))) float win[Wn::LDS];
  const int NA = hA * wA, NB = hB * wB;
  const int ntbw = (wB + RL_BW - 1) / RL_BW;
  const int hb0 = ((int)blockIdx.x / ntbw) * RL_BH, wb0 = ((int)blockIdx.x % ntbw) * RL_BW;
  const int c0 = blockIdx.y * wc, c1 = min(wA, c0 + wc);
  const int z = blockIdx.z / nsa, ha0 = (blockIdx.z % nsa) * RL_RA;
  const float* xz = x + (long)z * NA * NB * CIN;
  float* yz = y + (long)z * NA * NB * COUT;
  const int t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const int r = lane & 15, g4 = lane >> 4;
  // this thread's share of a window column: global offset at a column 0 (+ col NB CIN), -1 when
  // off the map or not needed (the ring of the two halo rows), and its LDS offset in a slot
  int goff[Wn::IL], loff[Wn::IL];
#pragma unroll
  for (int k = 0; k < Wn::IL; ++k) {
    const int i = t + 256 * k;
    const int q = i % VP, p = i / VP;
    const int pos = p % RL_NX, row = p / RL_NX;
    const int py = pos / RL_XW, px = pos % RL_XW;
    const int ha = ha0 - 1 + row, hb = hb0 - 1 + py, wb = wb0 - 1 + px;
    const bool ring = py == 0 || py == RL_XH - 1 || px == 0 || px == RL_XW - 1;
    const bool in = i < Wn::L && (!ring || (row >= 1 && row <= RL_RA)) && (unsigned)ha < (unsigned)hA &&
                    (unsigned)hb < (unsigned)hB && (unsigned)wb < (unsigned)wB;
    goff[k] = in ? (((ha * wA) * NB + hb * wB + wb) * CIN + q * V) * 4 : RL_OOR;
    loff[k] = i < Wn::L ? row * Wn::ROW + pos * CIN + q * V : Wn::FLOATS + (i - Wn::L) * V;
  }
  vec_t rg[Wn::IL];
  auto load = [&](int col) { rl_load<CIN, Wn::V, Wn::IL>(rg, goff, xz, col, wA, NA, NB); };
  auto store = [&](int slot) {
#pragma unroll
    for (int k = 0; k < Wn::IL; ++k) *(vec_t*)(win + (k < Wn::IL - 1 || loff[k] < Wn::FLOATS ? slot * Wn::SLOT : 0) + loff[k]) = rg[k];
  };
  load(c0 - 1);
  // weights (B operand: column r = output channel) in CmK's K order; the mixed MFMAs' offsets:
  // a plane (ky ROW + c) * 4 + kx (the column slot picked per step), b plane the box offset
  float wra[NM], wrb[NM];
  int mixa[NMIX > 0 ? NMIX : 1], mixb[NMIX > 0 ? NMIX : 1];
#pragma unroll
  for (int m = 0; m < NM; ++m) {
    int tap, c;
    bool kin;
    if (m < K::NFULL && K::PAIR) {
      const int pp = m / 2, h = m % 2;
      tap = pp / (K::F / 2);
      c = 8 * (pp % (K::F / 2)) + 2 * g4 + h;
      kin = true;
    } else if (m < K::NFULL) {
      tap = m / K::F;
      c = 4 * (m % K::F) + g4;
      kin = true;
    } else {
      const int i = m - K::NFULL;
      tap = i * K::PER + g4 / (K::R ? K::R : 1);
      c = 4 * K::F + g4 % (K::R ? K::R : 1);
      kin = g4 / (K::R ? K::R : 1) < K::PER && tap < 9;
      if (!kin) tap = c = 0;
      mixa[i] = ((tap / 3) * Wn::ROW + c) * 4 + tap % 3;
      mixb[i] = ((tap / 3 - 1) * RL_XW + tap % 3 - 1) * CIN + c;
    }
    const bool live = kin && r < COUT;
    const int wi = MODE == 0 ? (r * CIN + c) * 9 + tap : (c * COUT + r) * 9 + 8 - tap;
    wra[m] = live ? Wa[wi] : 0.f;
    wrb[m] = live ? Wb[wi] : 0.f;
  }
  const float bias = (MODE == 0 && r < COUT) ? ba[r] + bb[r] : 0.f;
  // group j's row r: tile b position 16 j + 4 (r % 4) + r / 4 -> its box position (times CIN); the
  // D rows 4 g4 + i of a lane are then the positions 16 j + 4 i + g4, so each of its stores covers
  // 4 consecutive b positions (160 contiguous bytes) instead of 4 positions 4 apart
  int pbj[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int tp = 16 * j + 4 * (r & 3) + (r >> 2);  // D row 4 g4 + i <-> tile position 16 j + 4 i + g4
    pbj[j] = ((tp / RL_BW + 1) * RL_XW + tp % RL_BW + 1) * CIN;
  }
  const float* wwin = win + wv * Wn::ROW;  // a row wv of the strip: window rows wv .. wv + 2
  const int ha = ha0 + wv;
  int yoff[3][4];  // byte offsets of this lane's outputs from column wa's base
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int tp = 16 * j + 4 * i + g4;  // one store instruction: 4 consecutive b positions x 10 outputs
      const int hb = hb0 + tp / RL_BW, wb = wb0 + tp % RL_BW;
      yoff[j][i] = (r < COUT && ha < hA && hb < hB && wb < wB) ? ((ha * wA * NB + hb * wB + wb) * COUT + r) * 4 : RL_OOR;
    }
  vec_t rg2[Wn::IL];
  auto load2 = [&](int col) { rl_load<CIN, Wn::V, Wn::IL>(rg2, goff, xz, col, wA, NA, NB); };
  auto store2 = [&](int slot) {
#pragma unroll
    for (int k = 0; k < Wn::IL; ++k) *(vec_t*)(win + (k < Wn::IL - 1 || loff[k] < Wn::FLOATS ? slot * Wn::SLOT : 0) + loff[k]) = rg2[k];
  };
  // step wa: publish column wa + 1 (barrier), store column wa + 2 into the slot of column wa - 2,
  // issue the loads of column wa + 1 + PF (PF = 2: two register sets, even / odd steps), compute
  // column wa from the slots of columns wa - 1, wa, wa + 1
  auto step = [&](int wa, auto&& st, auto&& ld) {
    const int s = (wa - c0) & 3;  // slot of column wa - 1
    __syncthreads();
    if (wa + 2 <= c1) st((s + 3) & 3);
    if (wa + 2 + PF <= c1 && !(dbg & 2)) ld(wa + 2 + PF);  // dbg (timing study): 2 no loads, 1 no arithmetic
    const int cb0 = s * Wn::SLOT, cb1 = ((s + 1) & 3) * Wn::SLOT, cb2 = ((s + 2) & 3) * Wn::SLOT;
    f32x4 acc[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m = 0; m < (K::PAIR ? K::NFULL : 0); m += 2) {
      if (dbg & 1) break;
      const int pp = m / 2, tap = pp / (K::F / 2), q8 = 8 * (pp % (K::F / 2)) + 2 * g4;
      const int ky = tap / 3, kx = tap % 3;
      const int oa = ky * Wn::ROW + (kx == 0 ? cb0 : kx == 1 ? cb1 : cb2) + q8;
      const int ob = Wn::ROW + cb1 + ((ky - 1) * RL_XW + kx - 1) * CIN + q8;
      f32x2 va[3], vb[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        va[j] = *(const f32x2*)(wwin + oa + pbj[j]);
        vb[j] = *(const f32x2*)(wwin + ob + pbj[j]);
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(va[j][h], wra[m + h], acc[j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(vb[j][h], wrb[m + h], acc[j], 0, 0, 0);
      }
    }
#pragma unroll
    for (int m = K::PAIR ? K::NFULL : 0; m < NM; ++m) {
      if (dbg & 1) break;
      int oa, ob;
      if (m < K::NFULL) {
        const int tap = m / K::F, ky = tap / 3, kx = tap % 3, c = 4 * (m % K::F) + g4;
        oa = ky * Wn::ROW + (kx == 0 ? cb0 : kx == 1 ? cb1 : cb2) + c;
        ob = Wn::ROW + cb1 + ((ky - 1) * RL_XW + kx - 1) * CIN + c;
      } else {
        const int ma = mixa[m - K::NFULL], kx = ma & 3;
        oa = (ma >> 2) + (kx == 0 ? cb0 : kx == 1 ? cb1 : cb2);
        ob = Wn::ROW + cb1 + mixb[m - K::NFULL];
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wwin[oa + pbj[j]], wra[m], acc[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wwin[ob + pbj[j]], wrb[m], acc[j], 0, 0, 0);
    }
    // D: lane (col o = r, rows 4 g4 + i) -> pair (a = (ha, wa), b = tile position 16 j + 4 g4 + i),
    // stored through a resource based at column wa (off-map pairs and dead columns: offset RL_OOR)
    {
      const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(yz + (long)wa * NB * COUT), (short)0, (int)((long)(NA - wa) * NB * COUT * 4), 0x00020000);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float v = MODE == 0 ? fmaxf(acc[j][i] + bias, 0.f) : acc[j][i];
          if (MODE == 1 && accum)
            v += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ry, yoff[j][i], 0, 0));
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ry, yoff[j][i], 0, 0);
        }
      }
    }
  };
  store(0);
  load(c0);
  store(1);
  load(c0 + 1);
  store(2);
  if (c0 + 2 <= c1) load(c0 + 2);
  if (PF == 2 && c0 + 3 <= c1) load2(c0 + 3);
  for (int wa = c0; wa < c1; wa += PF) {
    step(wa, store, load);
    if (PF == 2 && wa + 1 < c1) step(wa + 1, store2, load2);
  }
}

// COUT = 1 on the same rolling window (VALU: cp4d_c1_kernel's per-pair fmaf chains, the two
// branches' even / odd channels in two partial sums); thread t < 192 takes strip row t / 48 and
// tile b position t % 48; the filters are wave-uniform scalar loads (broadcast from LDS they made
// the kernel LDS-bound: 497 against 355 us at 60^2).
template <int CIN, int PF>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void cp4d_c1_roll_kernel(const float* __restrict__ x, int hA, int wA, int hB, int wB,
                                                           int nsa, int wc, const float* __restrict__ Wa,
                                                           const float* __restrict__ ba,
                                                           const float* __restrict__ Wb,
                                                           const float* __restrict__ bb, float* __restrict__ y,
                                                           int dbg) {
  static_assert(CIN % 2 == 0, "pairs of channels");
  using Wn = RlWin<CIN>;
  typedef typename Wn::vec_t vec_t;
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  constexpr int V = Wn::V, VP = Wn::VP;
  __shared__ __attribute__((aligned(16))) float win[Wn::LDS];
  const int NA = hA * wA, NB = hB * wB;
  const int ntbw = (wB + RL_BW - 1) / RL_BW;
  const int hb0 = ((int)blockIdx.x / ntbw) * RL_BH, wb0 = ((int)blockIdx.x % ntbw) * RL_BW;
  const int c0 = blockIdx.y * wc, c1 = min(wA, c0 + wc);
  const int z = blockIdx.z / nsa, ha0 = (blockIdx.z % nsa) * RL_RA;
  const float* xz = x + (long)z * NA * NB * CIN;
  float* yz = y + (long)z * NA * NB;
  const int t = threadIdx.x;
  int goff[Wn::IL], loff[Wn::IL];
#pragma unroll
  for (int k = 0; k < Wn::IL; ++k) {
    const int i = t + 256 * k;
    const int q = i % VP, p = i / VP;
    const int pos = p % RL_NX, row = p / RL_NX;
    const int py = pos / RL_XW, px = pos % RL_XW;
    const int ha = ha0 - 1 + row, hb = hb0 - 1 + py, wb = wb0 - 1 + px;
    const bool ring = py == 0 || py == RL_XH - 1 || px == 0 || px == RL_XW - 1;
    const bool in = i < Wn::L && (!ring || (row >= 1 && row <= RL_RA)) && (unsigned)ha < (unsigned)hA &&
                    (unsigned)hb < (unsigned)hB && (unsigned)wb < (unsigned)wB;
    goff[k] = in ? (((ha * wA) * NB + hb * wB + wb) * CIN + q * V) * 4 : RL_OOR;
    loff[k] = i < Wn::L ? row * Wn::ROW + pos * CIN + q * V : Wn::FLOATS + (i - Wn::L) * V;
  }
  vec_t rg[Wn::IL];
  auto load = [&](int col) { rl_load<CIN, Wn::V, Wn::IL>(rg, goff, xz, col, wA, NA, NB); };
  auto store = [&](int slot) {
#pragma unroll
    for (int k = 0; k < Wn::IL; ++k) *(vec_t*)(win + (k < Wn::IL - 1 || loff[k] < Wn::FLOATS ? slot * Wn::SLOT : 0) + loff[k]) = rg[k];
  };
  load(c0 - 1);
  const float bias = ba[0] + bb[0];
  const bool act = t < RL_RA * RL_NT;
  const int ai = act ? t / RL_NT : 0, tp = act ? t % RL_NT : 0;
  const int pb = ((tp / RL_BW + 1) * RL_XW + tp % RL_BW + 1) * CIN;
  const int ha = ha0 + ai, hb = hb0 + tp / RL_BW, wb = wb0 + tp % RL_BW;
  const bool outp = act && ha < hA && hb < hB && wb < wB;
  const int yoff = outp ? (ha * wA * NB + hb * wB + wb) * 4 : RL_OOR;  // from column wa's base
  const float* wwin = win + ai * Wn::ROW + pb;
  vec_t rg2[Wn::IL];
  auto load2 = [&](int col) { rl_load<CIN, Wn::V, Wn::IL>(rg2, goff, xz, col, wA, NA, NB); };
  auto store2 = [&](int slot) {
#pragma unroll
    for (int k = 0; k < Wn::IL; ++k) *(vec_t*)(win + (k < Wn::IL - 1 || loff[k] < Wn::FLOATS ? slot * Wn::SLOT : 0) + loff[k]) = rg2[k];
  };
  auto step = [&](int wa, auto&& st, auto&& ld) {  // as cp4d_roll_kernel's
    const int s = (wa - c0) & 3;
    __syncthreads();
    if (wa + 2 <= c1) st((s + 3) & 3);
    if (wa + 2 + PF <= c1 && !(dbg & 2)) ld(wa + 2 + PF);  // dbg (timing study): 2 no loads, 1 no arithmetic
    const int cb[3] = {s * Wn::SLOT, ((s + 1) & 3) * Wn::SLOT, ((s + 2) & 3) * Wn::SLOT};
    int wz = 0;
    asm volatile("" : "+s"(wz));  // the filters re-read per step as scalar loads (hoisted: 180 registers)
    const float* wga = Wa + wz;
    const float* wgb = Wb + wz;
    float s0 = 0.f, s1 = 0.f;
#pragma unroll 3
    for (int tap = 0; tap < 9; ++tap) {
      if (dbg & 1) break;
      const int ky = tap / 3, kx = tap % 3;
      const float* pa = wwin + ky * Wn::ROW + (kx == 0 ? cb[0] : kx == 1 ? cb[1] : cb[2]);
      const float* pbb = wwin + Wn::ROW + cb[1] + ((ky - 1) * RL_XW + kx - 1) * CIN;
#pragma unroll
      for (int c2 = 0; c2 < CIN / 2; ++c2) {
        const f32x2 va = *(const f32x2*)(pa + 2 * c2), vb = *(const f32x2*)(pbb + 2 * c2);
        const f32x2 w0 = {wga[(2 * c2) * 9 + tap], wga[(2 * c2 + 1) * 9 + tap]};
        const f32x2 w1 = {wgb[(2 * c2) * 9 + tap], wgb[(2 * c2 + 1) * 9 + tap]};
        s0 = fmaf(w0[0], va[0], s0);
        s1 = fmaf(w0[1], va[1], s1);
        s0 = fmaf(w1[0], vb[0], s0);
        s1 = fmaf(w1[1], vb[1], s1);
      }
    }
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(yz + (long)wa * NB), (short)0, (int)((long)(NA - wa) * NB * 4), 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, fmaxf((s0 + s1) + bias, 0.f)), ry, yoff, 0, 0);
  };
  store(0);
  load(c0);
  store(1);
  load(c0 + 1);
  store(2);
  if (c0 + 2 <= c1) load(c0 + 2);
  if (PF == 2 && c0 + 3 <= c1) load2(c0 + 3);
#pragma unroll 1
  for (int wa = c0; wa < c1; wa += PF) {
    step(wa, store, load);
    if (PF == 2 && wa + 1 < c1) step(wa + 1, store2, load2);
  }
}

// ---- CenterPivotConv4d weight / bias gradients (conv4d.py:40-62) ----
// dWa[o][c][tap] = sum over (a, b) of gm[a][b][o] x[a + tap - 1][b][c] (zero padding), dWb the
// same over the b plane, db[o] = sum gm[a][b][o] (conv1's and conv2's biases both).  Workgroups
// stride over 2x8 (a) by 2x8 (b) tiles, stage the tile's cross-shaped input and its gradient in
// LDS, and keep their partial sums in registers: thread = one (side, tap, o) entry with CIN
// accumulators, 256 / (18 COUT) thread groups over the tile's 256 pairs.  Partials per
// workgroup [G][18 COUT CIN + COUT], summed in workgroup order by cp4d_wgrad_reduce_kernel.
constexpr int WG_NA = WG_TAH * WG_TAW, WG_NB = WG_TBH * WG_TBW;
constexpr int WG_HA = (WG_TAH + 2) * (WG_TAW + 2), WG_HB = (WG_TBH + 2) * (WG_TBW + 2);

template <int CIN, int COUT>
__global__ __launch_bounds__(256) void cp4d_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ gm,
                                                         int B, int hA, int wA, int hB, int wB,
                                                         float* __restrict__ part) {
  constexpr int NE = 18 * COUT;
  constexpr int NG = 256 / NE;
  static_assert(NG >= 1, "COUT <= 14");
  __shared__ float xa[WG_HA][WG_NB][CIN];
  __shared__ float xb[WG_NA][WG_HB][CIN];
  __shared__ float gl[WG_NA * WG_NB][COUT];
  __shared__ float red[NG * NE][CIN + 1];
  const int NA = hA * wA, NB = hB * wB;
  const int t = threadIdx.x;
  const int e = t % NE, grp = t / NE;
  const bool active = grp < NG;
  const int side = e / (9 * COUT), tap = (e / COUT) % 9, o = e % COUT;
  const int ky = tap / 3, kx = tap - 3 * (tap / 3);
  float acc[CIN];
#pragma unroll
  for (int c = 0; c < CIN; ++c) acc[c] = 0.f;
  float bacc = 0.f;
  const int ntaw = (wA + WG_TAW - 1) / WG_TAW, ntah = (hA + WG_TAH - 1) / WG_TAH;
  const int ntbw = (wB + WG_TBW - 1) / WG_TBW, ntbh = (hB + WG_TBH - 1) / WG_TBH;
  const long ntb = (long)ntbh * ntbw, nta = (long)ntah * ntaw, ntiles = (long)B * nta * ntb;
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long tb = tile % ntb, rest = tile / ntb;
    const long ta = rest % nta, bz = rest / nta;
    const int ha0 = (int)(ta / ntaw) * WG_TAH, wa0 = (int)(ta % ntaw) * WG_TAW;
    const int hb0 = (int)(tb / ntbw) * WG_TBH, wb0 = (int)(tb % ntbw) * WG_TBW;
    const float* xz = x + bz * NA * NB * CIN;
    const float* gz = gm + bz * NA * NB * COUT;
    __syncthreads();  // the previous tile's LDS reads are done
    for (int i = t; i < WG_HA * WG_NB * CIN; i += 256) {  // a halo box at the tile's b positions
      const int c = i % CIN, p = i / CIN;
      const int bi = p % WG_NB, ai = p / WG_NB;
      const int ha = ha0 - 1 + ai / (WG_TAW + 2), wa = wa0 - 1 + ai % (WG_TAW + 2);
      const int hb = hb0 + bi / WG_TBW, wb = wb0 + bi % WG_TBW;
      const bool in = (unsigned)ha < (unsigned)hA && (unsigned)wa < (unsigned)wA && hb < hB && wb < wB;
      (&xa[0][0][0])[i] = in ? xz[((long)(ha * wA + wa) * NB + hb * wB + wb) * CIN + c] : 0.f;
    }
    for (int i = t; i < WG_NA * WG_HB * CIN; i += 256) {  // b halo box at the tile's a positions
      const int c = i % CIN, p = i / CIN;
      const int bi = p % WG_HB, ai = p / WG_HB;
      const int ha = ha0 + ai / WG_TAW, wa = wa0 + ai % WG_TAW;
      const int hb = hb0 - 1 + bi / (WG_TBW + 2), wb = wb0 - 1 + bi % (WG_TBW + 2);
      const bool in = ha < hA && wa < wA && (unsigned)hb < (unsigned)hB && (unsigned)wb < (unsigned)wB;
      (&xb[0][0][0])[i] = in ? xz[((long)(ha * wA + wa) * NB + hb * wB + wb) * CIN + c] : 0.f;
    }
    for (int i = t; i < WG_NA * WG_NB * COUT; i += 256) {  // the output gradient at the tile's pairs
      const int oo = i % COUT, p = i / COUT;
      const int ai = p / WG_NB, bi = p % WG_NB;
      const int ha = ha0 + ai / WG_TAW, wa = wa0 + ai % WG_TAW;
      const int hb = hb0 + bi / WG_TBW, wb = wb0 + bi % WG_TBW;
      const bool in = ha < hA && wa < wA && hb < hB && wb < wB;
      (&gl[0][0])[i] = in ? gz[((long)(ha * wA + wa) * NB + hb * wB + wb) * COUT + oo] : 0.f;
    }
    __syncthreads();
    if (active) {
      for (int p = grp; p < WG_NA * WG_NB; p += NG) {
        const int ai = p / WG_NB, bi = p - ai * WG_NB;
        const float gv = gl[p][o];
        const float* xv = side == 0
                              ? xa[(ai / WG_TAW + ky) * (WG_TAW + 2) + ai % WG_TAW + kx][bi]
                              : xb[ai][(bi / WG_TBW + ky) * (WG_TBW + 2) + bi % WG_TBW + kx];
#pragma unroll
        for (int c = 0; c < CIN; ++c) acc[c] = fmaf(gv, xv[c], acc[c]);
        bacc += gv;
      }
    }
  }
  __syncthreads();
  if (active) {
#pragma unroll
    for (int c = 0; c < CIN; ++c) red[t][c] = acc[c];
    red[t][CIN] = bacc;
  }
  __syncthreads();
  if (t < NE) {
    float s[CIN + 1];
#pragma unroll
    for (int c = 0; c <= CIN; ++c) s[c] = red[t][c];
    for (int g = 1; g < NG; ++g)
#pragma unroll
      for (int c = 0; c <= CIN; ++c) s[c] += red[g * NE + t][c];
    float* pw = part + (long)blockIdx.x * (NE * CIN + COUT);
#pragma unroll
    for (int c = 0; c < CIN; ++c) pw[t * CIN + c] = s[c];
    if (t < COUT) pw[NE * CIN + t] = s[CIN];  // side 0, tap 0, o = t
  }
}

// sum the partials in workgroup order; dWa / dWb [COUT][CIN][9] accumulate, and db1 / db2 [COUT]
// unless bias == 0 (cp4d_bias_grad_f64 sums those)
__global__ void cp4d_wgrad_reduce_kernel(const float* __restrict__ part, int G, int CIN, int COUT, float* dWa,
                                         float* dWb, float* db1, float* db2, int bias) {
  const int NE = 18 * COUT, n = NE * CIN + COUT;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n || (!bias && idx >= NE * CIN)) return;
  float s = 0.f;
  for (int g = 0; g < G; ++g) s += part[(long)g * n + idx];
  if (idx < NE * CIN) {
    const int e = idx / CIN, c = idx - e * CIN;
    const int side = e / (9 * COUT), tap = (e / COUT) % 9, o = e % COUT;
    float* W = side ? dWb : dWa;
    W[(o * CIN + c) * 9 + tap] += s;
  } else {
    const int o = idx - NE * CIN;
    db1[o] += s;
    db2[o] += s;
  }
}

// The bias gradients db1 = db2 += sum over every (a, b) pair of gm[p][o]: a sum of up to B (hA wA)
// (hB wB) terms whose ReLU-masked values cancel heavily (the last consensus layer's single bias is
// a few 1e-3 of sum |gm|), so it is accumulated in double, in a fixed order: chunks of
// CB64_ROWS rows per workgroup (a thread's rows strided by 256, then a fixed LDS tree), then the
// chunks in order.  Deterministic and accurate to the fp32 rounding of the result.
constexpr int CB64_ROWS = 16384, CB64_MAXC = 16;
__global__ __launch_bounds__(256) void colsum_f64_part_kernel(const float* __restrict__ X, long R, int Cc,
                                                              double* __restrict__ part) {
  __shared__ double red[256][CB64_MAXC + 1];
  const int t = threadIdx.x;
  const long r0 = (long)blockIdx.x * CB64_ROWS;
  const long r1 = min(R, r0 + CB64_ROWS);
  double acc[CB64_MAXC];
#pragma unroll
  for (int o = 0; o < CB64_MAXC; ++o) acc[o] = 0.0;
  for (long r = r0 + t; r < r1; r += 256)
#pragma unroll
    for (int o = 0; o < CB64_MAXC; ++o)
      if (o < Cc) acc[o] += (double)X[r * Cc + o];
#pragma unroll
  for (int o = 0; o < CB64_MAXC; ++o) red[t][o] = acc[o];
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (t < w)
      for (int o = 0; o < Cc; ++o) red[t][o] += red[t + w][o];
    __syncthreads();
  }
  if (t < Cc) part[(long)blockIdx.x * Cc + t] = red[0][t];
}

__global__ void colsum_f64_final_kernel(const double* __restrict__ part, int nch, int Cc, float* db1, float* db2) {
  const int o = threadIdx.x;
  if (o >= Cc) return;
  double s = 0.0;
  for (int c = 0; c < nch; ++c) s += part[(long)c * Cc + o];
  db1[o] = (float)((double)db1[o] + s);
  if (db2) db2[o] = (float)((double)db2[o] + s);
}


// ---- launchers: the plan (cp4d_plan.h) names the form, one switch instantiates it ----
#define CP4D_GO(KERNEL, ...)                                             \
  do {                                                                   \
    hipLaunchKernelGGL(KERNEL, grid, dim3(256), 0, st, __VA_ARGS__);     \
    CWT_LAUNCH_CHECK();                                                  \
    return 0;                                                            \
  } while (0)

// the persistent kernel's workgroups per CU, asked once per kernel: a device fact, not a knob
static int cp4d_persist_occ(int cin, int cout, int* occ) {
  static int cache[4] = {0, 0, 0, 0};
  const void* kernel[4] = {(const void*)cp4d_mfma_persist_kernel<1>, (const void*)cp4d_mfma_persist_kernel<2>,
                           (const void*)cp4d_mfma_persist_kernel<10>, (const void*)cp4d_c1_persist_kernel<10>};
  const int i = cout == 1 ? 3 : cin == 1 ? 0 : cin == 2 ? 1 : 2;
  if (!cache[i]) CWT_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&cache[i], kernel[i], 256, 0));
  *occ = cache[i];
  return 0;
}

// a forward (mode 0) or input-gradient (mode 1: ba, bb unused, accum adds into y) plan
static int cp4d_launch(const Cp4dPlan& p, const float* x, int hA, int wA, int hB, int wB, const float* Wa,
                       const float* ba, const float* Wb, const float* bb, float* y, int accum, hipStream_t st) {
  if (p.rc) return fail(p.rc, p.msg);
  const dim3 grid(p.gx, p.gy, p.gz);
  switch (p.form) {
    case CP4D_SCALAR:
#define CWT_CP(CI, CO, MD) \
  if (p.cin == CI && p.cout == CO && p.mode == MD) CP4D_GO((cp4d_layer_kernel<CI, CO, MD>), x, hA, wA, hB, wB, Wa, ba, Wb, bb, y, accum);
      CWT_CP(1, 10, 0)
      CWT_CP(2, 10, 0)
      CWT_CP(10, 10, 0)
      CWT_CP(10, 1, 0)
      CWT_CP(1, 10, 1)
      CWT_CP(10, 10, 1)
      CWT_CP(10, 1, 1)
      CWT_CP(10, 2, 1)
#undef CWT_CP
      break;
    case CP4D_TILE_MFMA:
#define CWT_CP(CI, MD) \
  if (p.cin == CI && p.mode == MD) CP4D_GO((cp4d_mfma_kernel<CI, MD>), x, hA, wA, hB, wB, Wa, ba, Wb, bb, y, accum);
      CWT_CP(1, 0)
      CWT_CP(2, 0)
      CWT_CP(10, 0)
      CWT_CP(1, 1)
      CWT_CP(10, 1)
#undef CWT_CP
      break;
    case CP4D_TILE_C1:
      CP4D_GO(cp4d_c1_kernel<10>, x, hA, wA, hB, wB, Wa, ba, Wb, bb, y);
    case CP4D_PERSIST_MFMA:
#define CWT_CP(CI) \
  if (p.cin == CI) CP4D_GO(cp4d_mfma_persist_kernel<CI>, x, hA, wA, hB, wB, p.ntiles, Wa, ba, Wb, bb, y, p.dbg, p.order);
      CWT_CP(1)
      CWT_CP(2)
      CWT_CP(10)
#undef CWT_CP
      break;
    case CP4D_PERSIST_C1:
      CP4D_GO(cp4d_c1_persist_kernel<10>, x, hA, wA, hB, wB, p.ntiles, Wa, ba, Wb, bb, y, p.dbg, p.order);
    case CP4D_ROLL:
#define CWT_CP(CI, MD)                                                                                          \
  if (p.cin == CI && p.mode == MD) {                                                                            \
    if (p.pf == 1)                                                                                              \
      CP4D_GO((cp4d_roll_kernel<CI, MD, 1>), x, hA, wA, hB, wB, p.nsa, p.wc, Wa, ba, Wb, bb, y, accum, p.dbg);  \
    CP4D_GO((cp4d_roll_kernel<CI, MD, 2>), x, hA, wA, hB, wB, p.nsa, p.wc, Wa, ba, Wb, bb, y, accum, p.dbg);    \
  }
      CWT_CP(1, 0)
      CWT_CP(2, 0)
      CWT_CP(10, 0)
      CWT_CP(1, 1)
      CWT_CP(10, 1)
#undef CWT_CP
      break;
    case CP4D_ROLL_C1:
      if (p.pf == 1) CP4D_GO((cp4d_c1_roll_kernel<10, 1>), x, hA, wA, hB, wB, p.nsa, p.wc, Wa, ba, Wb, bb, y, p.dbg);
      CP4D_GO((cp4d_c1_roll_kernel<10, 2>), x, hA, wA, hB, wB, p.nsa, p.wc, Wa, ba, Wb, bb, y, p.dbg);
    case CP4D_NC_FWD:
      CP4D_GO(cp4d_nc_fwd_kernel, x, p.cin, hA, wA, hB, wB, Wa, ba, Wb, bb, y);
    case CP4D_NC_DGRAD:
      CP4D_GO(cp4d_nc_dgrad_kernel, x, p.cout, hA, wA, hB, wB, Wa, Wb, y, accum);
    default:
      break;
  }
  return fail(CWT_ESTATE, "cp4d: the plan names a form with no kernel for these channels");
}

int launch_cp4d_layer(const float* x, int B, int hA, int wA, int hB, int wB, int cin, int cout, const float* Wa,
                      const float* ba, const float* Wb, const float* bb, float* y, hipStream_t st) {
  return launch_cp4d_layer_variant(x, B, hA, wA, hB, wB, cin, cout, Wa, ba, Wb, bb, y, 0, st);
}
// variant (cwt_debug_cp4d_layer): 0 the automatic choice, 1 never the rolling-window form, 2 only it,
// 3 the channel-chunked form
int launch_cp4d_layer_variant(const float* x, int B, int hA, int wA, int hB, int wB, int cin, int cout,
                              const float* Wa, const float* ba, const float* Wb, const float* bb, float* y, int variant,
                              hipStream_t st) {
  const Cp4dEnv env = cp4d_env();
  Cp4dPlan p = cp4d_plan_fwd(B, hA, wA, hB, wB, cin, cout, variant, env, 0, 0);
  if (!p.rc && (p.form == CP4D_PERSIST_MFMA || p.form == CP4D_PERSIST_C1)) {  // its grid fills the device: ask it
    int dev = 0, cu = 0, occ = 0, rc;
    CWT_HIP(hipGetDevice(&dev));
    CWT_HIP(hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev));
    if ((rc = cp4d_persist_occ(cin, cout, &occ))) return rc;
    p = cp4d_plan_fwd(B, hA, wA, hB, wB, cin, cout, variant, env, cu, occ);
  }
  return cp4d_launch(p, x, hA, wA, hB, wB, Wa, ba, Wb, bb, y, 0, st);
}

// the input gradient of one CenterPivotConv4d layer (mode 1 of the forward's kernels): g [B][NA][NB][gin]
// is the layer's ReLU-masked output gradient, dx [B][NA][NB][gout] (gout = the layer's input
// channels), Wa / Wb the a-plane / b-plane filters the forward applied ([gin][gout][3][3]);
// variant as the forward's (cwt_debug_cp4d_dgrad)
int launch_cp4d_dgrad(const float* g, int B, int hA, int wA, int hB, int wB, int gin, int gout, const float* Wa,
                      const float* Wb, float* dx, int accum, hipStream_t st, int variant) {
  return cp4d_launch(cp4d_plan_dgrad(B, hA, wA, hB, wB, gin, gout, variant, cp4d_env(), 0, 0), g, hA, wA, hB, wB, Wa,
                     nullptr, Wb, nullptr, dx, accum, st);
}

// dWa / dWb / db1 / db2 += the layer's weight and bias gradients; part: cp4d_wgrad_part_floats() floats
int launch_cp4d_wgrad(const float* x, const float* gm, int B, int hA, int wA, int hB, int wB, int cin, int cout,
                      float* part, size_t part_floats, float* dWa, float* dWb, float* db1, float* db2,
                      hipStream_t st) {
  const Cp4dPlan p = cp4d_plan_wgrad(B, hA, wA, hB, wB, cin, cout, 0, cp4d_env(), 0, 0);
  if (p.rc) return fail(p.rc, p.msg);
  const int G = p.G, n = p.n;
  if ((size_t)G * n > part_floats) return fail(CWT_ESTATE, "cp4d wgrad: partial workspace too small");
  const dim3 grid(p.gx, p.gy, p.gz);
#define CP4D_WG(KERNEL, ...)                                           \
  {                                                                    \
    hipLaunchKernelGGL(KERNEL, grid, dim3(256), 0, st, __VA_ARGS__);   \
    CWT_LAUNCH_CHECK();                                                \
    break;                                                             \
  }
#define CWT_CP(KERNEL, CI, CO) \
  if (cin == CI && cout == CO) CP4D_WG((KERNEL<CI, CO>), x, gm, B, hA, wA, hB, wB, part)
  switch (p.form) {
    case CP4D_WGRAD_MFMA:
      CWT_CP(cp4d_wgrad_mfma_kernel, 1, 10)
      CWT_CP(cp4d_wgrad_mfma_kernel, 2, 10)
      CWT_CP(cp4d_wgrad_mfma_kernel, 10, 10)
      CWT_CP(cp4d_wgrad_mfma_kernel, 10, 1)
      break;
    case CP4D_WGRAD_SCALAR:
      CWT_CP(cp4d_wgrad_kernel, 1, 10)
      CWT_CP(cp4d_wgrad_kernel, 2, 10)
      CWT_CP(cp4d_wgrad_kernel, 10, 10)
      CWT_CP(cp4d_wgrad_kernel, 10, 1)
      break;
    default:  // CP4D_NC_WGRAD
      CP4D_WG(cp4d_nc_wgrad_kernel, x, gm, B, cin, hA, wA, hB, wB, part)
  }
#undef CWT_CP
#undef CP4D_WG
  hipLaunchKernelGGL(cp4d_wgrad_reduce_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, (const float*)part, G, cin, cout,
                     dWa, dWb, db1, db2, 0);
  CWT_LAUNCH_CHECK();
  // the biases in double (the partials above are consumed: their workspace takes the chunks)
  const long R = (long)B * hA * wA * hB * wB;
  const int nch = (int)cdiv(R, (long)CB64_ROWS);
  if (cout > CB64_MAXC || (size_t)nch * cout * 2 > part_floats) return fail(CWT_ESTATE, "cp4d bias sum: workspace");
  hipLaunchKernelGGL(colsum_f64_part_kernel, dim3(nch), dim3(256), 0, st, gm, R, cout, (double*)part);
  CWT_LAUNCH_CHECK();
  hipLaunchKernelGGL(colsum_f64_final_kernel, dim3(1), dim3(64), 0, st, (const double*)part, nch, cout, db1, db2);
  CWT_LAUNCH_CHECK();
  return 0;
}
#undef CP4D_GO

}  // namespace cwt
