// Host side of the fusion trainer's kernels (fuse.hip; reference src/train_fuse.py and FuseNet1,
// src/model/transformer.py:286-330): the stack's geometry and the launchers api_fuse.hip calls.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace cwt {

constexpr int FUSE_C = 16;      // FuseNet1's hidden width (transformer.py:293)
constexpr int FUSE_NACC = 38;   // gradient sums per hidden channel: 9 + 9 + 1 (layer 1), 9 + 9 + 1 (layer 2)
constexpr int FUSE_MAXBLK = 1024;  // workgroups of the stack's backward: rows of its partial sums

// One correlation [B][hA*wA][hB*wB] through CenterPivotConv4d(1, 16, stride (1,1,2,2)), ReLU,
// CenterPivotConv4d(16, 1), ReLU: the support plane shrinks to mB x nB = ceil(hB/2) x ceil(wB/2)
struct FuseGeom {
  int B, hA, wA, hB, wB, mB, nB;
  __host__ __device__ long NA() const { return (long)hA * wA; }
  __host__ __device__ long NB() const { return (long)hB * wB; }
  __host__ __device__ long NB2() const { return (long)mB * nB; }
  __host__ __device__ long units() const { return (long)B * NA() * NB2(); }  // outputs of the stack; y1 has FUSE_C floats per unit
};
static inline FuseGeom fuse_geom(int B, int hA, int wA, int hB, int wB) {
  return FuseGeom{B, hA, wA, hB, wB, (hB + 1) / 2, (wB + 1) / 2};
}

// the eight parameter tensors in PyTorch's layout: layer 1 conv1 / conv2 weight [16][1][3][3] and
// bias [16], layer 2 conv1 / conv2 weight [1][16][3][3] and bias [1]; conv1 runs over the query
// plane, conv2 over the support plane (conv4d.py:16-19)
struct FuseParams {
  const float *w1a, *b1a, *w1b, *b1b, *w2a, *b2a, *w2b, *b2b;
};
struct FuseGrads {
  float *w1a, *b1a, *w1b, *b1b, *w2a, *b2a, *w2b, *b2b;
};

int fuse_bwd_blocks(const FuseGeom& g);
size_t fuse_bwd_part_doubles(const FuseGeom& g);

// y1 NULL: the fused forward (layer 1 recomputed on each output's cross-shaped halo, y1 never
// stored); y1 given: layer 1 to y1 [B][NA][NB2][16] (after its ReLU), then layer 2 from it.
// Both write y2 into X[(b * NA + a) * ldx + col + b'] and give the same bits.
int launch_fuse_stack(const float* x, const FuseGeom& g, const FuseParams& p, float* y1, float* X, long ldx, int col,
                      hipStream_t st);
// dX: the gradient at X (same ldx / col); part: fuse_bwd_part_doubles doubles
int launch_fuse_stack_bwd(const float* x, const FuseGeom& g, const FuseParams& p, const float* y1, const float* X,
                          const float* dX, long ldx, int col, int accumulate, const FuseGrads& d, double* part,
                          hipStream_t st);
int launch_fuse_support_mask(const int64_t* label, int H, int W, int m, int align_corners, int pool, float* out,
                             hipStream_t st);
int launch_fuse_mask_bias(const float* W, long ldw, int col, const float* s_mask, int n, const float* b, int mid,
                          float* b_eff, hipStream_t st);
int launch_fuse_mask_bias_bwd(const float* d_b, const float* s_mask, int mid, int n, float* d_W, long ldw, int col,
                              hipStream_t st);
int launch_fuse_softmax2(const float* z, int B, long P, float* wt, hipStream_t st);
int launch_fuse_softmax2_bwd(const float* wt, const float* d_wt, int B, long P, float* d_z, hipStream_t st);
int launch_fuse_blend(const float* wv, const float* fq, const float* wt, int B, long P, int C, float* out,
                      hipStream_t st);
int launch_fuse_blend_bwd(const float* wv, const float* fq, const float* d_out, int B, long P, int C, float* d_wt,
                          hipStream_t st);
// part: fuse_loss_part_doubles doubles, counts: fuse_loss_count_words words, sc: 2 doubles
size_t fuse_loss_part_doubles();
size_t fuse_loss_count_words();
int launch_fuse_loss_head(const float* pd_q, const float* pd_q0, const float* pd_q1, int h, int w,
                          const int64_t* label, int S, float* loss_out, float* d_pd_q, float* iut_out,
                          float* disagree_out, double* part, unsigned* counts, double* sc, hipStream_t st);

}  // namespace cwt
