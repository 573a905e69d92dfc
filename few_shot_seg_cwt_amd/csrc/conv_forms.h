// The kernel forms of the LDS-DMA conv family (conv_igemm_x3s / _b16 / _f32d in conv_x3s.hip,
// conv_igemm_x6 in conv_x6.hip): the one table that says which (tile, plan.var) pairs exist and
// which template arguments each launches.  The launcher (launch_form), the lookup behind
// launch_conv_x3s and the debug entry points (find_conv_form) and the exports
// cwt_debug_conv_form / cwt_debug_conv_plan are all generated from these lists; a pair with no
// row here is CWT_EARG, never another form.
#pragma once
#include <type_traits>

#include "kernels.h"

namespace cwt {

// X(bm, bn, var, WAVES_M, WAVES_N, NSTG, PF, FIXED): the form conv_igemm_*<bm, bn, WAVES_M, WAVES_N,
//   NSTG, STAGE, PF> (block = WAVES_M * WAVES_N * 64 threads; NSTG the LDS ring's depth; PF the
//   body's main-loop bits, conv_body.h: 1 prefetch, 2 / 4 / 16 / 32 / 64 timing studies, 128 two A
//   sources; 8 (buffer addressing) is set by every kernel, 256 (the GEMM-shaped path) by the x6
//   launcher for the rows of CWT_CONV_GEMM_ROWS_X6 below -- neither appears in a row).  FIXED = 1:
//   a timing-study form that carries its own tile -- the debug entry points replace whatever tile
//   is named beside its var with the row's (the grid must be the kernel's), and x3s / b16 / f32d
//   build it at STAGE 0 only.
// A(bm, bn, var, target): var on this tile launches the same tile's row `target`.
//
// All four families.  var 0 the base loop; 1 fragment prefetch, same waves; 2 prefetch with 8 waves
// (two per SIMD) on the 128- and 64-row tiles; 4 = 128x128 on a 2-stage ring (64 KB: two workgroups
// per CU).  Deeper rings measured no faster (a workgroup's LDS-DMA intake, not its bytes in flight,
// is the limit: DESIGN.md §3).  256x256 has no prefetch form: its second fragment set does not fit
// the 256 VGPRs of a wave at two waves per SIMD.
#define CWT_CONV_FORMS(X, A)                                                                   \
  X(256, 256, 0, 2, 4, 2, 0, 0) A(256, 256, 1, 0) A(256, 256, 2, 0)                            \
  X(256, 128, 0, 4, 2, 3, 0, 0) X(256, 128, 1, 4, 2, 3, 1, 0) A(256, 128, 2, 1)                \
  X(128, 256, 0, 2, 4, 3, 0, 0) X(128, 256, 1, 2, 4, 3, 1, 0) A(128, 256, 2, 1)                \
  X(128, 128, 0, 2, 2, 3, 0, 0) X(128, 128, 1, 2, 2, 3, 1, 0) X(128, 128, 2, 2, 4, 3, 1, 0)    \
  X(128, 128, 4, 2, 2, 2, 0, 0)                                                                \
  X(128, 64, 0, 2, 2, 3, 0, 0) X(128, 64, 1, 2, 2, 3, 1, 0) X(128, 64, 2, 4, 2, 3, 1, 0)       \
  X(64, 128, 0, 2, 2, 3, 0, 0) X(64, 128, 1, 2, 2, 3, 1, 0) X(64, 128, 2, 2, 4, 3, 1, 0)       \
  X(64, 64, 0, 2, 2, 4, 0, 0) X(64, 64, 1, 2, 2, 4, 1, 0) X(64, 64, 2, 2, 4, 4, 1, 0)          \
  /* timing study (wrong numbers): the base 64x64 without MFMAs / without operand DMA */       \
  X(64, 64, 8, 2, 2, 4, 2, 1) X(64, 64, 9, 2, 2, 4, 4, 1)                                      \
  /* ... and the 8-wave prefetch 128x128 the same */                                           \
  X(128, 128, 10, 2, 4, 3, 3, 1) X(128, 128, 11, 2, 4, 3, 5, 1)

// conv_igemm_x6 only.  Its main loop's VALU is the A split (~44 instructions per 8 fp32 values, per
// A fragment per K-tile) against 6 MFMAs per fragment pair, so a wave that holds more output columns
// amortises each split over more MFMAs: var 3 lays the waves out WN = 128 wide (FN = 8: ~0.9 VALU
// per MFMA against ~1.8 at WN = 64; profiles/r5), var 5 is var 3's 4x1 layout on a 2-stage ring
// (two workgroups per CU).  On 128x64 and 64x64 (the Co = 64 layers: stem conv2, layer1 conv1 /
// conv2, where the 2x2 forms split every A fragment twice) var 3 / 5 are 4x1 at WN = 64: the A
// split once per row block.
#define CWT_CONV_FORMS_X6(X, A)                                                                \
  X(256, 256, 3, 4, 2, 2, 0, 0) X(256, 128, 3, 8, 1, 2, 0, 0) X(128, 256, 3, 4, 2, 2, 0, 0)    \
  X(128, 128, 3, 4, 1, 3, 0, 0) X(128, 128, 5, 4, 1, 2, 0, 0)                                  \
  X(128, 64, 3, 4, 1, 3, 0, 0) X(128, 64, 5, 4, 1, 2, 0, 0)                                    \
  X(64, 128, 3, 4, 1, 3, 0, 0) X(64, 128, 5, 4, 1, 2, 0, 0)                                    \
  X(64, 64, 3, 4, 1, 4, 0, 0)                                                                  \
  /* timing study (wrong numbers): 128x128 var 5 without the A split (12), without operand */  \
  /* DMA (14), without MFMAs (15), without both (16), ... and without the epilogue (17), */    \
  /* the launch alone (18: every workgroup returns) */                                         \
  X(128, 128, 12, 4, 1, 2, 16, 0) X(128, 128, 14, 4, 1, 2, 4, 0) X(128, 128, 15, 4, 1, 2, 2, 0) \
  X(128, 128, 16, 4, 1, 2, 6, 0) X(128, 128, 17, 4, 1, 2, 38, 0) X(128, 128, 18, 4, 1, 2, 64, 0) \
  /* ... and 256x256 var 3 without the A split */                                              \
  X(256, 256, 13, 4, 2, 2, 16, 0)                                                              \
  /* two A sources (PF bit 128, ConvSArgs::xs2: conv3 + downsample conv as one GEMM): var  */  \
  /* kConvDualVar + v is var v's loop, on the tiles the fused shapes' plans take           */  \
  X(128, 128, 24, 2, 2, 2, 128, 0) X(128, 128, 25, 4, 1, 2, 128, 0)                            \
  X(128, 64, 25, 4, 1, 2, 128, 0) X(64, 128, 25, 4, 1, 2, 128, 0)

constexpr int kConvDualVar = 20;

// conv_igemm_x6 only: G(bm, bn, var) names a row above that also exists with PF bit 256, the
// GEMM-shaped path of conv_body.h.  The x6 launcher (conv_x6.hip), not the plan tables, takes it
// for a launch with kh == kw == 1 && pad == 0 -- every 1x1 conv, the two-source forms and the
// Winograd products -- unless CWT_X6_GEMM_BODY=0; a row not listed here runs its general form.
// The rows are those the 473^2 x 2 plan table (conv_plans_x6.inc) takes on such launches, each kept
// because no table shape ran slower on it than on the general body (profiles/r11/sweeps): var 3 / 4
// / 5 and the dual 24 / 25 on their tiles and the base 64x64.  The base 256x256 and 128x256 rows of
// the 473^2 x 4 and 641^2 tables have no GEMM-shaped body: not measured.
#define CWT_CONV_GEMM_ROWS_X6(G)                                                               \
  G(128, 128, 3) G(64, 64, 3) G(128, 128, 4) G(128, 128, 5) G(128, 64, 5) G(64, 128, 5)        \
  G(128, 128, 24) G(128, 128, 25) G(128, 64, 25) G(64, 128, 25) G(64, 64, 0)

constexpr bool x6_gemm_row(int bm, int bn, int var) {
#define CWT_G(BM, BN, VAR) \
  if (bm == BM && bn == BN && var == VAR) return true;
  CWT_CONV_GEMM_ROWS_X6(CWT_G)
#undef CWT_G
  return false;
}

struct ConvForm {
  int bm, bn, var, waves_m, waves_n, nstg, pf;
  bool fixed_tile;
  int alias;  // >= 0: no kernel of its own, launches row (bm, bn, alias)
};
// The row of (bm, bn, var) in the table of prec (0 f32d, 1 b16, 3 x3s, 6 x6), aliases resolved;
// nullptr: no such form
const ConvForm* find_conv_form(int prec, int bm, int bn, int var);
// The FIXED row of var (whatever tile), or nullptr
const ConvForm* fixed_tile_form(int prec, int var);

// f(std::integral_constant<int, S>) for the runtime stage: S = stage in [0, LAST), else LAST.  STAGE
// only names the instantiation for rocprofv3 (0 stem, 1-4 layer1-4, 5 PPM, 6 bottleneck; x6 also 7 /
// 8: the F(2x2) / F(4x4) Winograd forms' batched GEMMs, so their counters are not averaged with the
// direct convs').
template <int LAST, class F>
void with_stage(int stage, F&& f) {
  if constexpr (LAST > 0)
    if (stage >= 0 && stage < LAST) return with_stage<LAST - 1>(stage, f);
  f(std::integral_constant<int, LAST>{});
}

// Launch the row p names directly (aliases already resolved: find_conv_form).  Fam::launch<BM, BN,
// WAVES_M, WAVES_N, NSTG, STAGE, PF>(a, grid, st) launches the family's kernel; Fam::kX6 adds the
// x6-only rows, Fam::kStudyStage0 builds the FIXED rows at STAGE 0 only.  gemm (x6 only): a row of
// CWT_CONV_GEMM_ROWS_X6 launches its GEMM-shaped body (PF | 256), any other row its own.
template <class Fam, int STAGE>
void launch_form(const ConvPlan& p, const ConvSArgs& a, dim3 grid, hipStream_t st, bool gemm = false) {
#define CWT_ROW(BM, BN, VAR, WM, WN, NS, PF, FIXED)                                            \
  if (p.bm == BM && p.bn == BN && p.var == VAR) {                                              \
    constexpr int S = (FIXED && Fam::kStudyStage0) ? 0 : STAGE;                                \
    if constexpr (Fam::kX6 && x6_gemm_row(BM, BN, VAR))                                        \
      if (gemm) return Fam::template launch<BM, BN, WM, WN, NS, S, (PF) | 256>(a, grid, st);   \
    return Fam::template launch<BM, BN, WM, WN, NS, S, PF>(a, grid, st);                       \
  }
#define CWT_ALIAS(BM, BN, VAR, TARGET)
  CWT_CONV_FORMS(CWT_ROW, CWT_ALIAS)
  if constexpr (Fam::kX6) {
    CWT_CONV_FORMS_X6(CWT_ROW, CWT_ALIAS)
  }
#undef CWT_ROW
#undef CWT_ALIAS
}

// The family of one kernel template: launch<...> with the block size its wave layout implies
#define CWT_CONV_FAMILY(NAME, KERNEL, X6, STUDY_STAGE0)                                        \
  struct NAME {                                                                                \
    static constexpr bool kX6 = X6, kStudyStage0 = STUDY_STAGE0;                               \
    template <int BM, int BN, int WM, int WN, int NS, int STAGE, int PF>                       \
    static void launch(const ConvSArgs& a, dim3 grid, hipStream_t st) {                        \
      hipLaunchKernelGGL((KERNEL<BM, BN, WM, WN, NS, STAGE, PF>), grid, dim3(WM * WN * 64), 0, st, a); \
    }                                                                                          \
  }

}  // namespace cwt
