// The host-side plan of one CenterPivotConv4d consensus layer (cp4d.hip): which kernel form a
// shape takes in each direction -- forward, input gradient, weight gradient -- with which template
// arguments, grid and knobs.  One value per launch, computed by cp4d_plan_fwd / _dgrad / _wgrad
// from the shape, the channels, the debug variant, the environment's knobs and two device facts;
// the launchers, cwt_debug_cp4d_plan and the tests all read it, and nothing else chooses a form.
// Host only: no HIP call, includable from a plain C++ file.
#pragma once
#include <algorithm>
#include <cstdlib>

#include "../../include/cwt.h"

namespace cwt {

// ---- the tiles the grids are computed from (the kernels in cp4d.hip are written for them) ----
constexpr int CP_TAH = 2, CP_TAW = 8, CP_TBH = 2, CP_TBW = 8;  // scalar kernel: a patch x b patch
constexpr int CM_T = 4;                                        // matrix-core / C1 / chunked forms: 4 x 4 by 4 x 4
constexpr int RL_BH = 4, RL_BW = 12, RL_RA = 4;                // rolling window: b tile, a rows per strip
constexpr int RL_OOR = 0x40000000;  // a buffer offset past every num_records: loads read 0, stores drop
constexpr int NC_CK = 8;            // channels per chunk of the chunked forms
constexpr int WG_TAH = 2, WG_TAW = 8, WG_TBH = 2, WG_TBW = 8;  // weight gradient: a patch x b patch
// workgroups of the weight-gradient pass: 512 for the 10 -> 10 layer (two per CU by LDS), 2048 for
// the thinner layers (less LDS each; measured 0.52 against 1.26 ms for 2 -> 10 at 60^2); 256 per
// channel chunk for the chunked L -> 10 form (its partials are 180 L + 10 floats)
constexpr int WG_G_WIDE = 512, WG_G_THIN = 2048, WG_G_NC = 256;

enum Cp4dForm : int {
  // cp4d_layer_kernel: CWT_CP4D_MFMA=0 forward (16 % of the fp32 VALU peak at 60^2), and the input
  // gradients with no matrix-core form (10 -> 1, 10 -> 2) or under CWT_DGRAD_SCALAR=1
  CP4D_SCALAR = 0,
  // cp4d_mfma_kernel: 10 output channels, one tile per workgroup, where neither the rolling window
  // nor the persistent form is taken (2 -> 10: 297 against 331 us persistent at 60^2); MODE 1 the
  // input gradient where the rolling window refuses the shape
  CP4D_TILE_MFMA = 1,
  // cp4d_c1_kernel: 10 -> 1 as the tile form (471 against 605 us persistent at 60^2)
  CP4D_TILE_C1 = 2,
  // cp4d_mfma_persist_kernel: persistent workgroups with the next tile's loads in flight; 10 -> 10
  // by default (1,169 against 1,207 us at 60^2), every width with CWT_CP4D_PERSIST=2, none with =0
  CP4D_PERSIST_MFMA = 3,
  // cp4d_c1_persist_kernel: 10 -> 1 persistent, CWT_CP4D_PERSIST=2 only
  CP4D_PERSIST_C1 = 4,
  // cp4d_roll_kernel: the first choice for 10 output channels, forward and input gradient, while
  // a batch entry's byte offsets stay below RL_OOR (691 against 1,171 us for 10 -> 10 at 60^2);
  // CWT_CP4D_ROLL=0 never
  CP4D_ROLL = 5,
  // cp4d_c1_roll_kernel: 10 -> 1 (its VALU form with the filters from scalar loads: 355 against the
  // tile kernel's 482 us at 60^2); CWT_CP4D_ROLL=2 (default), not =1
  CP4D_ROLL_C1 = 6,
  // cp4d_nc_{fwd,dgrad,wgrad}_kernel: a first layer of any width 1 .. CWT_MATCH_MAX_L other than
  // 1, 2 and 10 (MMN's every-block channels), in chunks of NC_CK channels; 1.40x the tile kernel
  // at equal work, so never chosen where an instantiated form exists (debug variant 3 forces it)
  CP4D_NC_FWD = 7,
  CP4D_NC_DGRAD = 8,
  CP4D_NC_WGRAD = 9,
  // cp4d_wgrad_mfma_kernel: the weight gradient of every instantiated width
  CP4D_WGRAD_MFMA = 10,
  // cp4d_wgrad_kernel: CWT_WGRAD_SCALAR=1 (A/B only)
  CP4D_WGRAD_SCALAR = 11,
};
constexpr int CP4D_NFORMS = 12;

// A form's name, its kernel and the plan fields that are the kernel's template arguments, in order
struct Cp4dFormInfo {
  const char *name, *kernel, *targs;
};
constexpr Cp4dFormInfo cp4d_form_info(int form) {
  switch (form) {
    case CP4D_SCALAR: return {"scalar", "cp4d_layer_kernel", "cin,cout,mode"};
    case CP4D_TILE_MFMA: return {"tile_mfma", "cp4d_mfma_kernel", "cin,mode"};
    case CP4D_TILE_C1: return {"tile_c1", "cp4d_c1_kernel", "cin"};
    case CP4D_PERSIST_MFMA: return {"persist_mfma", "cp4d_mfma_persist_kernel", "cin"};
    case CP4D_PERSIST_C1: return {"persist_c1", "cp4d_c1_persist_kernel", "cin"};
    case CP4D_ROLL: return {"roll", "cp4d_roll_kernel", "cin,mode,pf"};
    case CP4D_ROLL_C1: return {"roll_c1", "cp4d_c1_roll_kernel", "cin,pf"};
    case CP4D_NC_FWD: return {"nc_fwd", "cp4d_nc_fwd_kernel", ""};
    case CP4D_NC_DGRAD: return {"nc_dgrad", "cp4d_nc_dgrad_kernel", ""};
    case CP4D_NC_WGRAD: return {"nc_wgrad", "cp4d_nc_wgrad_kernel", ""};
    case CP4D_WGRAD_MFMA: return {"wgrad_mfma", "cp4d_wgrad_mfma_kernel", "cin,cout"};
    case CP4D_WGRAD_SCALAR: return {"wgrad_scalar", "cp4d_wgrad_kernel", "cin,cout"};
    default: return {nullptr, nullptr, nullptr};
  }
}

// The environment's say in the plan.  Read once per launch and never cached: tests change these
// inside one process.
struct Cp4dEnv {
  bool mfma = true;           // CWT_CP4D_MFMA=0: the scalar forward kernel
  int roll = 2;               // CWT_CP4D_ROLL: 0 never, 1 the 10-output layers only, 2 also 10 -> 1
  int persist = 1;            // CWT_CP4D_PERSIST: 0 none, 1 the 10 -> 10 layer, 2 every layer (A/B)
  // CWT_CP4D_ORDER: the persistent forms' tile order (CmSched); 1 cuts the 10 -> 10 layer's L2 misses
  // 25 -> 15 M per launch at the same time
  int order = 1;
  int dbg = 0;                // CWT_CP4D_DBG: the persistent forms' timing study
  int rdbg = 0;               // CWT_CP4D_RDBG: the rolling window's timing study
  int wc = 30;                // CWT_CP4D_WC: a columns per rolling-window workgroup
  int pf = 2;                 // CWT_CP4D_PF=1: the rolling window's prefetch depth 1 instead of 2
  bool dgrad_scalar = false;  // CWT_DGRAD_SCALAR=1 (A/B only)
  bool wgrad_scalar = false;  // CWT_WGRAD_SCALAR=1 (A/B only)
};

inline Cp4dEnv cp4d_env() {
  Cp4dEnv e;
  const auto num = [](const char* name, int dflt) {
    const char* s = getenv(name);
    return s ? atoi(s) : dflt;
  };
  const auto is = [](const char* name, char c) {
    const char* s = getenv(name);
    return s && s[0] == c;
  };
  e.mfma = !is("CWT_CP4D_MFMA", '0');
  e.roll = num("CWT_CP4D_ROLL", 2);
  e.persist = num("CWT_CP4D_PERSIST", 1);
  e.order = num("CWT_CP4D_ORDER", 1);
  e.dbg = num("CWT_CP4D_DBG", 0);
  e.rdbg = num("CWT_CP4D_RDBG", 0);
  e.wc = num("CWT_CP4D_WC", 30);
  e.pf = num("CWT_CP4D_PF", 2) == 1 ? 1 : 2;
  e.dgrad_scalar = is("CWT_DGRAD_SCALAR", '1');
  e.wgrad_scalar = is("CWT_WGRAD_SCALAR", '1');
  return e;
}

// rc != 0: the shape is refused (CWT_EARG, msg) and nothing else is set.  cin / cout / mode / pf are
// the kernel's template arguments (cp4d_form_info's targs; for an input gradient cin is the
// gradient's channel count gin, cout the layer's input channels); gx, gy, gz the grid in workgroups
// of 256 threads.
struct Cp4dPlan {
  int rc = 0;
  const char* msg = nullptr;
  int form = CP4D_SCALAR;
  int cin = 0, cout = 0, mode = 0, pf = 0;
  int gx = 0, gy = 1, gz = 1;
  int wc = 0, nsa = 0;                // rolling window: a columns per workgroup, strips of RL_RA a rows
  int ntiles = 0, order = 0, dbg = 0; // persistent forms (dbg also the rolling window's)
  int G = 0, n = 0;                   // weight gradient: partials, floats per partial
};

inline int cp4d_cdiv(long a, long b) { return (int)((a + b - 1) / b); }
inline Cp4dPlan cp4d_refuse(const char* msg) {
  Cp4dPlan p;
  p.rc = CWT_EARG, p.msg = msg;
  return p;
}
// the widths with instantiated kernels (every form but the chunked ones)
inline bool cp4d_instantiated(int cin, int cout) {
  return (cout == 10 && (cin == 1 || cin == 2 || cin == 10)) || (cout == 1 && cin == 10);
}
// one workgroup per (tah x taw) a patch by (tbh x tbw) b patch and batch entry
inline void cp4d_tile_grid(Cp4dPlan& p, int B, int hA, int wA, int hB, int wB, int tah, int taw, int tbh, int tbw) {
  p.gx = cp4d_cdiv(hB, tbh) * cp4d_cdiv(wB, tbw), p.gy = cp4d_cdiv(hA, tah) * cp4d_cdiv(wA, taw), p.gz = B;
}
// The rolling window addresses a batch entry with 32-bit byte offsets and marks a skipped access
// with RL_OOR: it takes a shape only while every real offset (10 channels of 4 bytes) stays below
inline bool cp4d_roll_fits(int hA, int wA, int hB, int wB) { return (long)hA * wA * hB * wB * 10 * 4 <= RL_OOR; }
inline void cp4d_roll_grid(Cp4dPlan& p, int B, int hA, int wA, int hB, int wB, const Cp4dEnv& env) {
  p.wc = std::max(1, std::min(wA, env.wc));
  p.nsa = cp4d_cdiv(hA, RL_RA);
  p.pf = env.pf, p.dbg = env.rdbg;
  p.gx = cp4d_cdiv(hB, RL_BH) * cp4d_cdiv(wB, RL_BW), p.gy = cp4d_cdiv(wA, p.wc), p.gz = B * p.nsa;
}

// Forward.  variant (cwt_debug_cp4d_layer): 0 the automatic choice, 1 never the rolling window,
// 2 only it, 3 the chunked form.  cu, occ: the device's CUs and the persistent kernel's workgroups
// per CU (only the persistent forms' grid reads them).
inline Cp4dPlan cp4d_plan_fwd(int B, int hA, int wA, int hB, int wB, int cin, int cout, int variant,
                              const Cp4dEnv& env, int cu, int occ) {
  Cp4dPlan p;
  p.cin = cin, p.cout = cout;
  if (variant == 3 || (cin != 1 && cin != 2 && cin != 10)) {
    if (cout != 10 || cin < 1 || cin > CWT_MATCH_MAX_L || (variant != 0 && variant != 3))
      return cp4d_refuse("cp4d layer: the channel-chunked form takes 1..32 -> 10 channels");
    p.form = CP4D_NC_FWD;
    cp4d_tile_grid(p, B, hA, wA, hB, wB, CM_T, CM_T, CM_T, CM_T);
    return p;
  }
  const bool inst = cp4d_instantiated(cin, cout);
  const bool roll = variant == 2 || (variant == 0 && env.mfma && (env.roll == 2 || (env.roll == 1 && cout == 10)));
  if (roll && inst && cp4d_roll_fits(hA, wA, hB, wB)) {
    p.form = cout == 1 ? CP4D_ROLL_C1 : CP4D_ROLL;
    cp4d_roll_grid(p, B, hA, wA, hB, wB, env);
    return p;
  }
  if (variant == 2) return cp4d_refuse("cp4d layer: no rolling-window form for this shape");
  if (!inst) return cp4d_refuse("cp4d layer: channels (1|2 -> 10, 10 -> 10, 10 -> 1) only");
  if (!env.mfma) {
    cp4d_tile_grid(p, B, hA, wA, hB, wB, CP_TAH, CP_TAW, CP_TBH, CP_TBW);
    return p;
  }
  cp4d_tile_grid(p, B, hA, wA, hB, wB, CM_T, CM_T, CM_T, CM_T);
  if (env.persist == 2 || (env.persist == 1 && cin == 10 && cout == 10)) {
    p.form = cout == 1 ? CP4D_PERSIST_C1 : CP4D_PERSIST_MFMA;
    p.ntiles = p.gx * p.gy * p.gz;
    p.order = env.order, p.dbg = env.dbg;
    p.gx = std::max(1, std::min(p.ntiles, std::max(1, occ) * cu));  // a multiple of 8 when cu is
    p.gy = p.gz = 1;
    return p;
  }
  p.form = cout == 1 ? CP4D_TILE_C1 : CP4D_TILE_MFMA;
  return p;
}

// Input gradient of a layer with gout input and gin output channels (mode 1 of the forward's
// kernels: transposed, flipped filters).  variant as the forward's (cwt_debug_cp4d_dgrad).
inline Cp4dPlan cp4d_plan_dgrad(int B, int hA, int wA, int hB, int wB, int gin, int gout, int variant,
                                const Cp4dEnv& env, int cu, int occ) {
  (void)cu, (void)occ;  // no persistent input gradient
  Cp4dPlan p;
  p.cin = gin, p.cout = gout, p.mode = 1;
  if (variant == 3 || (gin == 10 && gout != 1 && gout != 2 && gout != 10)) {  // the L -> 10 first layer's
    if (gin != 10 || gout < 1 || gout > CWT_MATCH_MAX_L || (variant != 0 && variant != 3))
      return cp4d_refuse("cp4d input gradient: 10 -> 1..32 channels");
    p.form = CP4D_NC_DGRAD;
    cp4d_tile_grid(p, B, hA, wA, hB, wB, CM_T, CM_T, CM_T, CM_T);
    return p;
  }
  const bool mfma = gout == 10 && (gin == 1 || gin == 10);  // 10 output channels: the matrix-core forms
  const bool roll = variant == 2 || (variant == 0 && !env.dgrad_scalar && env.roll != 0);
  if (roll && mfma && cp4d_roll_fits(hA, wA, hB, wB)) {
    p.form = CP4D_ROLL;
    cp4d_roll_grid(p, B, hA, wA, hB, wB, env);
    return p;
  }
  if (variant == 2) return cp4d_refuse("cp4d input gradient: no rolling-window form for this shape");
  if (mfma && !env.dgrad_scalar) {
    p.form = CP4D_TILE_MFMA;
    cp4d_tile_grid(p, B, hA, wA, hB, wB, CM_T, CM_T, CM_T, CM_T);
    return p;
  }
  if (!((gin == 1 && gout == 10) || (gin == 10 && (gout == 10 || gout == 1 || gout == 2))))
    return cp4d_refuse("cp4d input gradient: channels (1 -> 10, 10 -> 10, 10 -> 1..32) only");
  cp4d_tile_grid(p, B, hA, wA, hB, wB, CP_TAH, CP_TAW, CP_TBH, CP_TBW);
  return p;
}

// Weight gradient: G workgroups stride over the tiles and write one partial of n floats each.
// No variant and no device fact changes it; the arguments are there so the three directions share
// a signature.  CWT_WGRAD_SCALAR=1 has no chunked form: a wide first layer is refused under it.
inline Cp4dPlan cp4d_plan_wgrad(int B, int hA, int wA, int hB, int wB, int cin, int cout, int variant,
                                const Cp4dEnv& env, int cu, int occ) {
  (void)variant, (void)cu, (void)occ;
  Cp4dPlan p;
  p.cin = cin, p.cout = cout;
  const bool inst = cp4d_instantiated(cin, cout);
  const bool chunked = cout == 10 && cin != 1 && cin != 2 && cin != 10;
  if (env.wgrad_scalar) {
    if (!inst) return cp4d_refuse("cp4d wgrad: channels (1|2 -> 10, 10 -> 10, 10 -> 1) only");
    p.form = CP4D_WGRAD_SCALAR;
  } else if (inst) {
    p.form = CP4D_WGRAD_MFMA;
  } else if (chunked && cin >= 1 && cin <= CWT_MATCH_MAX_L) {
    p.form = CP4D_NC_WGRAD;
  } else {
    return cp4d_refuse("cp4d wgrad: channels (1..32 -> 10, 10 -> 10, 10 -> 1) only");
  }
  // the chunked form walks the matrix-core kernels' 4 x 4 by 4 x 4 tiles: its grid is sized by their count
  const long ntiles = chunked ? (long)B * cp4d_cdiv(hA, CM_T) * cp4d_cdiv(wA, CM_T) * cp4d_cdiv(hB, CM_T) * cp4d_cdiv(wB, CM_T)
                              : (long)B * cp4d_cdiv(hA, WG_TAH) * cp4d_cdiv(wA, WG_TAW) * cp4d_cdiv(hB, WG_TBH) *
                                    cp4d_cdiv(wB, WG_TBW);
  p.G = (int)std::min<long>(chunked ? WG_G_NC : cin * cout >= 100 ? WG_G_WIDE : WG_G_THIN, ntiles);
  p.n = 18 * cin * cout + cout;
  p.gx = p.G, p.gy = chunked ? cp4d_cdiv(cin, NC_CK) : 1;
  return p;
}

// floats of the weight gradient's partial workspace: the largest G * n of any plan above (the
// 10 -> 10 layer, the thin layers at 2 -> 10, the chunked form at CWT_MATCH_MAX_L)
constexpr int cp4d_wgrad_part_floats() {
  return std::max(std::max(WG_G_WIDE * (18 * 10 * 10 + 10), WG_G_THIN * (18 * 2 * 10 + 10)),
                  WG_G_NC * (18 * CWT_MATCH_MAX_L * 10 + 10));
}
static_assert(cp4d_wgrad_part_floats() == 1477120, "the weight gradient's workspace (match_plan.h sizes it once)");

}  // namespace cwt
