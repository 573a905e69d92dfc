// The host-side plan of the inner adaptation loop (adapt.hip): which launch a geometry takes -- the
// per-step launches or one of the persistent forms -- and that launch's grid.  One value, computed
// once per API call by adapt_plan() from the geometry, the CU count and the environment's knobs;
// the launcher, the profile-record names, the fused-tail decision and the workgroup count the
// pipeline asks for all read it.  Host only: no HIP call, includable from a plain C++ file.
#pragma once
#include <algorithm>
#include <cstdlib>

namespace cwt {

constexpr int PA_UC = 31;        // max lo-res columns owned per unit (the plan's uc: 31, or 15 on request)
constexpr int PA_R_DEFAULT = 8;  // replica rows used (CWT_ADAPT_PR: 2, 4, 8 or 16)
constexpr int PA_EW = 4;         // episodes one workgroup's units may span, at most

// A unit is one lo-res row pair x up to uc columns of one support image; a persistent workgroup
// (1,024 threads, one per CU, resident for the whole loop) holds a contiguous range of k units.
// The forms differ in where those units' f lives.  The values are the kernels' NRES template
// argument and so part of the kernel names the profiles carry: they do not change.
enum AdaptForm : int {
  PA_STEPS = -1,  // no persistent form: one launch per step (adapt_step_kernel)
  // k units streamed from L2 into registers every step.  Not faster than the step launches:
  // only with CWT_ADAPT_PERSIST=2
  PA_REG_STREAM = 0,
  // k = 1: the unit's f in registers
  PA_ONE = 1,
  // k = 2 in lockstep (one set of LDS barriers, one butterfly and one set of atomics per step
  // when both units belong to one episode), the first unit in registers, the second in LDS
  // (128 KB, lane-major: conflict-free).  CWT_ADAPT_BREG=0 selects it over PA_PAIR_REG
  PA_PAIR_LDS = 2,
  // k >= 4 (5-shot 641^2: 1200 units, 4-5 per workgroup): units streamed every step, each wave's
  // slice by LDS-DMA into its private 8 KB while the previous unit is computed; 6.04 against
  // 6.35 ms for the step launches.  At k = 3 (5-shot 473^2) the stream is slower than the step
  // launches (4.09 against 3.53 ms: the 37 MB per step of f come from the Infinity Cache and
  // the 3-unit workgroups set the pace).  CWT_ADAPT_STREAM=0 disables it, =1 allows it from k = 3
  PA_LDS_STREAM = 3,
  // k = 3 in lockstep (5-shot 473^2: 590 units on 197 workgroups), the first and third unit in
  // registers, the second in LDS; CWT_ADAPT_LOCK3=0 returns it to the step launches.  As few
  // workgroups as three units each take (197, not 256 with two or three each -- the step waits
  // for the three-unit ones either way, and fewer workgroups make the barrier cheaper and leave
  // CUs free)
  PA_LOCK3 = 4,
  // k = 2 in lockstep, both units in registers (the second as PA_LOCK3's third): no LDS reads of f
  // in the z and dW passes.  The form EpisodePipeline's adapt context runs, and the only one the
  // episode tail fuses behind (adapt_persist_tail_kernel)
  PA_PAIR_REG = 5,
  // PA_LDS_STREAM with the workgroup's first unit resident in registers: its f is never streamed,
  // the DMA ring carries only the units after it (about a fifth of the per-step stream at 5-shot
  // 641^2).  Opt in with CWT_ADAPT_RES1=1 -- measured slower (5-shot 641^2 alone: 6.77 against
  // 5.87 ms; the resident f does not fit beside the streamed unit at 1,024 threads and 25 VGPRs
  // spill to scratch, whose per-step reloads cost more than the fifth of the stream they save;
  // profiles/r4/run_n)
  PA_LDS_STREAM_RES1 = 6,
};
constexpr int PA_NFORMS = 7;

// What the kernel body (adapt_persist_body) and the planner need to know of a form; the body's
// constexpr flags and the planner's span bound are both read from here.
struct PaFormTraits {
  int nu;       // units a workgroup runs in lockstep
  int ewk;      // episodes a workgroup's units may span (the body's per-episode W copies)
  bool lock;    // lockstep with the second unit's f in LDS
  bool breg;    // lockstep pair, both in registers
  bool stream;  // units streamed through LDS every step
  bool res1;    // ... with the first one resident
};
constexpr PaFormTraits pa_form_traits(int form) {
  switch (form) {
    case PA_ONE: return {1, 1, false, false, false, false};
    case PA_PAIR_LDS: return {2, 2, true, false, false, false};
    case PA_LDS_STREAM: return {1, 2, false, false, true, false};
    case PA_LOCK3: return {3, 2, true, false, false, false};
    case PA_PAIR_REG: return {2, 2, false, true, false, false};
    case PA_LDS_STREAM_RES1: return {1, 2, false, false, true, true};
    default: return {1, PA_EW, false, false, false, false};  // PA_REG_STREAM
  }
}

// The environment's say in the plan.  Read once per API call and never cached: tests and bench.py
// change these inside one process.
struct AdaptKnobs {
  int persist = 1;      // CWT_ADAPT_PERSIST: 0 the step launches always, 2 also admits PA_REG_STREAM
  int uc = PA_UC;       // CWT_ADAPT_UC: 15 or 31 owned columns.  15 halves each workgroup's hi-res pixels
                        // but doubles the workgroups, and the barrier's atomics and arrivals cost more than
                        // that saves (1-shot 473: 7.0 vs 5.9 us per step, tools/persist_stamps.py)
  int upw = 0;          // CWT_ADAPT_UPW: units per workgroup aimed at, 1 or 2 (0: unset)
  int stream_from = 4;  // CWT_ADAPT_STREAM: the k from which PA_LDS_STREAM is taken (=0: never, =1: 3)
  bool lock3 = true;    // CWT_ADAPT_LOCK3
  bool breg = true;     // CWT_ADAPT_BREG
  bool res1 = false;    // CWT_ADAPT_RES1
  int nrep = PA_R_DEFAULT;  // CWT_ADAPT_PR
  int dbg = 0;          // CWT_ADAPT_DBG (the study bits; the step engine reads its own)
  // the kernel instantiation: 1 stamps (timing study, & 32), 2 latency floor (& 64), 3 side leg (& 128), 0 product
  int mode() const { return (dbg & 32) ? 1 : (dbg & 64) ? 2 : (dbg & 128) ? 3 : 0; }
};

inline AdaptKnobs adapt_knobs_from_env() {
  AdaptKnobs kn;
  const auto is = [](const char* s, char c) { return s && s[0] == c; };
  const char* pe = getenv("CWT_ADAPT_PERSIST");
  kn.persist = is(pe, '0') ? 0 : is(pe, '2') ? 2 : 1;
  const char* ucs = getenv("CWT_ADAPT_UC");
  if (ucs && (atoi(ucs) == 15 || atoi(ucs) == 31)) kn.uc = atoi(ucs);
  const char* upws = getenv("CWT_ADAPT_UPW");
  kn.upw = upws ? (atoi(upws) == 1 ? 1 : 2) : 0;
  const char* sts = getenv("CWT_ADAPT_STREAM");
  kn.stream_from = sts ? (sts[0] == '0' ? 1 << 30 : 3) : 4;
  kn.lock3 = !is(getenv("CWT_ADAPT_LOCK3"), '0');
  kn.breg = !is(getenv("CWT_ADAPT_BREG"), '0');
  kn.res1 = is(getenv("CWT_ADAPT_RES1"), '1');
  const char* pr = getenv("CWT_ADAPT_PR");
  kn.nrep = pr ? atoi(pr) : PA_R_DEFAULT;
  if (kn.nrep != 2 && kn.nrep != 4 && kn.nrep != 8 && kn.nrep != 16) kn.nrep = PA_R_DEFAULT;
  const char* dbg = getenv("CWT_ADAPT_DBG");
  kn.dbg = dbg ? atoi(dbg) : 0;
  return kn;
}

// persist == false: the per-step launches, and the grid fields are zero (those launches take none
// of them).  Otherwise G workgroups share units = E * n * (h - 1) * ncb units of uc columns, at
// most k each, a workgroup's range touching at most span episodes.
struct AdaptPlan {
  bool persist = false;
  int form = PA_STEPS, G = 0, units = 0, ncb = 0, uc = 0;
  int nrep = PA_R_DEFAULT, mode = 0;  // replica rows, kernel instantiation (AdaptKnobs::mode)
  long k = 0, span = 0;
  int E = 0, n = 0, h = 0, w = 0, iters = 0;  // the call it was made for
};

// upw_pref: the context's units per workgroup (cwt_ctx_set_adapt_units: EpisodePipeline asks for 2;
// 0 none); cu_count: the device's CUs -- the persistent loop needs all G workgroups co-resident.
inline AdaptPlan adapt_plan(int E, int n, int h, int w, int iters, int upw_pref, int cu_count, const AdaptKnobs& kn) {
  AdaptPlan p;
  p.nrep = kn.nrep;
  p.mode = kn.mode();
  p.E = E, p.n = n, p.h = h, p.w = w, p.iters = iters;
  if (iters <= 0 || kn.persist == 0 || cu_count <= 0) return p;
  const int ncb = (w - 1 + kn.uc - 1) / kn.uc;
  const int ntile = (h - 1) * ncb;
  const long units = (long)E * n * ntile;
  // units per workgroup: 1, or 2 (half the workgroups, and CUs left for a concurrent extractor
  // pass).  The context's choice, else CWT_ADAPT_UPW, else 1 while that takes at most half the
  // CUs (1-shot 473^2: 118 workgroups) and 2 beyond
  const int upw = upw_pref ? upw_pref : kn.upw ? kn.upw : (units <= cu_count / 2 ? 1 : 2);
  int G = (int)std::min<long>((units + upw - 1) / upw, cu_count);
  const long k = (units + G - 1) / G;
  const long per_ep = (long)n * ntile;
  const long span = (k - 1 + per_ep - 1) / per_ep + 1;
  int form = k == 1                               ? PA_ONE
             : (k == 2 && span <= 2)              ? (kn.breg ? PA_PAIR_REG : PA_PAIR_LDS)
             : (k == 3 && span <= 2 && kn.lock3)  ? PA_LOCK3
             : (k >= kn.stream_from && span <= 2) ? (kn.res1 ? PA_LDS_STREAM_RES1 : PA_LDS_STREAM)
                                                  : PA_REG_STREAM;
  if (span > pa_form_traits(form).ewk) return p;
  if (form == PA_REG_STREAM && kn.persist != 2) return p;
  if (form == PA_LOCK3) G = (int)((units + 2) / 3);
  p.persist = true;
  p.form = form, p.G = G, p.units = (int)units, p.ncb = ncb, p.uc = kn.uc;
  p.k = k, p.span = span;
  return p;
}

// The inner-loop kernel of a plan as the profile records name it: "adapt_persist_kernel<NRES" or
// "adapt_step_kernel<"
inline const char* adapt_plan_kernel_name(const AdaptPlan& p) {
  static const char* names[PA_NFORMS] = {"adapt_persist_kernel<0", "adapt_persist_kernel<1", "adapt_persist_kernel<2",
                                         "adapt_persist_kernel<3", "adapt_persist_kernel<4", "adapt_persist_kernel<5",
                                         "adapt_persist_kernel<6"};
  return p.persist && p.form >= 0 && p.form < PA_NFORMS ? names[p.form] : "adapt_step_kernel<";
}

}  // namespace cwt
