// The host-side plan of MatchNet's match pass (api_match.hip): MutualMatching -> the three
// NeighConsensus layers in one or two branches -> the branches' sum -> MutualMatching -> the softmax
// readout (match.py:142-163), and of its backward.  One MatchPlan / MatchBwdPlan per call makes every
// decision of the call -- refusals, the form of each MutualMatching, the layer stack, the branches
// and their stream, where every tensor lives -- from the arguments and the environment's two knobs;
// match_params is the one table of the packed parameter vector and match_saved_layout the one
// layout of the activations the training forward keeps.  The executors, cwt_debug_match_plan and
// the tests all read them, and nothing else decides or computes an offset.  Decisions and tables,
// not a step list: the executors stay straight-line code.  Host only: no HIP call, includable from
// a plain C++ file.
#pragma once
#include <cstdlib>

#include "../../include/cwt.h"
#include "cp4d_plan.h"

namespace cwt {

// The environment's say in the plan.  Read once per call and never cached: tests change these
// inside one process.
struct MatchEnv {
  // CWT_MM_FUSE=1: the 2-channel correlation's transposition folded into the first MutualMatching's
  // passes, and the symmetric branches' sum into the second's (fewer passes over the 4-D map)
  bool fuse = false;
  // CWT_MATCH_BRANCH_STREAMS=0: the symmetric branches one after the other on the caller's stream
  bool two_streams = true;
};
inline MatchEnv match_env() {
  const auto is = [](const char* name, char c) {
    const char* s = getenv(name);
    return s && s[0] == c;
  };
  MatchEnv e;
  e.fuse = is("CWT_MM_FUSE", '1');
  e.two_streams = !is("CWT_MATCH_BRANCH_STREAMS", '0');
  return e;
}

// channels of the consensus stack: L -> 10 -> 10 -> 1
inline int match_ch(int L, int i) { return i == 0 ? L : i == 3 ? 1 : 10; }
inline long ld32(long n) { return (n + 31) & ~31L; }  // a row padded to whole 32-deep K tiles (gemm_f32d)

// The packed parameter vector (NeighConsensus.param_list's order), in float offsets.  'red' layers
// (CenterPivotConv4d): per layer conv1.weight [co][ci][3][3], conv1.bias [co], conv2.weight,
// conv2.bias -- slot 0 is conv1, slot 1 conv2.  'cv4' layers (Conv4d): per layer the one filter
// [3][co][ci][3][3][3] and its bias in slot 0 (slot 1: -1).  The gradient vector d_params has the
// same layout.
struct MatchParams {
  long W[3][2] = {}, b[3][2] = {};
  long nW[3] = {}, nb[3] = {};  // floats of one filter, of one bias
  long total = 0;
  // 'red': the filter and bias branch br applies over the query positions a and over the support
  // positions b.  Branch 0 is conv(x): conv1 over a, conv2 over b; branch 1 (symmetric mode) is
  // conv(x^T)^T = the same stack with the two roles exchanged (match.py:75-80).
  long Wa(int l, int br) const { return W[l][br]; }
  long ba(int l, int br) const { return b[l][br]; }
  long Wb(int l, int br) const { return W[l][1 - br]; }
  long bb(int l, int br) const { return b[l][1 - br]; }
};
inline MatchParams match_params(int L, bool cv4) {
  MatchParams p;
  long off = 0;
  for (int l = 0; l < 3; ++l) {
    p.nW[l] = (cv4 ? 81L : 9L) * match_ch(L, l) * match_ch(L, l + 1);
    p.nb[l] = match_ch(L, l + 1);
    for (int s = 0; s < 2; ++s) {
      const bool has = s == 0 || !cv4;
      p.W[l][s] = has ? off : -1;
      off += has ? p.nW[l] : 0;
      p.b[l][s] = has ? off : -1;
      off += has ? p.nb[l] : 0;
    }
  }
  p.total = off;
  return p;
}

// The activations the backward reads, carved from the caller's one `saved` buffer
// (cwt_match_corr_saved_floats), in float offsets (-1: not kept): x0 = MutualMatching(corr)
// channels-last [E][L], o[branch][layer] the ReLU outputs [E][10], [E][10], [E][1],
// y = o[0][2] + o[1][2] [E] (E = B NA NA), attn [B][NA][ld32(NA)].
struct MatchSavedLayout {
  long x0 = -1, o[2][3] = {{-1, -1, -1}, {-1, -1, -1}}, y = -1, attn = -1;
  long total = 0;
};
inline MatchSavedLayout match_saved_layout(int B, int L, long NA, bool symmetric, bool readout) {
  const long E = (long)B * NA * NA;
  MatchSavedLayout s;
  const auto take = [&](long n) {
    const long at = s.total;
    s.total += n;
    return at;
  };
  s.x0 = take(E * L);
  for (int br = 0; br < (symmetric ? 2 : 1); ++br)
    for (int l = 0; l < 3; ++l) s.o[br][l] = take(E * match_ch(L, l + 1));
  s.y = take(E);
  if (readout) s.attn = take((long)B * NA * ld32(NA));
  return s;
}

// One tensor of a pass: `floats` of the context's workspace named `ws`, or, ws == nullptr, at
// saved + off.  floats == 0: the pass has no such tensor.  per_cv: floats counts one value channel
// (the plan does not depend on Cv); the executor asks for Cv times as many.
struct MatchBuf {
  const char* ws = nullptr;
  long off = 0, floats = 0;
  bool per_cv = false;
};
inline MatchBuf match_in_ws(const char* name, long floats, bool per_cv = false) {
  MatchBuf b;
  b.ws = name, b.floats = floats, b.per_cv = per_cv;
  return b;
}
inline MatchBuf match_in_saved(long off, long floats) {
  MatchBuf b;
  b.off = off, b.floats = floats;
  return b;
}

enum MatchMm1 : int {
  MM1_DIRECT = 0,   // L == 1: MutualMatching straight from corr (channel-first is channels-last)
  MM1_PLANAR2 = 1,  // fuse, L == 2: launch_mutual_matching_planar2 reads the two planes as they lie
  MM1_CLAST = 2,    // otherwise: to channels-last, then MutualMatching in place
};
enum MatchMm2 : int {
  MM2_PLAIN = 0,  // one branch: MutualMatching of y
  MM2_ADD = 1,    // two branches: y += o[1][2], then MutualMatching of y
  MM2_SUM = 2,    // two branches, fuse, not training: launch_mutual_matching_sum(o[0][2], o[1][2])
};
constexpr const char* MATCH_MSG_ARGS = "bad arguments (in_channel 1 .. CWT_MATCH_MAX_L = 32)";

// rc != 0: the call is refused (CWT_EARG; the entry points report msg behind CWT_CHECK's
// "bad argument: ") and nothing else is set.
struct MatchPlan {
  int rc = 0;
  const char* msg = nullptr;
  int mm1 = MM1_DIRECT, mm2 = MM2_PLAIN;
  bool cv4 = false;    // the layer stack: launch_cv4d_layer (Conv4d), else launch_cp4d_layer
  int branches = 1;    // 2 in the symmetric mode
  bool fork = false;   // branch 1 on the context's aux stream, forked from and joined into the caller's
  bool train = false;  // the activations are kept in `saved`, y in a slot of its own (a copy of o[0][2])
  bool readout = false;
  MatchParams params;
  // x0: the first MutualMatching's output; o[branch][layer]: the layers' outputs; y: the second
  // MutualMatching's input (inference: o[0][2] itself); attn, vt: the readout's softmax and the
  // transposed, zero-padded v
  MatchBuf x0, o[2][3], y, attn, vt;
};
inline MatchPlan match_refuse(const char* msg) {
  MatchPlan p;
  p.rc = CWT_EARG, p.msg = msg;
  return p;
}

inline MatchPlan match_plan(int B, int L, int h, int w, bool symmetric, bool cv4, bool train, bool readout,
                            const MatchEnv& env) {
  if (B < 1 || L < 1 || L > CWT_MATCH_MAX_L || h < 1 || w < 1) return match_refuse(MATCH_MSG_ARGS);
  if (cv4 && L > 2)
    return match_refuse("Conv4d ('cv4') layers take in_channel 1 or 2 only (CenterPivotConv4d: up to 32)");
  if (train && cv4) return match_refuse("the training forward keeps CenterPivotConv4d ('red') activations only");
  MatchPlan p;
  p.mm1 = L == 1 ? MM1_DIRECT : env.fuse && L == 2 ? MM1_PLANAR2 : MM1_CLAST;
  p.cv4 = cv4, p.train = train, p.readout = readout;
  p.branches = symmetric ? 2 : 1;
  // the two branches are independent until their sum: one branch's store-bound layers overlap the
  // other's MFMA-bound ones.  The Conv4d stack runs both on the caller's stream.
  p.fork = symmetric && env.two_streams && !cv4;
  p.mm2 = !symmetric ? MM2_PLAIN : env.fuse && !train ? MM2_SUM : MM2_ADD;
  p.params = match_params(L, cv4);
  const long NA = (long)h * w, E = (long)B * NA * NA, attn = (long)B * NA * ld32(NA);
  if (train) {
    const MatchSavedLayout s = match_saved_layout(B, L, NA, symmetric, readout);
    p.x0 = match_in_saved(s.x0, E * L);
    for (int br = 0; br < p.branches; ++br)
      for (int l = 0; l < 3; ++l) p.o[br][l] = match_in_saved(s.o[br][l], E * match_ch(L, l + 1));
    p.y = match_in_saved(s.y, E);
    if (readout) p.attn = match_in_saved(s.attn, attn);
  } else {
    // branch 1 has intermediate buffers of its own only where it runs beside branch 0
    static const char* const names[2][2][3] = {{{"match.x1", "match.x2", "match.y1"}, {"match.x1", "match.x2", "match.y2"}},
                                               {{"match.x1", "match.x2", "match.y1"}, {"match.x1b", "match.x2b", "match.y2"}}};
    p.x0 = match_in_ws("match.x0", E * L);
    for (int br = 0; br < p.branches; ++br)
      for (int l = 0; l < 3; ++l) p.o[br][l] = match_in_ws(names[p.fork][br][l], E * match_ch(L, l + 1));
    p.y = p.o[0][2];
    if (readout) p.attn = match_in_ws("match.attn", attn);
  }
  if (readout) p.vt = match_in_ws("match.vt", (long)B * ld32(NA), true);
  return p;
}

// The backward of the training forward ('red' layers): the gradients wanted, the saved
// activations' offsets, and the executor's workspaces.  (The readout backward's own scratch --
// mb.dA, mb.PT, mb.dwvT -- belongs to match_readout_bwd, which cwt_match_readout_backward also runs.)
struct MatchBwdPlan {
  int rc = 0;
  const char* msg = nullptr;
  int branches = 1;
  bool d_corr = false, d_v = false;
  bool readout = false;  // d_weighted_v given: the softmax readout's gradient joins the caller's at corr2d
  bool clast = false;    // L > 1: the first MutualMatching's backward through the channels-last round trip
  MatchParams params;
  MatchSavedLayout saved;
  // g2d: the gradient at corr2d; dy: at y; gA: at a layer's input; gm: through a layer's ReLU;
  // dx0: at x0 (both branches' sum); part: the weight gradient's partials; xcl, dxcl: corr and its
  // gradient channels-last
  MatchBuf g2d, dy, gA, gm, dx0, part, xcl, dxcl;
};

inline MatchBwdPlan match_bwd_plan(int B, int L, int h, int w, bool symmetric, bool d_corr, bool d_v, bool readout) {
  MatchBwdPlan p;
  if (B < 1 || L < 1 || L > CWT_MATCH_MAX_L || h < 1 || w < 1) {
    p.rc = CWT_EARG, p.msg = MATCH_MSG_ARGS;
    return p;
  }
  p.branches = symmetric ? 2 : 1;
  p.d_corr = d_corr, p.d_v = d_v, p.readout = readout;
  p.clast = L > 1;
  p.params = match_params(L, false);
  const long NA = (long)h * w, E = (long)B * NA * NA;
  p.saved = match_saved_layout(B, L, NA, symmetric, readout);
  p.g2d = match_in_ws("mb.g2d", E);
  p.dy = match_in_ws("mb.dy", E);
  p.gA = match_in_ws("mb.gA", E * 10);
  p.gm = match_in_ws("mb.gm", E * 10);
  p.dx0 = match_in_ws("mb.dx0", E * L);
  p.part = match_in_ws("mb.part", cp4d_wgrad_part_floats());
  if (d_corr && p.clast) {
    p.xcl = match_in_ws("mb.xcl", E * L);
    p.dxcl = match_in_ws("mb.dxcl", E * L);
  }
  return p;
}

}  // namespace cwt
