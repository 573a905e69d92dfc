"""The float64 reference of the match head's backward with the tie rule written out, and the tie /
dead-position fixtures its tests share -- a helper, not a test.  Plain torch on the CPU; nothing here
runs device code, so the kernels are never their own reference.

The reference takes torch.max(corr4d, dim=..., keepdim=True) (src/model/match.py:42-43): under
autograd a maximum's gradient goes to ONE index, the first maximal one (torch.max(dim) on the CPU is
documented to return it).  oracle/match_oracle.mutual_matching restates the forward with amax, whose
backward splits the gradient evenly among tied positions: the two agree wherever no two entries of
a row or a column are equal, and nowhere else.  mutual_matching_first is the oracle's forward with
the reference's backward, in the closed form of csrc/match_bwd.hip's header comment.

mutual_matching_first   the autograd Function; corr_forward_ref the oracle's corr_forward with it
corr_forward_sided      the same chain with the ReLU units float64 cannot settle for fp32 open to the caller
normalize_fwd_bwd       token_norm_kernel / token_norm_bwd_kernel (F.normalize and its Jacobian)
readout_fwd_bwd         softmax(temp * corr2d) . v and its backward
support_masks_first     match.hip's support masks with first-index argmaxes
cp4d_wgrad_ref          the consensus layer's weight / bias gradients by autograd
dup_support / dup_query / dead_lines / chain_case / dead_chain_case / mask_corr
                        the fixtures of tests/test_gpu_match_ties.py; tests/test_match_ref_cpu.py
                        asserts on the CPU what those tests rely on (the ties separate first-index
                        from amax by > SEPARATION of max|gradient|, the dead rows exist, ...)
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import match_oracle as M

TOL_FWD = 2e-5      # the project's forward bar (tests/test_gpu_match.py)
TOL_MM = 1e-6       # MutualMatching's forward (tests/test_gpu_match.py::test_mutual_matching)
TOL_GRAD = 1e-4     # the project's gradient bar (tests/test_gpu_match_bwd.TOL)
SEPARATION = 1e-2   # what a tie fixture must put between the two tie rules: 100 x TOL_GRAD
PARAM_NAMES = [f"NeighConsensus.conv.{i}.{c}.{p}" for i in (0, 2, 4) for c in ("conv1", "conv2")
               for p in ("weight", "bias")]


def rel(a, b):
    """max|a - b| / max|b|, in float64 on the CPU (tests/test_gpu_match_bwd.rel)"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def rand(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g, dtype=torch.float64) * (hi - lo) + lo


# ---- MutualMatching with the reference's backward ----
class _MutualMatchingFirst(torch.autograd.Function):
    """m [B, C, NA, NB]: u[a] = max_b m + eps, v[b] = max_a m + eps, y = m (m / u) (m / v);
    dm = dy 3 m^2 / (u v) - [b = first argmax of row a] (sum_b dy y) / u[a]
                          - [a = first argmax of column b] (sum_a dy y) / v[b]."""

    @staticmethod
    def forward(ctx, m, eps):
        mu, iu = m.max(dim=3, keepdim=True)   # per query position a; the first maximal b
        mv, iv = m.max(dim=2, keepdim=True)   # per support position b; the first maximal a
        u, v = mu + eps, mv + eps
        y = m * ((m / u) * (m / v))
        ctx.save_for_backward(m, y, u, v, iu, iv)
        return y

    @staticmethod
    def backward(ctx, dy):
        m, y, u, v, iu, iv = ctx.saved_tensors
        dm = dy * (3.0 * m * m / (u * v))
        srow = (dy * y).sum(dim=3, keepdim=True)
        scol = (dy * y).sum(dim=2, keepdim=True)
        dm = dm - torch.zeros_like(m).scatter_(3, iu, srow / u)
        dm = dm - torch.zeros_like(m).scatter_(2, iv, scol / v)
        return dm, None


def mutual_matching_first(x: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """oracle.match_oracle.mutual_matching's forward (x [B, C, ha, wa, hb, wb]); the backward of
    torch.max(dim): each maximum's gradient to the first maximal index of its row / column."""
    B, C, ha, wa, hb, wb = x.shape
    return _MutualMatchingFirst.apply(x.reshape(B, C, ha * wa, hb * wb), eps).reshape(x.shape)


def corr_forward_ref(corr4d, v, layers, temp, symmetric=True):
    """oracle.match_oracle.corr_forward with mutual_matching_first in place of its mutual_matching:
    the oracle's own chain (NeighConsensus, reshape, softmax readout) run unchanged, the one name it
    looks up at call time bound to the first-index form for the duration of the call."""
    kept = M.mutual_matching
    M.mutual_matching = mutual_matching_first
    try:
        return M.corr_forward(corr4d, v, layers, temp, symmetric)
    finally:
        M.mutual_matching = kept


def corr_forward_sided(corr4d, v, layers, temp, symmetric=True, sides=None, info=None):
    """corr_forward_ref's chain put together from the oracle's layer (center_pivot_conv4d) with every ReLU
    written as pre * [pre > 0], so that a caller can settle the units float64 cannot settle for fp32.

    A ReLU's gradient jumps at 0.  A unit whose float64 pre-activation lies within the forward bar of 0
    (|pre| < TOL_FWD max|pre| of its layer -- the distance a correct fp32 layer may be off, the bar
    tests/test_gpu_cp4d_forms.py holds these kernels to) may land on either side in fp32, and the
    gradient of the function the device evaluated is the one of ITS side: at 285 positions a pass has
    6.5 M hidden units, a handful of them within 5e-8 of 0, and one such unit on the other side moves
    d_corr by 4e-3 of its maximum and the first two layers' weight gradients by 1e-3 (measured; the flip
    of that one unit in float64 reproduces the device's figures to every printed digit).  sides[branch]
    [layer] (bool [B, C, ha, wa, hb, wb]: the device's own ReLU output > 0) settles those units and no
    others; info receives, per ReLU, (units settled by sides, units OUTSIDE the margin where sides
    disagrees with float64 -- a correct forward has none).  sides None: corr_forward_ref, to rounding
    (tests/test_match_ref_cpu.py)."""
    B, L, h, w = corr4d.shape[:4]

    def swap(z):
        return z.permute(0, 1, 4, 5, 2, 3)

    def stack(z, side):
        for l, (w1, b1, w2, b2) in enumerate(layers):
            pre = M.center_pivot_conv4d(z, w1, b1, w2, b2)
            on = pre.detach() > 0
            if side is not None:
                near = pre.detach().abs() < TOL_FWD * pre.detach().abs().max()
                if info is not None:
                    info.append((int(near.sum()), int((on != side[l])[~near].sum())))
                on = torch.where(near, side[l], on)
            z = pre * on.to(pre.dtype)
        return z

    x = mutual_matching_first(corr4d)
    y = stack(x, sides[0] if sides is not None else None)
    if symmetric:   # match.py:75-80: the stack on the pair-swapped tensor, swapped back
        y = y + swap(stack(swap(x), [swap(s_) for s_ in sides[1]] if sides is not None else None))
    corr2d = mutual_matching_first(y).reshape(B, h * w, h * w)
    attn = torch.softmax(corr2d * temp, dim=-1)
    wv = torch.bmm(v.reshape(B, v.shape[1], h * w), attn.transpose(1, 2)).reshape(B, v.shape[1], h, w)
    return corr2d, wv


def mm_tie_terms(m, dy, eps=1e-5):
    """What the maxima send back, alone: dm - dy 3 m^2 / (u v) of the first-index rule, and the
    subtrahend dy 3 m^2 / (u v) itself (m, dy [B, C, NA, NB])."""
    u = m.amax(dim=3, keepdim=True) + eps
    v = m.amax(dim=2, keepdim=True) + eps
    direct = dy * (3.0 * m * m / (u * v))
    x = m.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(_MutualMatchingFirst.apply(x, eps), x, dy)
    return g - direct, direct


# ---- F.normalize, the readout, the support masks, the weight gradient ----
def normalize_fwd_bwd(x, dxn, eps):
    """token_norm_kernel / token_norm_bwd_kernel on rows x [T, C]: xn = x / max(|x|, eps);
    dx = (dxn - xn (xn . dxn)) / |x| where |x| > eps, dxn / eps elsewhere.  -> (xn, dx)
    (At |x| == eps exactly torch's clamp_min passes its gradient and the kernel's branch does not; no
    fp32 token lands on 1e-12 in practice, and no test here puts one there.)"""
    n = x.pow(2).sum(-1, keepdim=True).sqrt()
    xn = x / n.clamp_min(eps)
    s = (xn * dxn).sum(-1, keepdim=True)
    dx = torch.where(n > eps, (dxn - xn * s) / n.clamp_min(1e-300), dxn / eps)
    return xn, dx


def readout_fwd_bwd(corr2d, v, temp, d_wv):
    """corr2d [B, NA, NB], v [B, NB, Cv] tokens, d_wv [B, NA, Cv] the gradient at the weighted v:
    P = softmax(temp corr2d, -1), wv = P v; dP = d_wv v^T, d_corr2d = temp P (dP - sum_n P dP),
    d_v = P^T d_wv.  -> (P, wv, d_corr2d, d_v)"""
    z = temp * corr2d
    e = torch.exp(z - z.amax(-1, keepdim=True))
    P = e / e.sum(-1, keepdim=True)
    wv = torch.bmm(P, v)
    dP = torch.bmm(d_wv, v.transpose(1, 2))
    d_corr2d = temp * P * (dP - (P * dP).sum(-1, keepdim=True))
    return P, wv, d_corr2d, torch.bmm(P.transpose(1, 2), d_wv)


def support_masks_first(corr2d, ig, s_mask):
    """csrc/match.hip's support masks (ig constant 1e-4, then k2q / q2k by first-index argmax, the
    inconsistent columns shifted by -1000) -> (masked corr2d, inconsistent [B, NB] or None).
    oracle.match_oracle.support_masks takes its indices from max(dim)[1], the first on the CPU."""
    assert corr2d.device.type == "cpu"
    return M.support_masks(corr2d, ig, s_mask)


def cp4d_wgrad_ref(x, gm, shape):
    """x [B, NA, NB, cin], gm [B, NA, NB, cout] (float64), shape (B, hA, wA, hB, wB) -> dWa, dWb
    [cout][cin][3][3] and db [cout] of <gm, layer(x)>, by autograd through the layer without ReLU
    (tests/test_gpu_cp4d_forms.lin_layer) plus a bias."""
    from test_gpu_cp4d_forms import lin_layer
    cin, cout = x.shape[-1], gm.shape[-1]
    Wa = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, device=x.device, requires_grad=True)
    Wb = torch.zeros_like(Wa, requires_grad=True)
    b = torch.zeros(cout, dtype=torch.float64, device=x.device, requires_grad=True)
    return torch.autograd.grad(lin_layer(x, *shape, Wa, Wb) + b, (Wa, Wb, b), gm)


# ---- fixtures ----
def consensus_params(L, seed):
    """name -> float64 parameter of a NeighConsensus with CenterPivotConv4d layers L -> 10 -> 10 -> 1
    (nn.Conv2d's default bounds), the one-channel last layer's ReLU kept open as the gradient tests do"""
    g = torch.Generator().manual_seed(seed)
    sd, cin = {}, L
    for i, cout in zip((0, 2, 4), (10, 10, 1)):
        for c in ("conv1", "conv2"):
            bound = (9 * cin) ** -0.5
            sd[f"NeighConsensus.conv.{i}.{c}.weight"] = (torch.rand(cout, cin, 3, 3, generator=g, dtype=torch.float64) * 2 - 1) * bound
            sd[f"NeighConsensus.conv.{i}.{c}.bias"] = (torch.rand(cout, generator=g, dtype=torch.float64) * 2 - 1) * bound
        cin = cout
    # through float32: the values the device holds
    sd = {k: t.float().double() for k, t in sd.items()}
    sd["NeighConsensus.conv.4.conv1.bias"] += 0.2
    return {k: t.float().double() for k, t in sd.items()}


def dup_support(B, C, NA, NB, seed):
    """m [B, C, NA, NB]: columns j1 < j2 equal for every query row (two support positions with the
    same feature), and the maximum of every other row: those rows' argmax ties between j1 and j2.
    -> (m, tied rows, j1, j2)"""
    m = rand((B, C, NA, NB), seed, -0.2, 1.0)
    j1, j2 = 1, NB - 2
    rows = torch.arange(0, NA, 2)
    m[:, :, rows, j1] = 1.2 + 0.1 * rand((B, C, len(rows)), seed + 1)
    m[:, :, :, j2] = m[:, :, :, j1]
    return m.float().double(), rows, j1, j2


def dup_query(B, C, NA, NB, seed):
    """dup_support with the roles exchanged: rows a1 < a2 equal, the maximum of every other column"""
    m, cols, a1, a2 = dup_support(B, C, NB, NA, seed)
    return m.transpose(2, 3).contiguous(), cols, a1, a2


def dead_lines(B, C, NA, NB, seed):
    """m [B, C, NA, NB] with one whole row and one whole column exactly 0, the rest in [0, 1): the row's
    and the column's maxima are 0, so u = v = eps there, and every position of the row is maximal"""
    m = rand((B, C, NA, NB), seed)
    a0, b0 = NA // 2, 2
    m[:, :, a0, :] = 0.0
    m[:, :, :, b0] = 0.0
    return m.float().double(), a0, b0


def chain_case(kind, B, L, h, w, seed):
    """A corr_forward case on a tie fixture: corr4d [B, L, h, w, h, w] from dup_support / dup_query,
    v, the loss weights G1 (corr2d) and G2 (weighted v), the parameters.  Cv = 16."""
    make = dict(support=dup_support, query=dup_query)[kind]
    m = make(B, L, h * w, h * w, seed)[0]
    return dict(corr=m.reshape(B, L, h, w, h, w), v=rand((B, 16, h, w), seed + 2), G1=rand((B, h * w, h * w), seed + 3, -1, 1),
                G2=rand((B, 16, h, w), seed + 4, -1, 1), sd=consensus_params(L, seed + 5), temp=20.0, sym=True)


def chain_grads(case, forward):
    """forward = corr_forward_ref or oracle.match_oracle.corr_forward -> name -> float64 tensor:
    corr2d, wv, d_corr, d_v and the twelve parameter gradients of <G1, corr2d> + <G2, wv>"""
    sd = {k: t.clone().requires_grad_(True) for k, t in case["sd"].items()}
    c, v = case["corr"].clone().requires_grad_(True), case["v"].clone().requires_grad_(True)
    c2, wv = forward(c, v, M.layers_from_state(sd), case["temp"], case["sym"])
    ((c2 * case["G1"]).sum() + (wv * case["G2"]).sum()).backward()
    out = dict(corr2d=c2.detach(), wv=wv.detach(), d_corr=c.grad, d_v=v.grad)
    for n in PARAM_NAMES:
        out[n.replace("NeighConsensus.conv.", "")] = sd[n].grad
    return out


def consensus_out(case):
    """the NeighConsensus output y [B, hw, hw] of a chain case (what the second MutualMatching sees)"""
    B, L, h, w = case["corr"].shape[:4]
    y = M.neigh_consensus(M.mutual_matching(case["corr"]), M.layers_from_state(case["sd"]), case["sym"])
    return y.reshape(B, h * w, h * w)


DEAD_SHIFTS = [-0.05 * k for k in range(1, 41)]


def dead_chain_case(B, L, h, w, seed):
    """A tie-free chain case whose last consensus bias is lowered (in steps of 0.05, the first that
    does it) until some rows of y are all zero while y is not: the second MutualMatching then has
    u = eps on those rows and v = eps on the all-zero columns."""
    m = rand((B, L, h * w, h * w), seed, -0.2, 1.0).float().double()
    case = dict(corr=m.reshape(B, L, h, w, h, w), v=rand((B, 16, h, w), seed + 2), G1=rand((B, h * w, h * w), seed + 3, -1, 1),
                G2=rand((B, 16, h, w), seed + 4, -1, 1), sd=consensus_params(L, seed + 5), temp=20.0, sym=True)
    b0 = case["sd"]["NeighConsensus.conv.4.conv1.bias"].clone()
    for s in DEAD_SHIFTS:
        case["sd"]["NeighConsensus.conv.4.conv1.bias"] = (b0 + s).float().double()
        y = consensus_out(case)
        if int((y.amax(2) == 0).sum()) >= 2 and int((y > 0).sum()) >= 8:
            return case
    raise AssertionError("no bias shift leaves dead rows beside a live stack")


def mask_corr(NA, NB, seed):
    """corr2d [2, NA, NB], ig [2, NB] bool, s_mask [2, NB] int64: ig masks every support position of
    entry 0 (the whole entry becomes 1e-4: every argmax ties, index 0) and none of entry 1, whose
    columns 3 .. 6 each hold their maximum twice (rows 8 + j and 20 + j) and whose rows 0 .. 3 each
    hold theirs twice (columns 10 and NB - 1).  NA >= 27, NB >= 12."""
    c = rand((2, NA, NB), seed, -0.2, 1.0)
    for j in range(3, 7):
        c[1, 8 + j, j] = c[1, 20 + j, j] = 1.5 + 0.01 * j        # column maxima, twice
    for a in range(4):
        c[1, a, 10] = c[1, a, NB - 1] = 2.0 + 0.01 * a           # row maxima, twice
    ig = torch.zeros(2, NB, dtype=torch.bool)
    ig[0] = True
    g = torch.Generator().manual_seed(seed + 1)
    s_mask = (torch.rand(2, NB, generator=g) < 0.5).long()
    return c.float().double(), ig, s_mask
