"""tests/match_ref.py on the CPU: what tests/test_gpu_match_big.py and test_gpu_match_ties.py rely on,
asserted without a device.

Off ties, mutual_matching_first's hand-written backward is autograd's (1e-12 against the oracle's amax
chain); on every tie fixture the first-index gradient and the amax gradient differ by more than
match_ref.SEPARATION = 1e-2 of max|gradient|, 100 times the bar the device is held to, so a device
that split a tied maximum's gradient -- or sent it to the last index -- could not pass; the dead
chain case has all-zero rows beside live ones, with a margin the fp32 rounding cannot cross."""
import pytest
import torch
import torch.nn.functional as F

import match_ref as R
from oracle import match_oracle as M


@pytest.mark.parametrize("L,sym", [(1, True), (1, False), (3, True), (3, False)])
def test_first_index_backward_is_autograd_off_ties(L, sym):
    B, h, w = 2, 5, 6
    case = dict(corr=R.rand((B, L, h, w, h, w), 7 + L, -0.2, 1.0), v=R.rand((B, 16, h, w), 8),
                G1=R.rand((B, h * w, h * w), 9, -1, 1), G2=R.rand((B, 16, h, w), 10, -1, 1),
                sd=R.consensus_params(L, 11 + L), temp=20.0, sym=sym)
    a, b = R.chain_grads(case, R.corr_forward_ref), R.chain_grads(case, M.corr_forward)
    assert float(b["d_corr"].abs().max()) > 0 and float(b["4.conv2.bias"].abs().max()) > 0
    for k in a:
        assert R.rel(a[k], b[k]) < 1e-12, (k, R.rel(a[k], b[k]))
    assert M.mutual_matching is not R.mutual_matching_first   # the oracle's name is put back


@pytest.mark.parametrize("L,sym", [(2, True), (3, False)])
def test_sided_chain_is_the_reference_chain(L, sym):
    """corr_forward_sided without sides, and with float64's own sides, is corr_forward_ref; with one near
    unit put on the other side its gradients move and its outputs do not"""
    import functools
    B, h, w = 2, 5, 6
    case = dict(corr=R.rand((B, L, h, w, h, w), 7 + L, -0.2, 1.0), v=R.rand((B, 16, h, w), 8),
                G1=R.rand((B, h * w, h * w), 9, -1, 1), G2=R.rand((B, 16, h, w), 10, -1, 1),
                sd=R.consensus_params(L, 11 + L), temp=20.0, sym=sym)
    a = R.chain_grads(case, R.corr_forward_ref)
    b = R.chain_grads(case, R.corr_forward_sided)
    for k in a:
        assert R.rel(b[k], a[k]) < 1e-12, k
    # float64's own decisions as sides: nothing changes, nothing disagrees
    layers = M.layers_from_state(case["sd"])
    x = M.mutual_matching(case["corr"])
    sides = []
    for br in range(2 if sym else 1):
        z, row = x if br == 0 else x.permute(0, 1, 4, 5, 2, 3), []
        for lay in layers:
            z = torch.relu(M.center_pivot_conv4d(z, *lay))
            row.append((z if br == 0 else z.permute(0, 1, 4, 5, 2, 3)) > 0)
        sides.append(row)
    info = []
    c = R.chain_grads(case, functools.partial(R.corr_forward_sided, sides=sides, info=info))
    assert len(info) == 3 * len(sides) and all(bad == 0 for _, bad in info), info
    for k in a:
        assert R.rel(c[k], a[k]) < 1e-12, k
    # every near unit on the other side: the outputs stay within the forward bar, the gradients do not
    flipped = [[~s for s in row] for row in sides]
    info = []
    d = R.chain_grads(case, functools.partial(R.corr_forward_sided, sides=flipped, info=info))
    assert all(bad > 0 for _, bad in info)     # and the disagreement outside the margin is counted
    assert sum(n for n, _ in info) > 0
    assert R.rel(d["corr2d"], a["corr2d"]) < 1e-3 and R.rel(d["d_corr"], a["d_corr"]) > 1e-4


def _mm_grads(m, dy):
    out = []
    for f in (R.mutual_matching_first, M.mutual_matching):
        x = m.clone().requires_grad_(True)
        B, C, NA, NB = m.shape
        (g,) = torch.autograd.grad(f(x.reshape(B, C, NA, 1, NB, 1)), x, dy.reshape(B, C, NA, 1, NB, 1))
        out.append(g)
    return out


@pytest.mark.parametrize("kind", ["support", "query"])
@pytest.mark.parametrize("C", [1, 2, 3])
def test_direct_tie_fixtures_separate_the_rules(kind, C):
    NA, NB = (42, 42) if kind == "support" else (25, 25)
    m, lines, i1, i2 = (R.dup_support if kind == "support" else R.dup_query)(2, C, NA, NB, 31 + C)
    dy = R.rand(m.shape, 41 + C, -1, 1)
    mt = m if kind == "support" else m.transpose(2, 3)
    assert torch.equal(mt[..., i1], mt[..., i2]) and i1 < i2
    tied = (mt.amax(3) == mt[..., i1])
    assert 3 * int(tied.sum()) >= tied.numel()           # i1 holds the maximum of at least a third of the lines
    first, amax = _mm_grads(m, dy)
    sep = float((first - amax).abs().max() / first.abs().max())
    print(f"dup_{kind} C={C}: first-index vs amax gradient {sep:.2e} of max|gradient|")
    assert sep > R.SEPARATION
    # the tied maxima's gradient lands on i1 and not on i2 (the rows that are no column argmax besides)
    tie, _ = R.mm_tie_terms(m, dy)
    tt = tie if kind == "support" else tie.transpose(2, 3)
    mass1, mass2 = _tie_mass(tt, mt, lines, i1, i2)
    assert mass2 == 0.0 and mass1 > 0.0


def _tie_mass(tt, mt, lines, i1, i2):
    """sum |tie term| at (line, i1) and at (line, i2) over the tied lines that are not the cross
    direction's argmax of i1 / i2 (there the other maximum's own term lands)"""
    cross = mt[..., i1].argmax(dim=2)                      # per (b, c): the line holding i1's (= i2's) cross maximum
    keep = torch.ones(mt.shape[:3], dtype=torch.bool)
    keep.scatter_(2, cross.unsqueeze(2), False)
    sel = torch.zeros_like(keep)
    sel[:, :, lines] = True
    sel &= keep
    return float(tt[..., i1][sel].abs().sum()), float(tt[..., i2][sel].abs().sum())


@pytest.mark.parametrize("kind,B,L,h,w", [("support", 2, 1, 6, 7), ("support", 2, 2, 6, 7), ("query", 2, 1, 5, 5),
                                          ("query", 2, 2, 5, 5)])
def test_chain_tie_fixtures_separate_the_rules(kind, B, L, h, w):
    case = R.chain_case(kind, B, L, h, w, 50 + L)
    a, b = R.chain_grads(case, R.corr_forward_ref), R.chain_grads(case, M.corr_forward)
    sep = float((a["d_corr"] - b["d_corr"]).abs().max() / a["d_corr"].abs().max())
    print(f"chain dup_{kind} L={L}: first-index vs amax d_corr {sep:.2e} of max|gradient|")
    assert sep > R.SEPARATION
    for k in a:   # the ties sit in the first MutualMatching alone: nothing else moves
        if k != "d_corr":
            assert R.rel(a[k], b[k]) < 1e-12, k


def test_dead_lines_are_finite_and_tie_free_in_effect():
    m, a0, b0 = R.dead_lines(2, 3, 42, 42, 61)
    assert float(m[:, :, a0].abs().max()) == 0 and float(m[:, :, :, b0].abs().max()) == 0
    dy = R.rand(m.shape, 62, -1, 1)
    first, amax = _mm_grads(m, dy)
    assert torch.isfinite(first).all() and float(first.abs().max()) > 0
    # an all-zero line's y is zero, so its maximum sends nothing back under either rule
    assert R.rel(first, amax) < 1e-12


def test_dead_chain_case_has_dead_rows_with_margin():
    case = R.dead_chain_case(2, 1, 6, 7, 71)
    y = R.consensus_out(case)
    dead_rows, live = int((y.amax(2) == 0).sum()), int((y > 0).sum())
    print(f"dead chain: {dead_rows} all-zero rows of {y.shape[0] * y.shape[1]}, {live} live entries")
    assert dead_rows >= 2 and live >= 8
    # no last-layer pre-activation within 1e-5 of the ReLU's edge: fp32 rounding (1e-6 at most) flips none
    b = case["sd"]["NeighConsensus.conv.4.conv1.bias"]
    for d in (-1e-5, 1e-5):
        c2 = dict(case, sd=dict(case["sd"], **{"NeighConsensus.conv.4.conv1.bias": b + d}))
        assert torch.equal(R.consensus_out(c2) > 0, y > 0), d
    g = R.chain_grads(case, R.corr_forward_ref)
    assert all(torch.isfinite(t).all() for t in g.values())
    assert float(g["d_corr"].abs().max()) > 0 and float(g["0.conv1.weight"].abs().max()) > 0


def test_normalize_fwd_bwd_is_autograd_of_normalize():
    eps = 1e-12
    x = R.rand((6, 8), 81, -1, 1)
    x[1] = 0.0                      # zero norm
    x[2] = 0.0
    x[2, 3] = 1e-20                 # below eps
    x[3] *= 1e-11                   # just above eps
    x[4] *= 1e-13                   # just below
    dxn = R.rand((6, 8), 82, -1, 1)
    xa = x.clone().requires_grad_(True)
    xn_a = F.normalize(xa, dim=-1, eps=eps)
    (dx_a,) = torch.autograd.grad(xn_a, xa, dxn)
    xn, dx = R.normalize_fwd_bwd(x, dxn, eps)
    assert torch.equal(xn, xn_a.detach())
    for r in range(6):
        assert R.rel(dx[r], dx_a[r]) < 1e-12, r
    assert torch.equal(dx[1], dxn[1] / eps) and torch.equal(dx[2], dxn[2] / eps)


def test_readout_fwd_bwd_is_autograd():
    c, v, d = R.rand((2, 9, 11), 91, -0.2, 1.0), R.rand((2, 11, 4), 92, -1, 1), R.rand((2, 9, 4), 93, -1, 1)
    ca, va = c.clone().requires_grad_(True), v.clone().requires_grad_(True)
    wv_a = torch.bmm(torch.softmax(20.0 * ca, -1), va)
    dc_a, dv_a = torch.autograd.grad(wv_a, (ca, va), d)
    P, wv, dc, dv = R.readout_fwd_bwd(c, v, 20.0, d)
    assert R.rel(wv, wv_a) < 1e-12 and R.rel(dc, dc_a) < 1e-12 and R.rel(dv, dv_a) < 1e-12
    assert R.rel(P.sum(-1), torch.ones(2, 9, dtype=torch.float64)) < 1e-12


def test_support_masks_first_on_ties():
    NA = NB = 42
    c, ig, sm = R.mask_corr(NA, NB, 101)
    out, inc = R.support_masks_first(c, ig, sm)
    # entry 0: every support position masked, the whole entry 1e-4, every argmax index 0
    assert torch.equal(out[0], torch.full((NA, NB), 1e-4, dtype=torch.float64) + inc[0].unsqueeze(0) * -1000.0)
    assert torch.equal(inc[0], (sm[0] != sm[0, 0]).double())   # q2k[k2q[j]] = q2k[0] = 0 for every j
    # entry 1: the doubled maxima resolve to their first position
    masked = c[1]
    k2q, q2k = masked.max(0)[1], masked.max(1)[1]
    for j in range(3, 7):
        assert masked[8 + j, j] == masked[20 + j, j] == masked[:, j].max() and int(k2q[j]) == 8 + j
    for a in range(4):
        assert masked[a, 10] == masked[a, NB - 1] == masked[a].max() and int(q2k[a]) == 10
    want = (sm[1] != sm[1][q2k[k2q]]).double()
    assert torch.equal(inc[1], want)
    # the rule matters here: with last-index argmaxes the mask is another one
    k2q_l = NA - 1 - masked.flip(0).max(0)[1]
    q2k_l = NB - 1 - masked.flip(1).max(1)[1]
    assert not torch.equal((sm[1] != sm[1][q2k_l[k2q_l]]).double(), want)
