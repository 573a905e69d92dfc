"""The match head at ties and dead positions, against tests/match_ref.py (float64, first-index maxima).

The reference takes torch.max(dim) (src/model/match.py:42-43): a tied maximum's gradient goes to the
first maximal index, which is what csrc/match_bwd.hip's argmax_merge and csrc/match.hip's cycle-mask
argmaxes implement -- and what no other test exercises, their inputs being continuous random data.
The fixtures are match_ref's, small enough (6 x 7, 5 x 5) that every tie is placed by hand;
tests/test_match_ref_cpu.py asserts on the CPU that on each of them the first-index gradient and the
even split of amax differ by more than 1e-2 of max|gradient|, 100 times the 1e-4 bar held here.

Bars, the project's own: 2e-5 forward, 1e-4 gradients, the masks exact."""

import pytest
import torch

import match_ref as R
from few_shot_seg_cwt_amd import _lib
from oracle import match_oracle as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def mm_bwd(dev, m, dy):
    """cwt_debug_mutual_matching_bwd on m, dy [B, C, NA, NB] (float64, fp32-exact) -> dx of that shape"""
    B, Cc, NA, NB = m.shape
    xd = m.permute(0, 2, 3, 1).contiguous().float().to(dev)
    dyd = dy.permute(0, 2, 3, 1).contiguous().float().to(dev)
    dx = torch.full_like(xd, float("nan"))
    _lib.check(_lib.lib().cwt_debug_mutual_matching_bwd(_lib.ctx(dev.index), _lib.ptr(xd), _lib.ptr(dyd), B, NA, NB, Cc,
                                                        _lib.ptr(dx), _lib.stream_ptr(dev)),
               "cwt_debug_mutual_matching_bwd")
    return dx.permute(0, 3, 1, 2).double().cpu()


def mm_ref(m, dy):
    B, Cc, NA, NB = m.shape
    x = m.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(R.mutual_matching_first(x.reshape(B, Cc, NA, 1, NB, 1)), x, dy.reshape(B, Cc, NA, 1, NB, 1))
    return g


@pytest.mark.parametrize("kind", ["support", "query"])
@pytest.mark.parametrize("Cc", [1, 2, 3])
def test_mutual_matching_backward_duplicated_positions(dev, kind, Cc):
    """Two equal columns (two support positions with one feature) / two equal rows, holding the maximum of
    every other row / column: the gradient of those maxima lands on the first of the pair, none on the second."""
    NA, NB = (42, 42) if kind == "support" else (25, 25)
    m, lines, i1, i2 = (R.dup_support if kind == "support" else R.dup_query)(2, Cc, NA, NB, 31 + Cc)
    dy = R.rand(m.shape, 41 + Cc, -1, 1).float().double()
    ref = mm_ref(m, dy)
    dx = mm_bwd(dev, m, dy)
    e = R.rel(dx, ref)
    # where the maxima's gradient went: dx less the elementwise term, at (tied line, i1) and (tied line, i2)
    tie_ref, direct = R.mm_tie_terms(m, dy)
    tie = dx - direct
    cross = (m if kind == "support" else m.transpose(2, 3))[..., i1].argmax(dim=2)
    sel = torch.zeros(m.shape[:3] if kind == "support" else (2, Cc, NB), dtype=torch.bool)
    sel[:, :, lines] = True
    sel.scatter_(2, cross.unsqueeze(2), False)   # that line holds the pair's own cross maximum
    tt, tr = (tie, tie_ref) if kind == "support" else (tie.transpose(2, 3), tie_ref.transpose(2, 3))
    on1, on2, want1 = float(tt[..., i1][sel].abs().sum()), float(tt[..., i2][sel].abs().sum()), float(tr[..., i1][sel].abs().sum())
    print(f"MutualMatching backward dup_{kind} C={Cc}: {e:.2e}; tie mass on first {on1:.4g} (ref {want1:.4g}), on second {on2:.2e}")
    assert e < R.TOL_GRAD
    assert want1 > 0 and abs(on1 - want1) < R.TOL_GRAD * want1 and on2 < R.TOL_GRAD * want1


def test_mutual_matching_backward_dead_lines(dev):
    """One whole row and one whole column exactly 0: u = v = 1e-5 there, srow / u and scol / w finite."""
    m, a0, b0 = R.dead_lines(2, 3, 42, 42, 61)
    dy = R.rand(m.shape, 62, -1, 1).float().double()
    ref = mm_ref(m, dy)
    dx = mm_bwd(dev, m, dy)
    e = R.rel(dx, ref)
    print(f"MutualMatching backward dead row / column: {e:.2e}")
    assert torch.isfinite(dx).all() and e < R.TOL_GRAD
    assert float(dx[:, :, a0].abs().max()) == 0 and float(dx[:, :, :, b0].abs().max()) == 0


def run_chain(dev, case):
    """net.corr_forward under autograd on a match_ref chain case -> name -> tensor, as R.chain_grads"""
    from few_shot_seg_cwt_amd.match import MatchNet
    L = case["corr"].shape[1]
    net = MatchNet(temp=case["temp"], in_channel=L, sym_mode=case["sym"], device=dev)
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.copy_(case["sd"][n].float())
    corr = case["corr"].float().to(dev).requires_grad_(True)
    v = case["v"].float().to(dev).requires_grad_(True)
    corr2d, wv = net.corr_forward(corr, v, ret_attn=True)
    ((corr2d * case["G1"].float().to(dev)).sum() + (wv * case["G2"].float().to(dev)).sum()).backward()
    out = dict(corr2d=corr2d, wv=wv, d_corr=corr.grad, d_v=v.grad)
    for n, p in net.named_parameters():
        out[n.replace("NeighConsensus.conv.", "")] = p.grad
    return out


def chain_errs(got, ref):
    fwd = {k: R.rel(got[k], ref[k]) for k in ("corr2d", "wv")}
    grad = {k: R.rel(got[k], ref[k]) for k in ref if k not in fwd}
    return fwd, grad


@pytest.mark.parametrize("kind,h,w", [("support", 6, 7), ("query", 5, 5)])
@pytest.mark.parametrize("L", [1, 2])
def test_corr_forward_backward_duplicated_positions(dev, kind, L, h, w):
    case = R.chain_case(kind, 2, L, h, w, 50 + L)
    ref = R.chain_grads(case, R.corr_forward_ref)
    amax = R.chain_grads(case, M.corr_forward)     # the even split, for the printed distance alone
    got = run_chain(dev, case)
    fwd, grad = chain_errs(got, ref)
    far = R.rel(got["d_corr"], amax["d_corr"])
    print(f"corr_forward backward dup_{kind} L={L} {h}x{w}: " + ", ".join(f"{k} {e:.1e}" for k, e in {**fwd, **grad}.items())
          + f"; d_corr from the even split {far:.1e}")
    assert max(fwd.values()) < R.TOL_FWD, fwd
    assert max(grad.values()) < R.TOL_GRAD, grad
    assert far > R.SEPARATION / 2     # on the first index, not split


def test_corr_forward_backward_dead_rows(dev):
    """A last-layer bias low enough that whole rows of the consensus output are 0 (asserted on the device's
    own corr2d too): the second MutualMatching divides by u = v = 1e-5 there; everything finite, in the bars."""
    case = R.dead_chain_case(2, 1, 6, 7, 71)
    y = R.consensus_out(case)
    dead = y.amax(2) == 0
    assert int(dead.sum()) >= 2 and int((y > 0).sum()) >= 8
    ref = R.chain_grads(case, R.corr_forward_ref)
    got = run_chain(dev, case)
    assert all(torch.isfinite(t).all() for t in got.values())
    c2 = got["corr2d"].detach().cpu()
    assert float(c2[dead].abs().max()) == 0 and float(c2.abs().max()) > 0
    fwd, grad = chain_errs(got, ref)
    print(f"corr_forward backward dead rows ({int(dead.sum())} of {dead.numel()}): "
          + ", ".join(f"{k} {e:.1e}" for k, e in {**fwd, **grad}.items()))
    assert max(fwd.values()) < R.TOL_FWD, fwd
    assert max(grad.values()) < R.TOL_GRAD, grad


def test_masks_on_ties(dev):
    """cwt_match_masks: every support position of entry 0 ig-masked (the entry all 1e-4, every argmax a tie
    over the whole line: index 0), entry 1 with doubled column and row maxima.  Exact."""
    NA = NB = 42
    c, ig, sm = R.mask_corr(NA, NB, 101)
    want, inc_want = R.support_masks_first(c.float().double(), ig, sm)
    cd = c.float().to(dev)
    igd, smd = ig.to(torch.uint8).to(dev), sm.to(dev)
    inc = torch.full((2, NB), float("nan"), device=dev)
    _lib.check(_lib.lib().cwt_match_masks(_lib.ctx(dev.index), _lib.ptr(cd), 2, NA, NB, _lib.ptr(igd), _lib.ptr(smd),
                                          _lib.ptr(inc), _lib.stream_ptr(dev)), "cwt_match_masks")
    assert torch.equal(inc.cpu().double(), inc_want)
    assert torch.equal(cd.cpu(), want.float())   # 1e-4, the copied scores and the -1000 shift are exact in fp32


def _get_corr64(fq, fs):
    B, Cc, h, w = fq.shape
    nq = torch.nn.functional.normalize(fq, dim=1).reshape(B, Cc, h * w)
    ns = torch.nn.functional.normalize(fs, dim=1).reshape(B, Cc, h * w)
    return torch.bmm(nq.transpose(1, 2), ns).reshape(B, 1, h, w, h, w)


def test_forward_masks_all_masked_entry(dev):
    """MatchNet.forward(..., ig_mask, s_mask, use_cyc=True, ret_cyc=True) with every support position of entry
    0 masked and none of entry 1: the inconsistency mask is support_masks_first of the device's own unmasked
    corr2d, exactly; corr2d within 2e-5; the all-masked entry's softmax uniform (its weighted v the mean of
    v over the positions the cycle mask leaves); d_v and the parameter gradients within 1e-4."""
    from few_shot_seg_cwt_amd.match import MatchNet
    B, Cc, h, w, Cv, temp = 2, 64, 6, 7, 48, 20.0
    hw = h * w
    sd = R.consensus_params(1, 111)
    net = MatchNet(temp=temp, in_channel=1, sym_mode=True, cyc=True, device=dev)
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.copy_(sd[n].float())
    net.eval()
    fq0, fs0 = R.rand((B, Cc, h, w), 112).float().double(), R.rand((B, Cc, h, w), 113).float().double()
    v0 = R.rand((B, Cv, h, w), 114, -1, 1).float().double()
    ig = torch.zeros(B, hw, dtype=torch.bool)
    ig[0] = True
    sm = (torch.rand(B, h, w, generator=torch.Generator().manual_seed(115)) < 0.4).long()
    G1, G2 = R.rand((B, Cv, h, w), 116, -1, 1), R.rand((B, hw, hw), 117, -1, 1)
    fq, fs = fq0.float().to(dev), fs0.float().to(dev)
    with torch.no_grad():   # the device's own unmasked corr2d: what its argmaxes saw
        _, plain = net(fq, fs, v0.float().to(dev), ret_corr=True)
    _, inc_want = R.support_masks_first(plain.reshape(B, hw, hw).double().cpu(), ig, sm.reshape(B, hw))
    v = v0.float().to(dev).requires_grad_(True)
    wv, corr, inc = net(fq, fs, v, s_mask=sm.to(dev), ig_mask=ig.to(dev), ret_corr=True, use_cyc=True, ret_cyc=True)
    ((wv * G1.float().to(dev)).sum() + (corr.reshape(B, hw, hw) * G2.float().to(dev)).sum()).backward()
    assert torch.equal(inc[:, 0].detach().cpu().double(), inc_want)
    assert torch.equal(inc_want[0], (sm.reshape(B, hw)[0] != sm.reshape(B, hw)[0, 0]).double())   # index 0 everywhere
    # float64 chain with that mask
    sdr = {k: t.clone().requires_grad_(True) for k, t in sd.items()}
    vo = v0.clone().requires_grad_(True)
    c2 = R.corr_forward_ref(_get_corr64(fq0, fs0), vo, M.layers_from_state(sdr), temp, True)[0]
    c2 = c2.masked_fill(ig.reshape(B, 1, hw).expand(c2.shape), 0.0001) + inc_want.unsqueeze(1) * (-1000.0)
    attn = torch.softmax(c2 * temp, dim=-1)
    wvo = torch.bmm(vo.reshape(B, Cv, hw), attn.transpose(1, 2)).reshape(B, Cv, h, w)
    ((wvo * G1).sum() + (c2 * G2).sum()).backward()
    keep = inc_want[0] == 0
    uniform = v0[0].reshape(Cv, hw)[:, keep].mean(1)
    assert int(keep.sum()) > 1 and R.rel(wv[0].reshape(Cv, hw), uniform.unsqueeze(1).expand(Cv, hw)) < R.TOL_FWD
    params = dict(net.named_parameters())
    fwd = dict(wv=R.rel(wv, wvo), corr2d=R.rel(corr.reshape(B, hw, hw), c2))
    grad = dict(d_v=R.rel(v.grad, vo.grad))
    for n in R.PARAM_NAMES:
        grad[n.replace("NeighConsensus.conv.", "")] = R.rel(params[n].grad, sdr[n].grad)
    print("MatchNet masks, entry 0 all masked: " + ", ".join(f"{k} {e:.1e}" for k, e in {**fwd, **grad}.items()))
    assert float(sdr[R.PARAM_NAMES[0]].grad.abs().max()) > 0
    assert max(fwd.values()) < R.TOL_FWD, fwd
    assert max(grad.values()) < R.TOL_GRAD, grad


@pytest.mark.parametrize("Cc", [4, 100, 512])
def test_corr_and_backward_zero_norm_tokens(dev, Cc):
    """cwt_corr / cwt_corr_backward with an all-zero query token, an all-zero key token and a key token of norm
    1e-20 (below F.normalize's eps 1e-12: xn = x / eps, dx = dxn / eps).  Rows above eps against the existing
    bars relative to their own maximum; the dx = dxn / eps rows apart, relative to theirs, so their 1e12 scale
    hides nothing."""
    B, Pq, Pk, eps = 2, 37, 41, 1e-12
    q = (R.rand((B, Pq, Cc), 120 + Cc) - 0.3).float().double()
    k = (R.rand((B, Pk, Cc), 121 + Cc) - 0.3).float().double()
    q[0, 5] = 0.0
    k[1, 7] = 0.0
    k[0, 3] = 0.0
    k[0, 3, 1] = float(torch.tensor(1e-20, dtype=torch.float32))
    G = R.rand((B, Pq, Pk), 122 + Cc, -1, 1).float().double()
    small_q = torch.zeros(B, Pq, dtype=torch.bool)
    small_q[0, 5] = True
    small_k = torch.zeros(B, Pk, dtype=torch.bool)
    small_k[1, 7] = small_k[0, 3] = True
    # float64: normalize_fwd_bwd around the bmm
    qn, _ = R.normalize_fwd_bwd(q, torch.zeros_like(q), eps)
    kn, _ = R.normalize_fwd_bwd(k, torch.zeros_like(k), eps)
    sim_ref = torch.bmm(qn, kn.transpose(1, 2))
    _, dq_ref = R.normalize_fwd_bwd(q, torch.bmm(G, kn), eps)
    _, dk_ref = R.normalize_fwd_bwd(k, torch.bmm(G.transpose(1, 2), qn), eps)
    qd, kd, Gd = q.float().to(dev), k.float().to(dev), G.float().to(dev)
    sim = torch.full((B, Pq, Pk), float("nan"), device=dev)
    dq, dk = torch.full_like(qd, float("nan")), torch.full_like(kd, float("nan"))
    st = _lib.stream_ptr(dev)
    _lib.check(_lib.lib().cwt_corr(_lib.ctx(dev.index), _lib.ptr(qd), _lib.ptr(kd), B, Pq, Pk, Cc, _lib.ptr(sim), st),
               "cwt_corr")
    _lib.check(_lib.lib().cwt_corr_backward(_lib.ctx(dev.index), _lib.ptr(qd), _lib.ptr(kd), B, Pq, Pk, Cc, _lib.ptr(Gd),
                                            _lib.ptr(dq), _lib.ptr(dk), 0, 0, st), "cwt_corr_backward")
    sim, dq, dk = sim.cpu().double(), dq.cpu().double(), dk.cpu().double()
    assert torch.isfinite(sim).all() and torch.isfinite(dq).all() and torch.isfinite(dk).all()
    assert float(sim[0, 5].abs().max()) == 0 and float(sim[1, :, 7].abs().max()) == 0
    errs = dict(sim=R.rel(sim, sim_ref), dq=R.rel(dq[~small_q], dq_ref[~small_q]), dk=R.rel(dk[~small_k], dk_ref[~small_k]),
                dq_eps=R.rel(dq[small_q], dq_ref[small_q]), dk_eps=R.rel(dk[small_k], dk_ref[small_k]))
    print(f"corr / backward C={Cc} with zero-norm tokens: " + ", ".join(f"{k_} {e:.1e}" for k_, e in errs.items())
          + f"; max|dq_eps| {float(dq_ref[small_q].abs().max()):.1e}")
    assert float(dq_ref[small_q].abs().max()) > 1e9 and float(dk_ref[small_k].abs().max()) > 1e9
    assert errs["sim"] < R.TOL_FWD, errs
    assert max(errs["dq"], errs["dk"], errs["dq_eps"], errs["dk_eps"]) < R.TOL_GRAD, errs
