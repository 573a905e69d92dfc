"""The episode tail in its three forms, each against the float64 reference (tests/tail_ref.py: the
oracle composed on float64, nothing of the package), at the shapes and data where the kernels
take another path:

  modules      cwt_normalize + cwt_attention_fwd (t.infer) + cwt_classify + cwt_seg_metrics_pair
  fused        cwt_attention_infer + cwt_classify_scaled (cwt_tail) + cwt_seg_metrics_pair
  one launch   cwt_episode_tail, on its default grid and on CWT_TAIL_G = 1, 2 and 7 workgroups

Shapes (B, h), S = 8 (h - 1) + 1: one wave's tokens, one 32-token chunk, a ragged last chunk, more
than 32 chunks (the module combine's second round at h = 33) and h = 37, whose single-workgroup
launch takes P5's unstaged branch.  Data: benign, sparse, dead tokens (first, last, a whole chunk),
features scaled by 1e-3 / 1e3, one dominating token in the ragged last chunk, coinciding W rows
(pred_q0 ties on every pixel) and integer W, f (pred_q0 and its upsample exact in fp32).

Bars: W', pred_q, pred_q0 within 1e-5 of max |ref| (test_gpu_tail.TOL); the scaled and
dominating-token cases within max(4 x the fp32 oracle's own error against float64, 1e-5), measured
in tail_ref.case_reference and printed here.  Counts: the pixels whose reference margin |l1 - l0| is
within 2 x bar x max |logits| are set to 255 in the target both sides get (at most 0.5 % of the valid
pixels: test_tail_ref_cpu.py); on every other pixel a kernel within the bar has the reference's
argmax, so the counts are equal exactly, exact ties (class 0, as torch.argmax) included.  The CE
sum is held to 1e-5 relative (absolute below 1)."""
import os

import pytest
import torch

import tail_ref as R

pytestmark = pytest.mark.gpu

from few_shot_seg_cwt_amd import synthetic as syn  # noqa: E402

SEED = 2021
FORMS = ["modules", "fused", "one_launch", "one_launch_g1", "one_launch_g2", "one_launch_g7"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def tsd():
    return syn.make_transformer_state(4, 512, SEED)


@pytest.fixture(scope="module")
def transformer(dev, tsd):
    from few_shot_seg_cwt_amd import MultiHeadAttentionOne
    t = MultiHeadAttentionOne(4, 512, 512, 512, dropout=0.5)
    t.load_state_dict(tsd)
    t.eval()
    return t


def _one_launch(t, W, f, target, G):
    """episode_tail on G workgroups (None: the library's default grid)."""
    from few_shot_seg_cwt_amd.episode import episode_tail
    old = os.environ.get("CWT_TAIL_G")
    if G is None:
        os.environ.pop("CWT_TAIL_G", None)
    else:
        os.environ["CWT_TAIL_G"] = str(G)
    try:
        out = episode_tail(t, W, f, target)
        torch.cuda.synchronize()
    finally:
        if old is None:
            os.environ.pop("CWT_TAIL_G", None)
        else:
            os.environ["CWT_TAIL_G"] = old
    return out


def _run(t, form, W, f, target):
    """(W', pred_q, pred_q0, iut, ce, iut0, f_hat or None) of one form."""
    from few_shot_seg_cwt_amd.episode import classify, cwt_tail, normalize
    from few_shot_seg_cwt_amd.util import seg_metrics_pair
    if form == "modules":
        fqn, pq0 = normalize(f, W)
        W2 = t.infer(W, fqn)
        pq = classify(W2, fqn)
        iut, ce, iut0 = seg_metrics_pair(pq, pq0, target)
        torch.cuda.synchronize()
        return W2, pq, pq0, iut, ce, iut0, fqn
    if form == "fused":
        W2, pq, pq0 = cwt_tail(t, W, f)
        iut, ce, iut0 = seg_metrics_pair(pq, pq0, target)
        torch.cuda.synchronize()
        return W2, pq, pq0, iut, ce, iut0, None
    G = {"one_launch": None, "one_launch_g1": 1, "one_launch_g2": 2, "one_launch_g7": 7}[form]
    return (*_one_launch(t, W, f, target, G), None)


def _device_inputs(c, dev):
    f = c["f"].to(dev).contiguous(memory_format=torch.channels_last)
    return c["W"].to(dev), f, c["target"].to(dev)


def _ce_close(ce, ref_sum, tol=1e-5):
    d = (ce.double().cpu() - ref_sum).abs()
    return bool((d <= tol * ref_sum.abs().clamp_min(1.0)).all())   # relative; absolute below 1


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name,B,h", R.CASES)
def test_tail_form_vs_float64(dev, tsd, transformer, name, B, h, form):
    c = R.case_reference(name, B, h, tsd)
    W2r, pqr, pq0r, iutr, cesr, cecr, iut0r = c["ref"]
    bar = c["bar"]
    assert c["share"] <= R.MASK_CAP
    W, f, target = _device_inputs(c, dev)
    W2, pq, pq0, iut, ce, iut0, fqn = _run(transformer, form, W, f, target)
    from few_shot_seg_cwt_amd import _lib
    _lib.check_status()
    for x in (W2, pq, pq0, ce):
        assert bool(torch.isfinite(x).all()), f"{name} {form}: non-finite output"
    errs = dict(W2=R.relerr(W2, W2r), pred_q=R.relerr(pq, pqr), pred_q0=R.relerr(pq0, pq0r))
    print(f"{name} B={B} h={h} {form}: errors {errs} bar {bar:.3g} (fp32 oracle's own error {c['err32']}) "
          f"masked share {c['share']:.5f}")
    assert max(errs.values()) < bar, errs
    hw = h * h
    if name in R.SCALE:   # the unscaled reference: the normalisation cancels the scale, pred_q0 carries it
        base = R.case_reference("benign", B, h, tsd)["ref"]
        eb = dict(W2=R.relerr(W2, base[0]), pred_q=R.relerr(pq, base[1]),
                  pred_q0=R.relerr(pq0, base[2] * R.SCALE[name]))
        print(f"  against the unscaled reference: {eb}")
        assert max(eb.values()) < bar, eb
    dead = R.dead_tokens(name, hw)
    if dead:   # f_hat = 0 there (F.normalize's eps), so both logits are exactly 0
        assert float(pq.reshape(B, 2, hw)[:, :, dead].abs().max()) == 0.0
        assert float(pq0.reshape(B, 2, hw)[:, :, dead].abs().max()) == 0.0
        if fqn is not None:
            assert float(fqn.permute(0, 2, 3, 1).reshape(B, hw, 512)[:, dead].abs().max()) == 0.0
    if name == "exact":
        assert torch.equal(pq0.double().cpu(), pq0r)
        assert c["tie0"] >= 0.01
    # counts: exact on the masked target
    iut, iut0 = iut.double().cpu(), iut0.double().cpu()
    assert torch.equal(iut0, iut0r), (iut0, iut0r)
    if name == "wtie":
        # W's rows coincide: pred_q0 ties on every pixel -> class 0 everywhere (output count of
        # class 1 = intersection + union - target = 0); pred_q's planes coincide only up to
        # rounding, so of its counts only the target's are defined
        assert float((iut0[:, 0, 1] + iut0[:, 1, 1] - iut0[:, 2, 1]).abs().max()) == 0.0
        assert torch.equal(iut[:, 2], iutr[:, 2])
    else:
        assert torch.equal(iut, iutr), (iut, iutr)
    assert torch.equal(ce[:, 1].double().cpu(), cecr)
    assert _ce_close(ce[:, 0], cesr), (ce[:, 0], cesr)
    if B >= 2:   # the all-255 item: count 0, CE sum 0, counts all 0
        assert float(ce[1].abs().sum()) == 0.0 and float(iut[1].abs().sum() + iut0[1].abs().sum()) == 0.0


@pytest.mark.parametrize("name,B,h", [("benign", 1, 37), ("benign", 2, 6), ("exact", 1, 17)])
def test_one_launch_tail_does_not_depend_on_its_grid(dev, tsd, transformer, name, B, h):
    """P5 stages the low-res rows of a workgroup's pixel range in the LDS left beside its partials:
    sizeof(TailTok) - sizeof(TailMet) = 53760 - 33280 = 20480 bytes = 4 planes x 1280 floats.  One
    workgroup over h = 37 needs 37 x 37 = 1369 floats per plane and reads global memory instead;
    two workgroups (19 rows x 37 = 703) stage.  W', both logits and both count sets are bitwise
    the same on 1, 2, 7 and the default number of workgroups; the CE sums are double sums grouped
    by workgroup (1e-12 relative)."""
    c = R.case_reference(name, B, h, tsd)
    W, f, target = _device_inputs(c, dev)
    outs = {G: _one_launch(transformer, W, f, target, G) for G in (None, 1, 2, 7)}
    from few_shot_seg_cwt_amd import _lib
    _lib.check_status()
    W2d, pqd, pq0d, iutd, ced, iut0d = outs[None]
    for G in (1, 2, 7):
        W2, pq, pq0, iut, ce, iut0 = outs[G]
        assert torch.equal(W2, W2d) and torch.equal(pq, pqd) and torch.equal(pq0, pq0d), G
        assert torch.equal(iut, iutd) and torch.equal(iut0, iut0d), G
        assert torch.equal(ce[:, 1], ced[:, 1])
        assert bool(((ce[:, 0] - ced[:, 0]).abs() <= 1e-12 * ced[:, 0].abs()).all()), (G, ce, ced)
