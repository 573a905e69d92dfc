"""The N-way inner loop (adapt_nway.hip through episode.inner_adapt_nway) against the float64
reference of tests/adapt_nway_ref.py: every case within max(4 x E32, 1e-5) of the update; the 2-way
loop and the N = 2 loop against one reference; bitwise repeatability; the NaN rule; iters = 0; and
CWT_EARG before any device call."""
import pytest
import torch

import adapt_nway_ref as R
import adapt_ref as R2

pytestmark = pytest.mark.gpu

CASES = R.all_cases()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def run(c, dev, iters=None, f=None):
    from few_shot_seg_cwt_amd.episode import inner_adapt_nway
    f = (c["f"] if f is None else f).to(dev).contiguous(memory_format=torch.channels_last)
    W = c["W0"].to(dev).clone()
    inner_adapt_nway(f, c["lbl"].to(dev), W, R.LR, c["iters"] if iters is None else iters, c["fg"], c["tp"])
    torch.cuda.synchronize()
    return W.cpu()


@pytest.mark.parametrize("name,regime", CASES, ids=[f"{n}-{r}" for n, r in CASES])
def test_case_within_bar(dev, name, regime):
    c = R.make_case(name, regime)
    W = run(c, dev)
    if c["kind"] == "allign":
        assert torch.equal(W, c["W0"])   # every pixel ignored: W comes back as it went in
        return
    e = R.err(W, c["W_ref"], c["W0"])
    print(f"{name}/{regime}: err {e:.3g} bar {c['bar']:.3g}")
    assert torch.isfinite(W).all()
    assert e <= c["bar"], (e, c["bar"])


@pytest.mark.parametrize("iters", R.ITERS_SET)
def test_iters(dev, iters):
    c = R.make_case(R.ITERS_CASE, "steep")
    W = run(c, dev, iters)
    if iters == 0:
        assert torch.equal(W, c["W0"])
        return
    ref = R.adapt_nway_loop(c["f"], c["lbl"], c["W0"], R.LR, iters, c["fg"], c["tp"])
    e = R.err(W, ref, c["W0"])
    print(f"iters {iters}: err {e:.3g}")
    assert e <= c["bar"], e


@pytest.mark.parametrize("regime", ["flat", "steep"])
def test_two_way_agrees_with_inner_adapt(dev, regime):
    """N = 2, fg_idx = 1, tp = 1 and the 2-way loop on the same inputs, each within its bar of the
    same float64 reference (adapt_ref's 'pair' case)."""
    from few_shot_seg_cwt_amd.episode import inner_adapt, inner_adapt_nway
    c = R2.make_case("pair", regime)
    f = c["f"].to(dev).contiguous(memory_format=torch.channels_last)
    lbl, W0 = c["lbl"][0].to(dev), c["W0"][0]
    Wn = inner_adapt_nway(f, lbl, W0.to(dev).clone(), R2.LR, c["iters"], 1, 1.0).cpu()
    W2 = inner_adapt(f, lbl, W0.to(dev).clone(), R2.LR, c["iters"]).cpu()
    ref = R.adapt_nway_loop(c["f"], c["lbl"][0], W0, R2.LR, c["iters"], 1, 1.0)
    assert float((ref - c["W_ref"][0]).abs().max()) < 1e-12   # one reference
    en, e2 = float(R2.err(Wn, ref, W0)), float(R2.err(W2, ref, W0))
    print(f"{regime}: n-way {en:.3g} 2-way {e2:.3g} bar {c['bar']:.3g}")
    assert en <= c["bar"] and e2 <= c["bar"], (en, e2)


def test_bitwise_repeatable(dev):
    c = R.make_case("pair-N17", "steep")
    assert c["N"] == 17 and c["n"] == 5
    assert torch.equal(run(c, dev), run(c, dev))


def test_nan_in_features_poisons_every_entry(dev):
    c = R.make_case("pair-N17", "flat")
    f = c["f"].clone()
    f[2, 7, 1, 1] = float("nan")
    assert torch.isnan(run(c, dev, f=f)).all()
    assert torch.isnan(run(c, dev, iters=1, f=f)).all()


def test_earg(dev):
    from few_shot_seg_cwt_amd import _lib
    lib, ctx = _lib.lib(), _lib.ctx(dev.index)
    f = torch.zeros(1, 3, 3, 512, device=dev)
    lbl = torch.zeros(1, 17, 17, dtype=torch.int64, device=dev)
    W = torch.zeros(65, 512, device=dev)

    def call(N, fg, S=17):
        return lib.cwt_inner_adapt_nway(ctx, _lib.ptr(f), _lib.ptr(lbl), 1, 3, 3, 512, S, N, fg, 1.0, 0.1, 1,
                                        _lib.ptr(W), None)
    assert call(1, 0) == 1001
    assert call(65, 0) == 1001
    assert call(17, 17) == 1001
    assert call(17, -2) == 1001
    assert call(17, 1, S=18) == 1001
    assert call(17, 1) == 0
    torch.cuda.synchronize()
