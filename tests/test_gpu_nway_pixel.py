"""cwt_relabel_support and cwt_seg_metrics_nway (nway_pixel.hip) against float64 torch
(tests/nway_pixel_ref.py): labels and intersection / union / target counts exactly, the NLL to 1e-6
relative -- a saturated pixel (p_fg = 1 in float32) included."""
import numpy as np
import pytest
import torch

import nway_pixel_ref as P

pytestmark = pytest.mark.gpu

SHAPES = [(2, 9), (3, 17), (5, 23), (17, 129)]
NS = [2, 17, 62]
B = 2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


_inputs = {}


def inputs(h, S, N):
    """Logits, their float64 upsample and the labels of a shape, drawn once and never modified."""
    if (h, S, N) not in _inputs:
        z = P.draw_logits(7 + 100 * N + S, B, N, h, S)
        hi = P.upsample(z, S)
        gap, share = P.gap_of(hi)
        assert gap > P.GAP and share <= 1e-3, (gap, share)   # on the reference alone
        rng = np.random.default_rng([S, N])
        lbl = torch.from_numpy(rng.choice([0, 1, 255], size=(B, S, S), p=[0.6, 0.3, 0.1]).astype(np.int64))
        lbl[:, 0, 0] = torch.tensor([0, 1])
        _inputs[(h, S, N)] = (z, hi, lbl)
    return _inputs[(h, S, N)]


def idx_of(N, which):
    return 1 if which == "one" else N - 1


@pytest.mark.parametrize("which", ["one", "last"])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("h,S", SHAPES)
def test_relabel_support(dev, h, S, N, which):
    from few_shot_seg_cwt_amd.incremental import reset_spt_label
    idx = idx_of(N, which)
    z, hi, lbl = inputs(h, S, N)
    keep = lbl.clone()
    dl = lbl.to(dev)
    out = reset_spt_label(dl, z.to(dev), idx).cpu()
    assert torch.equal(dl.cpu(), keep)
    assert torch.equal(out, P.reset_spt_label_literal(lbl, hi, idx))


@pytest.mark.parametrize("which", ["one", "last"])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("h,S", SHAPES)
def test_seg_metrics_nway(dev, h, S, N, which):
    from few_shot_seg_cwt_amd.incremental import pred2bmask_metrics
    idx = idx_of(N, which)
    z, hi, lbl = inputs(h, S, N)
    iut, ce = pred2bmask_metrics(z.to(dev), lbl.to(dev), idx)
    iut2, ce2 = pred2bmask_metrics(z.to(dev), lbl.to(dev), idx)
    riut, rce = P.metrics_ref(hi, lbl, idx)
    assert torch.equal(iut.cpu().double(), riut)
    assert torch.equal(ce.cpu()[:, 1], rce[:, 1])
    rel = ((ce.cpu()[:, 0] - rce[:, 0]).abs() / rce[:, 0].abs()).max()
    print(f"h {h} S {S} N {N} idx {idx}: nll rel {float(rel):.3g}")
    assert rel <= 1e-6
    assert torch.equal(ce, ce2) and torch.equal(iut, iut2)   # bitwise reproducible


@pytest.mark.parametrize("N", [2, 17])
def test_saturated_pixel_stays_finite(dev, N):
    """p_fg = 1 in float32 (a gap of 60 to every other class) on pixels labelled 0: -log(1 - p_fg) is
    the gap, finite, and matches."""
    from few_shot_seg_cwt_amd.incremental import pred2bmask_metrics
    h, S, idx = 3, 17, 1
    z = P.draw_logits(5, 1, N, h, S).clone()
    z[:, idx] = z.amax(1) + 60.0
    lbl = torch.zeros(1, S, S, dtype=torch.int64)
    lbl[0, ::2] = 1
    hi = P.upsample(z, S)
    assert float(torch.softmax(hi.float(), 1)[:, idx].min()) == 1.0
    iut, ce = pred2bmask_metrics(z.to(dev), lbl.to(dev), idx)
    riut, rce = P.metrics_ref(hi, lbl, idx)
    assert torch.isfinite(ce).all() and torch.equal(iut.cpu().double(), riut)
    assert float((ce.cpu()[0, 0] - rce[0, 0]).abs() / rce[0, 0]) <= 1e-6
    assert float(rce[0, 0]) > 60.0 * int((lbl == 0).sum()) * 0.99


def test_earg(dev):
    from few_shot_seg_cwt_amd import _lib
    lib, ctx = _lib.lib(), _lib.ctx(dev.index)
    z = torch.zeros(1, 3, 2, 2, device=dev)
    lbl = torch.zeros(1, 9, 9, dtype=torch.int64, device=dev)
    out = torch.zeros_like(lbl)
    iut = torch.zeros(1, 3, 2, device=dev)
    assert lib.cwt_relabel_support(ctx, _lib.ptr(z), _lib.ptr(lbl), 1, 3, 2, 2, 9, 3, _lib.ptr(out), None) == 1001
    assert lib.cwt_relabel_support(ctx, _lib.ptr(z), _lib.ptr(lbl), 1, 65, 2, 2, 9, 1, _lib.ptr(out), None) == 1001
    assert lib.cwt_seg_metrics_nway(ctx, _lib.ptr(z), _lib.ptr(lbl), 1, 3, 2, 1, 9, 1, _lib.ptr(iut), None, None) == 1001
    assert lib.cwt_seg_metrics_nway(ctx, _lib.ptr(z), _lib.ptr(lbl), 1, 1, 2, 2, 9, 0, _lib.ptr(iut), None, None) == 1001
