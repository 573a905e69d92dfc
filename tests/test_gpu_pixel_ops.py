"""The per-pixel kernels of csrc/seg.hip, one at a time, against float64 torch (and the oracle's
intersection_union) at the shapes where a kernel goes wrong: sizes that are no multiple of the
pixels per block, one block and more than one grid stride, h != w, S != 8 (h - 1) + 1, exact
argmax ties, targets all ignored or all one class, out-of-range class indices, an accumulating
output that is not zero, and n = 0."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tail_ref as R
from oracle import cwt_oracle as O

pytestmark = pytest.mark.gpu

SEED = 2021
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _rng(*key):
    return np.random.default_rng([SEED, *key])


def _cl(x, dev):
    return x.to(dev).contiguous(memory_format=torch.channels_last)


# ---------------------------------------------------------------- seg_metrics / seg_metrics_pair
def _targets(rng, B, S):
    """item 0 a mix of 0 / 1 / 255, item 1 all 0, item 2 all 255."""
    tg = (rng.random((B, S, S)) < 0.3).astype(np.int64)
    tg[rng.random((B, S, S)) < 0.05] = 255
    if B >= 2:
        tg[1] = 0
    if B >= 3:
        tg[2] = 255
    return torch.from_numpy(tg)


def _metrics_both(lg, lg2, tg, dev):
    """seg_metrics of lg and of lg2, and seg_metrics_pair(lg, lg2): the pair call must equal the
    two single calls bitwise.  Returns (iut, ce, iut2) on the host."""
    from few_shot_seg_cwt_amd.util import seg_metrics, seg_metrics_pair
    lg, lg2, tg = lg.to(dev), lg2.to(dev), tg.to(dev)
    iut, ce = seg_metrics(lg, tg)
    iut2, none = seg_metrics(lg2, tg, with_ce=False)
    piut, pce, piut2 = seg_metrics_pair(lg, lg2, tg)
    torch.cuda.synchronize()
    assert none is None
    assert torch.equal(piut, iut) and torch.equal(pce, ce) and torch.equal(piut2, iut2)
    return iut.double().cpu(), ce.double().cpu(), iut2.double().cpu()


@pytest.mark.parametrize("B,h,S", [(1, 2, 9), (3, 5, 33), (2, 33, 257)])
def test_seg_metrics_integer_logits_exact_counts(dev, B, h, S):
    """Integer logits in [-8, 8] at S - 1 = 8 (h - 1), the left half of plane 1 copied from plane 0:
    the upsample is exact in fp32 (test_tail_ref_cpu.py), so the counts equal the float64
    reference's with no slack, every exact tie counted as class 0; the CE terms are fp32 and
    their sum double: 1e-6 relative.  S = 9: one block; S = 257: the grid-stride loop runs twice."""
    rng = _rng(1, B, h, S)
    lg, lg2 = R.integer_logits(rng, B, h, h), R.integer_logits(rng, B, h, h)
    tg = _targets(rng, B, S)
    up = O.upsample(lg.double(), S)
    assert float(((up[:, 1] == up[:, 0]) & (tg != 255)).sum()) >= 0.01 * float((tg != 255).sum())
    iut, ce, iut2 = _metrics_both(lg, lg2, tg, dev)
    iutr, cesr, cecr = R.metrics_reference(lg, tg)
    iut2r, _, _ = R.metrics_reference(lg2, tg)
    assert torch.equal(iut, iutr), (iut, iutr)
    assert torch.equal(iut2, iut2r), (iut2, iut2r)
    assert torch.equal(ce[:, 1], cecr)
    assert bool(((ce[:, 0] - cesr).abs() <= 1e-6 * cesr.abs()).all()), (ce[:, 0], cesr)
    if B >= 3:   # the all-255 item
        assert float(ce[2].abs().sum() + iut[2].abs().sum()) == 0.0
    if B >= 2:   # the all-0 item: no class-1 target, every valid pixel counted
        assert float(iut[1, 2, 1]) == 0.0 and float(iut[1, 2, 0]) == S * S == float(ce[1, 1])


@pytest.mark.parametrize("h,w,S", [(5, 9, 33), (7, 7, 50), (3, 4, 1), (33, 33, 257)])
def test_seg_metrics_real_logits_any_geometry(dev, h, w, S):
    """N(0,1) logits at h != w, S != 8 (h - 1) + 1 and S = 1.  The kernel's lerp is two levels over
    four taps in fp32, so an upsampled logit is within 8 x 2^-24 x max |logits| of the float64 one
    (weights and products rounded once each, three adds): pixels whose reference margin is within
    tau = that bound are set to 255 for both sides (at most 0.1 % of the valid ones), and the counts
    on the others are equal exactly.  CE: each fp32 term is within 2 tau (both logits) + 4 ulps of
    max |logits| + 1 (max, exp, log, the two adds) of its float64 value."""
    B = 2
    rng = _rng(2, h, w, S)
    lg = torch.from_numpy(rng.standard_normal((B, 2, h, w)).astype(np.float32))
    lg2 = torch.from_numpy(rng.standard_normal((B, 2, h, w)).astype(np.float32))
    tg = _targets(rng, B, S)
    lmax = float(max(lg.abs().max(), lg2.abs().max()))
    tau = 8 * EPS * lmax
    up, up2 = O.upsample(lg.double(), S), O.upsample(lg2.double(), S)
    low = ((up[:, 1] - up[:, 0]).abs() <= tau) | ((up2[:, 1] - up2[:, 0]).abs() <= tau)
    valid = tg != 255
    share = float((low & valid).sum()) / max(float(valid.sum()), 1.0)
    print(f"h={h} w={w} S={S}: masked share {share:.5f}")
    assert share <= 0.001
    tg = tg.clone()
    tg[low] = 255
    iut, ce, iut2 = _metrics_both(lg, lg2, tg, dev)
    iutr, cesr, cecr = R.metrics_reference(lg, tg)
    iut2r, _, _ = R.metrics_reference(lg2, tg)
    assert torch.equal(iut, iutr) and torch.equal(iut2, iut2r), (iut, iutr, iut2, iut2r)
    assert torch.equal(ce[:, 1], cecr)
    assert bool(((ce[:, 0] - cesr).abs() <= cecr * (2 * tau + 4 * EPS * (lmax + 1.0))).all()), (ce[:, 0], cesr)


def test_seg_metrics_large_logits_finite_ce(dev):
    """Logits of +-80: exp(160) overflows fp32 unless the log-sum-exp subtracts the max."""
    B, h, S = 2, 5, 33
    rng = _rng(3)
    lg = torch.from_numpy((rng.integers(0, 2, size=(B, 2, h, h)) * 160.0 - 80.0).astype(np.float32))
    tg = _targets(rng, B, S)
    iut, ce, _ = _metrics_both(lg, lg.flip(1).contiguous(), tg, dev)
    iutr, cesr, cecr = R.metrics_reference(lg, tg)
    assert bool(torch.isfinite(ce).all()) and float(cesr.min()) > 80.0
    assert torch.equal(iut, iutr) and torch.equal(ce[:, 1], cecr)
    assert bool(((ce[:, 0] - cesr).abs() <= 1e-6 * cesr.abs()).all()), (ce[:, 0], cesr)


# ---------------------------------------------------------------- normalize / classify / classify_scaled
def _features(rng, B, Cc, h, w, zero_pixel):
    f = np.abs(rng.standard_normal((B, Cc, h, w))).astype(np.float32)
    if zero_pixel:
        f.reshape(B, Cc, h * w)[:, :, (h * w) // 2] = 0.0
    return torch.from_numpy(f)


def _weights(rng, f, B, Cc):
    """W [B,2,C] at 0.05.  The bar of these tests is 1e-6 of max |ref|, which presumes that the
    largest logit is at the scale of its sum: at least one standard deviation of its random-sign
    terms, sqrt(sum_c w_c^2 f_c^2).  A draw whose largest logit cancelled below that (likely only
    with one or two pixels) is redrawn -- judged on the float64 reference alone."""
    f64 = torch.as_tensor(f).double().flatten(2)
    for _ in range(64):
        W = torch.from_numpy((0.05 * rng.standard_normal((B, 2, Cc))).astype(np.float32))
        ref = torch.bmm(W.double(), f64)
        if float(ref.abs().max()) >= float(torch.bmm(W.double() ** 2, f64 ** 2).sqrt().max()):
            return W
    raise AssertionError("no well-scaled draw")


PIXELS = [(1, 1), (1, 5), (7, 9)]   # P = 1, 5, 63: no multiple of the four pixels of a block


@pytest.mark.parametrize("with_w0", [False, True])
@pytest.mark.parametrize("h,w", PIXELS)
@pytest.mark.parametrize("B", [1, 3])
def test_normalize_vs_float64(dev, B, h, w, with_w0):
    """F.normalize over channels (+ the baseline logits W0 . f): 512 fp32 FMAs and a wave sum per
    pixel, 1e-6 of max |ref|; an all-zero pixel gives zeros (the 1e-12 floor), not NaN."""
    from few_shot_seg_cwt_amd.episode import normalize
    rng = _rng(4, B, h, w)
    f = _features(rng, B, 512, h, w, zero_pixel=h * w > 1)
    W0 = _weights(rng, f, B, 512)
    out, lg0 = normalize(_cl(f, dev), W0.to(dev) if with_w0 else None)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    assert R.relerr(out, F.normalize(f.double(), dim=1)) < 1e-6
    if h * w > 1:
        assert float(out.permute(0, 2, 3, 1).reshape(B, h * w, 512)[:, (h * w) // 2].abs().max()) == 0.0
    if with_w0:
        assert R.relerr(lg0, O.classify(W0.double(), f.double())) < 1e-6
    else:
        assert lg0 is None


@pytest.mark.parametrize("Cc", [64, 192, 512, 2048])
@pytest.mark.parametrize("h,w", PIXELS)
@pytest.mark.parametrize("B", [1, 3])
def test_classify_vs_float64(dev, B, h, w, Cc):
    """W . f per pixel at C = 512 (classify_kernel) and any other multiple of 64
    (classify_c_kernel): C fp32 FMAs and a wave sum, 1e-6 of max |ref|."""
    from few_shot_seg_cwt_amd.episode import classify
    rng = _rng(5, B, h, w, Cc)
    f = _features(rng, B, Cc, h, w, zero_pixel=h * w > 1)
    W = _weights(rng, f, B, Cc)
    lg = classify(W.to(dev), _cl(f, dev))
    torch.cuda.synchronize()
    assert R.relerr(lg, O.classify(W.double(), f.double())) < 1e-6
    if h * w > 1:
        assert float(lg.reshape(B, 2, h * w)[:, :, (h * w) // 2].abs().max()) == 0.0


@pytest.mark.parametrize("Cc", [96, 4096])
def test_classify_refuses_other_widths(dev, Cc):
    from few_shot_seg_cwt_amd import _lib
    from few_shot_seg_cwt_amd.episode import classify
    f = torch.ones((1, Cc, 2, 2), device=dev).contiguous(memory_format=torch.channels_last)
    with pytest.raises(_lib.CwtError):
        classify(torch.ones((1, 2, Cc), device=dev), f)


@pytest.mark.parametrize("h,w", PIXELS)
@pytest.mark.parametrize("B", [1, 3])
def test_classify_scaled_vs_float64(dev, B, h, w):
    """(W . f_p) inv_p on the raw features, inv the fp32 1 / max(||f_p||, 1e-12) the token pass
    hands over (1e12 on an all-zero pixel, whose logits are 0)."""
    from few_shot_seg_cwt_amd.episode import classify_scaled
    rng = _rng(6, B, h, w)
    f = _features(rng, B, 512, h, w, zero_pixel=h * w > 1)
    W = _weights(rng, f, B, 512)
    inv = (1.0 / f.double().flatten(2).norm(dim=1).clamp_min(1e-12)).float()   # [B, hw]
    lg = classify_scaled(W.to(dev), _cl(f, dev), inv.to(dev))
    torch.cuda.synchronize()
    ref = O.classify(W.double(), f.double()) * inv.double().view(B, 1, h, w)
    assert bool(torch.isfinite(lg).all()) and R.relerr(lg, ref) < 1e-6
    if h * w > 1:
        assert float(inv[:, (h * w) // 2].min()) == float(np.float32(1e12))
        assert float(lg.reshape(B, 2, h * w)[:, :, (h * w) // 2].abs().max()) == 0.0


# ---------------------------------------------------------------- classify_bwd
@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (1, 17), (7, 9), (5, 13), (10, 13)])   # Pb = 1, 15, 17, 63, 65, 130
@pytest.mark.parametrize("B", [1, 3])
def test_classify_bwd_accumulates_into_dW(dev, B, h, w):
    """dW += sum_p dl_p f_p into a dW that is not zero, at pixel counts around the 16 pixels of a
    wave and the 64 of a block.  Element-wise bound: a sum of Pb products onto dW0 in fp32, in any
    order, is within (Pb + 2) 2^-24 (|dW0| + sum_p |dl_p| |f_p|) of the exact one."""
    from few_shot_seg_cwt_amd.episode import classify_bwd
    Pb = h * w
    rng = _rng(7, B, h, w)
    f = torch.from_numpy(rng.standard_normal((B, 512, h, w)).astype(np.float32))
    dl = torch.from_numpy(rng.standard_normal((B, 2, h, w)).astype(np.float32))
    dW0 = torch.from_numpy(rng.standard_normal((B, 2, 512)).astype(np.float32))
    dW = dW0.to(dev).clone()
    out = classify_bwd(dl.to(dev), _cl(f, dev), dW)
    torch.cuda.synchronize()
    assert out.data_ptr() == dW.data_ptr()
    dl64, f64 = dl.double().reshape(B, 2, Pb), f.double().reshape(B, 512, Pb)
    ref = dW0.double() + torch.einsum("bcp,bkp->bck", dl64, f64)
    bound = (Pb + 2) * EPS * (dW0.double().abs() + torch.einsum("bcp,bkp->bck", dl64.abs(), f64.abs()))
    err = (dW.double().cpu() - ref).abs()
    print(f"B={B} Pb={Pb}: max error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


# ---------------------------------------------------------------- intersectionAndUnionGPU
def _iou_numpy(preds, target, K, ignore):
    """util.py:280-308 restated with numpy: the ignored pixels take the ignore index as their
    prediction, the intersection is the predictions that equal the target, and each area is a
    K-bin histogram over [0, K - 1] (values outside it are dropped)."""
    p, t = preds.reshape(-1).copy(), target.reshape(-1)
    p[t == ignore] = ignore
    inter = p[p == t]
    hist = lambda x: np.histogram(x.astype(np.float64), bins=K, range=(0, K - 1))[0].astype(np.float64)
    ai, ao, at = hist(inter), hist(p), hist(t)
    return np.stack([ai, ao + at - ai, at])


@pytest.mark.parametrize("n", [0, 1, 255, 257, 131073])   # 131073: beyond the 512 x 256 threads of the grid
@pytest.mark.parametrize("ignore", [255, 7])
@pytest.mark.parametrize("K", [1, 2, 5, 16])
def test_iou_preds_vs_reference(dev, K, ignore, n):
    """Predictions in [-1, K] (so -1 and K occur), targets in [0, K + 3] and the ignore index:
    exact against the numpy restatement and, from two classes on, against the oracle's
    torch.histc form.  (With K = 1 the reference's histc(min=0, max=0) takes the data's own range
    -- torch's rule for min == max == 0 -- and counts every element; the kernel and the numpy
    restatement keep the literal range [0, K - 1].)  With the ignore index below K the reference
    counts an ignored pixel as intersection, output and target of that class."""
    from few_shot_seg_cwt_amd.util import intersectionAndUnionGPU
    rng = _rng(8, K, ignore, n)
    preds = rng.integers(-1, K + 1, size=n).astype(np.int64)
    target = rng.integers(0, K + 4, size=n).astype(np.int64)
    target[rng.random(n) < 0.1] = ignore
    if n >= 255:
        assert preds.min() == -1 and preds.max() == K and target.max() >= K + 3 and (target == ignore).any()
    i, u, t = intersectionAndUnionGPU(torch.from_numpy(preds).to(dev), torch.from_numpy(target).to(dev), K, ignore)
    torch.cuda.synchronize()
    got = torch.stack([i, u, t]).double().cpu().numpy()
    np.testing.assert_array_equal(got, _iou_numpy(preds, target, K, ignore))
    if K >= 2:
        ref = O.intersection_union(torch.from_numpy(preds), torch.from_numpy(target), K, ignore)
        np.testing.assert_array_equal(got, torch.stack(ref).double().numpy())


def test_iou_preds_refuses_17_classes(dev):
    from few_shot_seg_cwt_amd import _lib
    from few_shot_seg_cwt_amd.util import intersectionAndUnionGPU
    z = torch.zeros(8, dtype=torch.int64, device=dev)
    with pytest.raises(_lib.CwtError):
        intersectionAndUnionGPU(z, z, 17)


# ---------------------------------------------------------------- HipSGD / cwt_sgd_step
@pytest.mark.parametrize("n", [1, 1000, 524293])   # 524293: beyond the 2048 x 256 threads of the grid
@pytest.mark.parametrize("momentum,nesterov,wd", [(0.0, False, 0.0), (0.0, False, 1e-4), (0.9, False, 0.0),
                                                  (0.9, False, 1e-4), (0.9, True, 0.0), (0.9, True, 1e-4)])
def test_sgd_variants_vs_torch_float64(dev, n, momentum, nesterov, wd):
    """Three steps of every valid (momentum, nesterov, weight_decay) combination against
    torch.optim.SGD in float64 (1e-6 of max |ref|, test_sgd_nesterov_vs_torch's bar)."""
    from few_shot_seg_cwt_amd.optimizer import HipSGD
    rng = _rng(9, n)
    p0 = torch.from_numpy(rng.standard_normal(n).astype(np.float32))
    grads = [torch.from_numpy(rng.standard_normal(n).astype(np.float32)) for _ in range(3)]
    pr = p0.double().clone().requires_grad_(True)
    ref = torch.optim.SGD([pr], lr=0.05, momentum=momentum, weight_decay=wd, nesterov=nesterov)
    p = p0.to(dev).clone().requires_grad_(True)
    opt = HipSGD([p], lr=0.05, momentum=momentum, weight_decay=wd, nesterov=nesterov)
    for g in grads:
        pr.grad = g.double().clone()
        ref.step()
        p.grad = g.to(dev)
        opt.step()
        torch.cuda.synchronize()
        assert R.relerr(p, pr) < 1e-6
    if momentum:
        assert R.relerr(opt.bufs[0], ref.state[pr]["momentum_buffer"]) < 1e-6
    else:
        assert opt.bufs[0] is None


def test_sgd_step_of_nothing_is_a_no_op(dev):
    """cwt_sgd_step accepts n = 0: it returns 0, launches nothing and touches nothing (an empty
    grid is a launch error)."""
    from few_shot_seg_cwt_amd import _lib
    p = torch.arange(4, dtype=torch.float32, device=dev)
    g, buf = torch.ones_like(p), torch.full_like(p, 7.0)
    rc = _lib.lib().cwt_sgd_step(_lib.ctx(dev.index), _lib.ptr(p), _lib.ptr(g), _lib.ptr(buf), 0, 0.1, 0.9, 1e-4,
                                 1, 0, _lib.stream_ptr(dev))
    msg = _lib.lib().cwt_last_error().decode(errors="replace") if rc else ""
    torch.cuda.synchronize()
    assert rc == 0, msg
    assert p.tolist() == [0.0, 1.0, 2.0, 3.0] and g.tolist() == [1.0] * 4 and buf.tolist() == [7.0] * 4
