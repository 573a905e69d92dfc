"""FuseNet1's 4-D stack on the device (csrc/fuse.hip: cwt_fuse_stack, cwt_fuse_stack_backward) against
the float64 reference of tests/fuse_ref.py: the forward (fused and training form) and the eight weight /
bias gradients.  The output lands at a non-zero column offset of a wider matrix whose other columns must
stay untouched; two calls give the same bits.

Bars: the project's, TOL_FWD on the outputs and TOL_GRAD on the gradients (max|HIP - ref| / max|ref|).
The gradient reference takes the device's side for the ReLU units within TOL_FWD max|pre| of zero and for
no others (match_ref.corr_forward_sided's rule); the tests assert that no unit outside that margin
disagrees and that at most 0.1 % of a layer lies inside it."""
import functools

import pytest
import torch

import fuse_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


ALL_SHAPES = R.STACK_SHAPES + [R.BIG_SHAPE]   # the last: the backward's workgroups take their grid stride


def geometry(shape):
    hA, wA, hB, wB = shape
    nb2 = ((hB + 1) // 2) * ((wB + 1) // 2)
    K = 2 * nb2 + 4
    return nb2, (K + 3) // 4 * 4 + 8, nb2 + 3   # columns written, ldx > 2 m^2 + 4, a non-zero offset


@functools.lru_cache(maxsize=None)
def reference(shape):
    x, p, G = R.stack_case(shape)
    pre1, pre2 = R.stack_pre(x, p)
    return x, p, G, torch.relu(pre1), torch.relu(pre2).reshape(G.shape)


def run_forward(dev, shape, save):
    from few_shot_seg_cwt_amd.fuse import fuse_stack
    x, p, _, _, _ = reference(shape)
    nb2, ldx, col = geometry(shape)
    g = torch.Generator().manual_seed(9)
    fill = torch.rand(shape[0] * shape[1], ldx, generator=g) - 2.0   # negative: never a ReLU output
    X = fill.to(dev)
    y1 = fuse_stack(x.float().to(dev), [t.float().to(dev) for t in p], X, col, save=save)
    return X, y1, fill


@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_stack_forward(dev, shape):
    _, _, _, y1_ref, y2_ref = reference(shape)
    nb2, ldx, col = geometry(shape)
    X, _, fill = run_forward(dev, shape, save=False)
    Xt, y1, _ = run_forward(dev, shape, save=True)
    e2 = R.rel(X[:, col:col + nb2], y2_ref)
    hA, wA = shape[:2]
    y1_dev = y1.cpu().reshape(1, hA, wA, *y1_ref.shape[-2:], 16).permute(0, 5, 1, 2, 3, 4)
    e1 = R.rel(y1_dev, y1_ref)
    print(f"fuse stack {shape}: y2 {e2:.2e} y1 {e1:.2e}")
    assert e2 < R.TOL_FWD and e1 < R.TOL_FWD, (e1, e2)
    # the fused and the training form give the same bits, and so do two calls
    assert torch.equal(X, Xt)
    assert torch.equal(run_forward(dev, shape, save=False)[0], X)
    # nothing outside the column range was written
    keep = torch.ones(ldx, dtype=torch.bool)
    keep[col:col + nb2] = False
    assert torch.equal(X.cpu()[:, keep], fill[:, keep])


@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_stack_backward(dev, shape):
    from few_shot_seg_cwt_amd.fuse import fuse_stack_backward
    x, p, G, _, _ = reference(shape)
    nb2, ldx, col = geometry(shape)
    hA, wA, hB, wB = shape
    X, y1, _ = run_forward(dev, shape, save=True)
    g = torch.Generator().manual_seed(10)
    dX = torch.rand(hA * wA, ldx, generator=g)     # the other columns hold noise the kernel must not read
    dX[:, col:col + nb2] = G.float()
    dX = dX.to(dev)
    pd = [t.float().to(dev) for t in p]
    xd = x.float().to(dev)

    def grads(accumulate, into=None):
        out = into if into is not None else [torch.full_like(t, 7.0) for t in pd]
        return fuse_stack_backward(xd, pd, y1, X, dX, col, out, accumulate)

    first = [t.clone() for t in grads(False)]
    again = grads(False)
    assert all(torch.equal(a, b) for a, b in zip(first, again)), "two calls differ"
    twice = grads(True, [t.clone() for t in first])

    # float64 on the device's side of the units float64 cannot settle
    sides = R.device_sides(y1, X[:, col:col + nb2], (1, hA, wA, (hB + 1) // 2, (wB + 1) // 2))
    pr = [t.clone().requires_grad_(True) for t in p]
    info = []
    y2 = R.stack_sided(x, pr, sides, info)
    (y2[0] * G).sum().backward()
    for near, bad, n in info:
        assert bad == 0, f"{bad} ReLU units outside the margin disagree with float64"
        assert near <= R.NEAR_CAP * n, (near, n)
    errs = {n: R.rel(a, b.grad) for n, a, b in zip(R.CONV_NAMES, first, pr)}
    print(f"fuse stack backward {shape}: near {[i[0] for i in info]} " + " ".join(f"{k[7:]} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) < R.TOL_GRAD, errs
    # both biases of a layer receive the same sum; accumulate adds a second correlation's gradients
    assert torch.equal(first[1], first[3]) and torch.equal(first[5], first[7])
    for a, b in zip(twice, first):
        assert R.rel(a, 2 * b) < 1e-6


def test_stack_batch_of_two(dev):
    """B = 2: the batch arithmetic of the forward (both forms) and of the backward, whose sums run over both
    correlations"""
    from few_shot_seg_cwt_amd.fuse import fuse_stack, fuse_stack_backward
    shape = (5, 7, 8, 8)
    hA, wA, hB, wB = shape
    x, p, G = R.stack_case_b2(shape)
    nb2, ldx, col = geometry(shape)
    pd, xd = [t.float().to(dev) for t in p], x.float().to(dev)
    X = torch.full((2 * hA * wA, ldx), -1.0, device=dev)
    Xf = X.clone()
    y1 = fuse_stack(xd, pd, X, col, save=True)
    fuse_stack(xd, pd, Xf, col, save=False)
    assert torch.equal(X, Xf)
    pre1, pre2 = R.stack_pre(x, p)
    assert R.rel(X[:, col:col + nb2], torch.relu(pre2).reshape(G.shape)) < R.TOL_FWD
    assert not torch.equal(X[:hA * wA], X[hA * wA:])
    dX = torch.zeros_like(X)
    dX[:, col:col + nb2] = G.float().to(dev)
    got = fuse_stack_backward(xd, pd, y1, X, dX, col, [torch.empty_like(t) for t in pd], False)
    again = fuse_stack_backward(xd, pd, y1, X, dX, col, [torch.empty_like(t) for t in pd], False)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    sides = R.device_sides(y1, X[:, col:col + nb2], (2, hA, wA, (hB + 1) // 2, (wB + 1) // 2))
    pr = [t.clone().requires_grad_(True) for t in p]
    info = []
    y2 = R.stack_sided(x, pr, sides, info)
    (y2.reshape(G.shape) * G).sum().backward()
    assert all(bad == 0 and near <= R.NEAR_CAP * n for near, bad, n in info), info
    errs = {n: R.rel(a, b.grad) for n, a, b in zip(R.CONV_NAMES, got, pr)}
    print("fuse stack B=2: " + " ".join(f"{k[7:]} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) < R.TOL_GRAD, errs


def test_stack_arguments(dev):
    from few_shot_seg_cwt_amd import _lib
    from few_shot_seg_cwt_amd.fuse import fuse_stack
    x, p, _, _, _ = reference((3, 3, 3, 3))
    pd = [t.float().to(dev) for t in p]
    X = torch.zeros(9, 4, device=dev)
    with pytest.raises(_lib.CwtError, match="ldx"):
        fuse_stack(x.float().to(dev), pd, X, 1)          # 1 + 4 columns do not fit in 4
    with pytest.raises(_lib.CwtError, match="sides"):
        fuse_stack(torch.zeros(1, 1, 3, 3, 3, device=dev), pd, torch.zeros(3, 4, device=dev), 0)
