"""The fusion trainer's head on the device (csrc/fuse.hip) against the float64 reference of
tests/fuse_ref.py: the support mask's resize, FuseNet1's forward and its twelve parameter gradients
through autograd, the blend and its backward, and the disagreement-weighted loss head with its counts.

Bars: TOL_FWD on outputs, TOL_GRAD on gradients; the IoU counts and the disagreement count are exact
integers.  ReLU units within TOL_FWD max|pre| of zero take the device's side in the gradient reference
(tests/test_gpu_fuse_stack.py's rule, here also for the attention net's hidden layer).  The attention
net's first layer at the trainer's K = 1804 is held to the bar tests/test_gpu_detr.py holds cwt_linear to."""
import math

import pytest
import torch

import fuse_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


@pytest.mark.parametrize("S,m", [(17, 3), (33, 5), (57, 4), (57, 15)])
@pytest.mark.parametrize("align", [True, False])
@pytest.mark.parametrize("pool", [False, True])
def test_support_mask(dev, S, m, align, pool):
    from few_shot_seg_cwt_amd.fuse import support_mask
    lbl = R.label_case(S, S)
    assert int((lbl == 255).sum()) > 0
    got = support_mask(lbl.to(dev), m, align, pool)
    e = R.rel(got, R.support_mask(lbl, m, align, pool))
    print(f"support mask S={S} m={m} align={align} pool={pool}: {e:.2e}")
    assert got.shape == (1, 1, m, m) and e < R.TOL_FWD


def _net(dev, c, mid):
    from few_shot_seg_cwt_amd.transformer import FuseNet1
    net = FuseNet1(im_size=c["m"], mid_dim=mid, device=dev)
    net.load_state_dict({k: v.float() for k, v in c["sd"].items()})
    return net


@pytest.mark.parametrize("shape", R.STACK_SHAPES)
@pytest.mark.parametrize("mid", [32, 256])
def test_fusenet1_forward_and_gradients(dev, shape, mid):
    c = R.head_case(shape, mid)
    hA, wA, hB, wB = shape
    m = c["m"]
    net = _net(dev, c, mid)
    net.record = {}
    args = ([t.float().to(dev) for t in c["corr"]], c["s_mask"].float().to(dev), [t.float().to(dev) for t in c["pd"]])
    wt = net(*args)
    (wt * c["G"].float().to(dev)).sum().backward()
    rec = net.record
    first = {n: p.grad.clone() for n, p in net.named_parameters()}
    # a second forward + backward gives the same bits
    net.zero_grad(set_to_none=True)
    wt2 = net(*args)
    (wt2 * c["G"].float().to(dev)).sum().backward()
    assert torch.equal(wt, wt2)
    for n, p in net.named_parameters():
        assert torch.equal(first[n], p.grad), n
    # eval (no parameter asks for a gradient: the fused stack, y1 never stored) gives the same bits too
    with torch.no_grad():
        assert torch.equal(net(*args), wt)
        net.eval_form = "two_pass"   # layer 1 stored for the call, as in training
        assert torch.equal(net(*args), wt)

    n2 = m * m
    sides = [R.device_sides(rec["y1"][i], rec["X"][:, i * n2:(i + 1) * n2], (1, hA, wA, m, m)) for i in range(2)]
    sd = {k: v.clone().requires_grad_(True) for k, v in c["sd"].items()}
    info = []
    ref = R.fusenet1(c["corr"], c["s_mask"], c["pd"], sd, sides=sides, att_side=rec["hid"].cpu() > 0, info=info)
    (ref * c["G"]).sum().backward()
    for near, bad, n in info:
        assert bad == 0, f"{bad} ReLU units outside the margin disagree with float64"
        assert near <= R.NEAR_CAP * n, (near, n)
    e_fwd = R.rel(wt, ref)
    errs = {n: R.rel(first[n], sd[n].grad) for n in R.PARAM_NAMES}
    print(f"FuseNet1 {shape} mid={mid}: wt {e_fwd:.2e} " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert wt.shape == (1, 2, hA, wA) and e_fwd < R.TOL_FWD
    assert max(errs.values()) < R.TOL_GRAD, errs


def test_fusenet1_pooled_mask_and_arguments(dev):
    c = R.head_case((4, 5, 5, 5), 32)
    net = _net(dev, c, 32)
    corr = [t.float().to(dev) for t in c["corr"]]
    pd = [t.float().to(dev) for t in c["pd"]]
    big = R.support_mask(R.label_case(57, 1), 2 * c["m"], True).float()
    with torch.no_grad():
        wt = net(corr, big.to(dev), pd)
    ref = R.fusenet1(c["corr"], big.double(), c["pd"], c["sd"])
    assert R.rel(wt, ref) < R.TOL_FWD
    with pytest.raises(ValueError):
        net(corr[:1], c["s_mask"].float().to(dev), pd)
    with pytest.raises(ValueError):
        net([t.repeat(2, 1, 1, 1, 1) for t in corr], c["s_mask"].float().to(dev), pd)


def test_attention_linear_at_the_trainers_width(dev):
    """att.0 at 473^2: K = 2 * 900 + 4 = 1804 columns, N = 256, 40 tokens; cwt_linear's own bar (1e-5,
    tests/test_gpu_detr.py::test_linear_accumulate at K = 3072)"""
    from few_shot_seg_cwt_amd.detr import linear
    x = R.rand((40, 1804), 1)
    w = R.rand((256, 1804), 2, -1, 1) / math.sqrt(1804)
    b = R.rand((256,), 3, -1, 1)
    out = linear(x.float().to(dev), w.float().to(dev), b.float().to(dev), relu=True)
    ref = torch.relu(x.float().double() @ w.float().double().T + b.float().double())
    e = R.rel(out, ref)
    e32 = R.rel(torch.relu(x.float() @ w.float().T + b.float()), ref)
    print(f"att.0 at K=1804: device {e:.2e}, fp32 torch on the CPU {e32:.2e}")
    assert e < 1e-5


@pytest.mark.parametrize("C,h,w", [(64, 5, 7), (512, 8, 8), (96, 3, 3)])
def test_blend_and_backward(dev, C, h, w):
    from few_shot_seg_cwt_amd.fuse import fuse_blend
    wv, fq = R.rand((1, C, h, w), 1, -1, 1).float(), R.rand((1, C, h, w), 2, -1, 1).float()
    wt0 = torch.softmax(R.rand((1, 2, h, w), 3, -2, 2), 1).float()
    G = R.rand((1, C, h, w), 4, -1, 1).float()
    wt = wt0.to(dev).requires_grad_(True)
    out = fuse_blend(wv.to(dev), fq.to(dev), wt)
    (out * G.to(dev)).sum().backward()
    wr = wt0.double().requires_grad_(True)
    ref = R.blend(wv.double(), fq.double(), wr)
    (ref * G.double()).sum().backward()
    e, eg = R.rel(out, ref), R.rel(wt.grad, wr.grad)
    print(f"blend C={C} {h}x{w}: out {e:.2e} d_wt {eg:.2e}")
    assert e < R.TOL_FWD and eg < R.TOL_GRAD


@pytest.mark.parametrize("S,h", [(17, 3), (33, 5), (57, 8)])
@pytest.mark.parametrize("kind", ["mixed", "ignored", "agree", "edge"])
def test_loss_head(dev, S, h, kind):
    from few_shot_seg_cwt_amd.fuse import fuse_loss_head
    q, q0, q1, lbl = R.loss_case(h, S, kind, seed=S)
    q, q0, q1 = q.float(), q0.float(), q1.float()
    qd = q.to(dev).requires_grad_(True)
    loss, iut, dis = fuse_loss_head(qd, q0.to(dev), q1.to(dev), lbl.to(dev))
    loss.backward()
    qr = q.double().requires_grad_(True)
    ref = R.fuse_loss(qr, q0.double(), q1.double(), lbl)
    ref.backward()
    iut_ref, dis_ref = R.fuse_counts(q.double(), q0.double(), q1.double(), lbl)
    assert torch.equal(iut.double().cpu(), iut_ref), (iut, iut_ref)
    assert int(dis.item()) == dis_ref
    if kind == "agree":
        assert dis_ref == 0
    e, eg = R.rel(loss, ref), R.rel(qd.grad, qr.grad)
    print(f"loss head S={S} h={h} {kind}: loss {float(loss.detach()):.6f} ({e:.2e}) d_pd_q {eg:.2e} disagree {dis_ref}")
    if kind == "ignored":
        assert float(loss.detach()) == 0.0 and float(qd.grad.abs().max()) == 0.0
    else:
        assert e < R.TOL_FWD and eg < R.TOL_GRAD
    # two calls give the same bits
    loss2, iut2, _ = fuse_loss_head(qd.detach(), q0.to(dev), q1.to(dev), lbl.to(dev))
    assert torch.equal(loss2, loss.detach()) and torch.equal(iut2, iut)
