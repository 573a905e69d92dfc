"""The fusion trainer's step and validation on the device (few_shot_seg_cwt_amd/fuse_train.py) from
synthetic features: one train_step teacher-forced against the float64 chain of tests/fuse_ref.py on the
step's own recorded inputs (the frozen MatchNet's outputs included), the one-shot rule, and
validate_epoch's three mIoUs against the reference formula on the logits it returns."""
import numpy as np
import pytest
import torch

import fuse_ref as R

pytestmark = pytest.mark.gpu

H, S, C, CM, MID = 8, 57, 64, 128, 32
# The update is read off fp32 parameters, and p_new carries one fp32 rounding, up to 2^-24 |p_new|.  At this
# fixture the gradients are ~1e-4 (the blend weights move the loss little), so at the trainer's own learning
# rates lr |g| would lie below what |p| ~ 0.3 resolves to 1e-4.  The step is linear in lr, so the fixture takes
# a learning rate at which every tensor's update IS resolvable (asserted below from the float64 reference
# alone) and holds it to TOL_GRAD of its size unchanged.
LR = 4096.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def features(dev, seed):
    f = lambda shape, s: R.rand(shape, s, -0.3, 1.0).float().to(dev).contiguous(memory_format=torch.channels_last)
    W = R.rand((2, C), seed + 4, -1, 1).float().to(dev) * 0.3
    return W, f((1, C, H, H), seed), f((1, C, H, H), seed + 1), f((1, CM, H, H), seed + 2), f((1, CM, H, H), seed + 3)


def batch(seed, shots=1):
    lbl = R.label_case(S, seed)
    return None, lbl[None], None, R.label_case(S, seed + 1)[None, None].repeat(1, shots, 1, 1), torch.tensor([3 + seed % 2])


def nets(dev):
    from few_shot_seg_cwt_amd.match import MatchNet, init_match_params
    from few_shot_seg_cwt_amd.transformer import FuseNet1
    corr = MatchNet(temp=20.0, cv_type="red", sym_mode=True, device=dev)
    init_match_params(corr, 7)
    torch.manual_seed(11)
    return corr, FuseNet1(im_size=H // 2, mid_dim=MID, device=dev)


def test_train_step_teacher_forced(dev):
    from few_shot_seg_cwt_amd.fuse_train import get_scheduler, train_step
    from few_shot_seg_cwt_amd.optimizer import HipSGD
    corr, net = nets(dev)
    args = dict(scheduler="cosine", epochs=1)
    opt = HipSGD(net.parameters(), lr=LR, momentum=0.9, weight_decay=0.0, nesterov=False)
    sched = get_scheduler(args, opt, 10)
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    frozen = {n: p.detach().clone() for n, p in corr.named_parameters()}
    net.record = {}
    rec = {}
    r = train_step(args, None, corr, net, opt, sched, batch(0), dev, rec, features=features(dev, 100))
    gates = net.record
    net.record = None
    assert all(torch.equal(frozen[n], p) for n, p in corr.named_parameters()), "the frozen MatchNet moved"
    assert opt.lr < LR   # the cosine scheduler stepped

    d = lambda t: t.detach().double().cpu()
    sd = {n: d(t).requires_grad_(True) for n, t in before.items()}
    m = H // 2
    sides = [R.device_sides(gates["y1"][i], gates["X"][:, i * m * m:(i + 1) * m * m], (1, H, H, m, m)) for i in range(2)]
    info = []
    wt = R.fusenet1([d(rec["l_corr"]), d(rec["h_corr"])], d(rec["s_mask"]), [d(rec["pred_q0"]), d(rec["pred_q1"])], sd,
                    sides=sides, att_side=gates["hid"].cpu() > 0, info=info)
    for near, bad, n in info:
        assert bad == 0 and near <= R.NEAR_CAP * n, (near, bad, n)
    out = R.blend(d(rec["weighted_v"]), d(rec["f_q"]), wt)
    pd_q = torch.einsum("kc,bchw->bkhw", d(rec["W"]), out)
    loss = R.fuse_loss(pd_q, d(rec["pred_q0"]), d(rec["pred_q1"]), rec["q_label"].cpu())
    loss.backward()
    # the support mask the step made is the training one (align_corners=True)
    assert R.rel(rec["s_mask"], R.support_mask(rec["s_label"][0].cpu(), m, True)) < R.TOL_FWD
    errs = {"loss": R.rel(r["q_loss"], loss), "wt": R.rel(r["wt"], wt), "pd_q": R.rel(r["pred_q"], pd_q)}
    assert max(errs.values()) < R.TOL_FWD, errs
    iut_ref, dis_ref = R.fuse_counts(pd_q.detach(), d(rec["pred_q0"]), d(rec["pred_q1"]), rec["q_label"].cpu())
    assert int(r["disagree"].item()) == dis_ref and dis_ref > 0
    assert torch.equal(r["iut"].double().cpu()[1:], iut_ref[1:])   # pred_q0, pred_q1: the recorded logits themselves
    # The step's gradients (train_step zeroes them before its backward, so they are still there), then the
    # update p_new - p_old against -lr g_ref (the first momentum step: buf = g), each at TOL_GRAD of its size.
    grd, upd = {}, {}
    for n, p in net.named_parameters():
        grd[n] = R.rel(p.grad, sd[n].grad)
        want = -LR * sd[n].grad
        # the fixture's precondition, from float64 alone: fp32 resolves this update 10x finer than the bar
        p_new = d(before[n]) + want
        assert 2.0 ** -24 * float(p_new.abs().max()) <= 0.1 * R.TOL_GRAD * float(want.abs().max()), n
        upd[n] = R.rel(d(p) - d(before[n]), want)
    print("fuse train step: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    print("  gradients: " + " ".join(f"{k} {v:.1e}" for k, v in grd.items()))
    print("  updates:   " + " ".join(f"{k} {v:.1e}" for k, v in upd.items()))
    assert max(grd.values()) < R.TOL_GRAD, grd
    assert max(upd.values()) < R.TOL_GRAD, upd


def test_more_than_one_shot_raises(dev):
    from few_shot_seg_cwt_amd.fuse_train import train_step
    from few_shot_seg_cwt_amd.optimizer import HipSGD
    corr, net = nets(dev)
    opt = HipSGD(net.parameters(), lr=LR)
    with pytest.raises(ValueError, match="one-shot"):
        train_step({}, None, corr, net, opt, None, batch(0, shots=2), dev, features=features(dev, 100))


def test_validate_epoch(dev):
    from few_shot_seg_cwt_amd.fuse_train import validate_epoch
    corr, net = nets(dev)
    loader = [batch(s) for s in (0, 1, 2)]
    seeds = {id(b): 200 + 10 * i for i, b in enumerate(loader)}
    eps = []
    m0, m1, m, loss = validate_epoch(dict(test_num=3), loader, None, corr, net, episodes_out=eps, log=lambda *_: None,
                                     features=lambda b: features(dev, seeds[id(b)]))
    assert len(eps) == 3 and np.isfinite(loss)
    inter = [dict() for _ in range(3)]
    union = [dict() for _ in range(3)]
    for e, b in zip(eps, loader):
        iut, _ = R.fuse_counts(e["pred_q"].double(), e["pred_q0"].double(), e["pred_q1"].double(), b[1])
        assert torch.equal(e["iut"].double(), iut)
        # validation resizes the support mask with align_corners=False (train_fuse.py:321), not the trainer's True
        lbl = b[3][0, 0]
        assert R.rel(e["s_mask"], R.support_mask(lbl, H // 2, False)) < R.TOL_FWD
        assert R.rel(R.support_mask(lbl, H // 2, True), R.support_mask(lbl, H // 2, False)) > R.SEPARATION
        for k, src in enumerate((1, 2, 0)):
            inter[k][e["cls"]] = inter[k].get(e["cls"], 0.0) + float(iut[src, 0, 1])
            union[k][e["cls"]] = union[k].get(e["cls"], 0.0) + float(iut[src, 1, 1])
    want = [float(np.mean([inter[k][c] / (union[k][c] + 1e-10) for c in union[k]])) for k in range(3)]
    assert len(union[0]) == 2   # two classes among the three episodes
    assert (m0, m1, m) == pytest.approx(tuple(want), abs=1e-12)
