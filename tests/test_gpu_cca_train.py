"""The class-incremental trainer's step and epoch on the device (few_shot_seg_cwt_amd/incremental.py
train_step / train_epoch; src/train_cca.py:119-256) and pred_q2 in validate_epoch, on the stub
model and MMN head of tests/test_gpu_incremental.py at h = 8, S = 57, 2 shots, 16 base classes.

Teacher-forced: from the device's own features and adapted W of each episode the step is recomputed
in float64 -- oracle/match_oracle.mmn_forward -> tests/cca_loss_ref.head_loss -> autograd ->
torch.optim.SGD + CosineAnnealingLR on a copy of the parameters.  Bars: the project's
(tests/test_gpu_mmn_train.py): 1e-5 on loss values, 1e-4 relative (max-norm) on every parameter."""
import numpy as np
import pytest
import torch

import cca_loss_ref as R

pytestmark = pytest.mark.gpu

TOL, LOSS_TOL = 1e-4, 1e-5
H, S, SHOT, NTR, C = 8, 57, 2, 16, 512


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _args(**kw):
    a = dict(layers=50, rmid="l34", all_lr="l", shot=SHOT, cls_lr=0.1, adapt_iter=5, tp=1.0, batch_size=1,
             num_classes_tr=NTR, loss_type="wt_dc", loss_shot="avg", aux=0.5, scheduler="cosine", epochs=1,
             att_wt=0.2, temp=20.0, conv4d="red", att_drop=0.0, proj_drop=0.0, main_optim="SGD", trans_lr=0.01,
             momentum=0.9, nesterov=True, weight_decay=1e-4, log_iter=0)
    # trans_lr: at 0.05 the two steps carry the last layer's one-element conv2.bias from -1.2e-2 to
    # 4e-5, where an absolute error of 1.4e-8 reads as 3e-4 relative to the parameter itself; at 0.01
    # no one-element parameter comes near zero and the relative max-norm means what it says
    a.update(kw)
    return a


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


class _StubModel:
    """extract_features as PSPNet's: (f [B,512,h,w], {layer: [features]}), from the image alone."""

    def __init__(self, h, dev):
        g = torch.Generator().manual_seed(3)
        self.h, self.proj = h, torch.randn(C, 3, generator=g).to(dev)
        self.p3, self.p4 = torch.randn(1024, 3, generator=g).to(dev), torch.randn(2048, 3, generator=g).to(dev)

    def eval(self):
        return self

    def extract_features(self, imgs):
        x = torch.nn.functional.adaptive_avg_pool2d(imgs, self.h)
        mk = lambda p: torch.einsum("kc,nchw->nkhw", p, x).contiguous(memory_format=torch.channels_last)  # noqa: E731
        # |.| and 0.12: post-ReLU-like features of a norm the inner loop's lr = 0.1 is stable at
        return 0.12 * mk(self.proj).abs(), {3: [mk(self.p3).abs()], 4: [mk(self.p4).abs()]}


def _trans(dev, args):
    from few_shot_seg_cwt_amd.match import MMN, init_match_params
    net = MMN(args, agg="cat", wa=True, red_dim=False, device=dev)
    init_match_params(net, seed=5)
    with torch.no_grad():   # keep the one-channel last layer's ReLU open somewhere (a live gradient)
        net.corr_net.NeighConsensus.conv[4].conv1.bias.add_(0.2)
    return net


def _loader(classes, seed=77):
    g = torch.Generator().manual_seed(seed)
    lab = lambda *shape: torch.tensor([0, 1, 255])[torch.multinomial(  # noqa: E731
        torch.tensor([0.6, 0.3, 0.1]), int(np.prod(shape)), True, generator=g)].reshape(shape)
    # blocky images: the stub's pooled features then differ from cell to cell, so the supports'
    # pseudo-labels spread over the base classes (a flat image relabels every pixel alike, and the
    # inner loop's bg / fg weight is 0 / n)
    img = lambda *lead: torch.rand(*lead, 3, H, H, generator=g).repeat_interleave(8, -2).repeat_interleave(  # noqa: E731
        8, -1)[..., :S, :S].contiguous()
    return [(img(1), lab(1, S, S), img(1, SHOT), lab(1, SHOT, S, S), [torch.tensor(cls)], None, None)
            for cls in classes]


def _train(dev, args, classes=(3, 7)):
    from few_shot_seg_cwt_amd.incremental import train_epoch
    from few_shot_seg_cwt_amd.mmn_train import get_scheduler
    from few_shot_seg_cwt_amd.optimizer import get_optimizer
    torch.manual_seed(11)
    Trans = _trans(dev, args)
    start = {k: v.detach().cpu().double().clone() for k, v in Trans.state_dict().items()}
    opt = get_optimizer(args, [dict(params=list(Trans.parameters()), lr=args["trans_lr"])])
    loader = _loader(classes)
    sch = get_scheduler(args, opt, len(loader))
    g = torch.Generator().manual_seed(5)
    W_base = (0.3 * torch.randn(NTR, C, generator=g)).to(dev)
    recs, lines = [], []
    res = train_epoch(args, loader, _StubModel(H, dev), Trans, W_base, opt, sch, 1, log=lines.append, records=recs)
    return Trans, start, recs, lines, res


@pytest.fixture(scope="module")
def trained(dev):
    return _train(dev, _args())


def test_teacher_forced_step(dev, trained):
    from oracle import match_oracle as M
    args = _args()
    Trans, start, recs, lines, _ = trained
    assert len(recs) == 2 and all(bool(torch.isfinite(r["W"]).all()) for r in recs)
    assert [r["idx_cls"] for r in recs] == [3, 7] and all(r["W"].shape == (NTR, C) for r in recs)
    names = [n for n, _ in Trans.named_parameters()]
    sd = {k: v.clone().requires_grad_(k in names) for k, v in start.items()}
    opt = torch.optim.SGD([sd[n] for n in names], lr=args["trans_lr"], momentum=0.9, nesterov=True, weight_decay=1e-4)
    sch = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 2 * args["epochs"], eta_min=1e-6)
    d = lambda t: t.detach().double().cpu()  # noqa: E731
    for step, r in enumerate(recs):
        wa = {b: M.wa_params_from_state(sd, f"wa_{b}.") for b in (3, 4)}
        layers = M.layers_from_state(sd, prefix="corr_net.NeighConsensus.conv.")
        fq, att_fq = M.mmn_forward({k: d(v[0]) for k, v in r["fq_lst"].items()},
                                   {k: d(v[0]) for k, v in r["fs_lst"].items()}, d(r["f_q"]), d(r["f_s"]), [3, 4], wa,
                                   layers, 20.0, 0.2)
        W, ql, idx = d(r["W"]), r["q_label"].cpu(), r["idx_cls"]
        l1, _ = R.head_loss(W, att_fq, ql, idx, "wt_dc")
        l, _ = R.head_loss(W, fq, ql, idx, "wt_dc")
        l0, _ = R.head_loss(W, d(r["f_q"]), ql, idx, "wt_dc")
        f1, f0 = float(l1.detach()), float(l.detach())
        e1, e = abs(float(r["q_loss1"]) - f1), abs(float(r["q_loss"]) - f0)
        print(f"step {step + 1}: q_loss1 {float(r['q_loss1']):.7f} (ref {f1:.7f}), q_loss {float(r['q_loss']):.7f} "
              f"(ref {f0:.7f}), q_loss0 {float(r['q_loss0']):.7f} (ref {float(l0):.7f})")
        assert e1 < LOSS_TOL and e < LOSS_TOL
        assert abs(float(r["q_loss0"]) - float(l0)) < LOSS_TOL
        opt.zero_grad()
        (l1 + 0.5 * l).backward()
        opt.step()
        sch.step()
    got = dict(Trans.named_parameters())
    errs = {n: rel(got[n], sd[n]) for n in names}
    moved = {n: rel(sd[n], start[n]) for n in names}
    print("parameters after step 2: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    worst = max(errs, key=errs.get)
    print(f"worst: {worst} {errs[worst]:.1e}, |value| max {float(sd[worst].abs().max()):.3e} "
          f"(start {float(start[worst].abs().max()):.3e}), abs err {float((d(got[worst]) - d(sd[worst])).abs().max()):.1e}")
    assert max(moved.values()) > 1e-3          # the step moved the parameters
    assert max(errs.values()) < TOL, errs


def test_meters_and_log_lines(dev, trained):
    _, _, recs, lines, res = trained
    def iou(t):   # (IoUf + IoUb) / 2, as the epoch forms it
        t = t.cpu().numpy()[0]
        v = t[0] / (t[1] + 1e-10)
        return (v[1] + v[0]) / 2

    want = (np.mean([iou(r["iut0"]) for r in recs]), np.mean([iou(r["iut1"]) for r in recs]),
            np.mean([float(r["q_loss0"]) for r in recs]), np.mean([float(r["q_loss1"]) for r in recs]))
    assert res == pytest.approx(want, rel=1e-12)
    assert lines and "===========Epoch 1===========: The mIoU0" in lines[-1]
    # the head's iut is the p > 0.5 mask of its own logits against the label
    for r in recs:
        for key, lg in (("iut0", "pred_q0"), ("iut1", "pred_q1"), ("iut", "pred_q")):
            hi = R.upsample(r[lg].cpu().double(), S)
            if R.half_share(hi, r["idx_cls"]) == 0.0:
                assert torch.equal(r[key].cpu().double(), R.iut_half(hi, r["q_label"].cpu(), r["idx_cls"]))


def test_log_lines_of_a_longer_epoch(dev):
    """20 episodes with a cheap step: the reference's 'Ep1/20 ...' line (epoch 1, i % 20 == 0), with
    auxL, and the CompareMeter line and val_hook at i % log_iter == 1."""
    calls = []
    from few_shot_seg_cwt_amd.incremental import train_epoch
    from few_shot_seg_cwt_amd.mmn_train import get_scheduler
    from few_shot_seg_cwt_amd.optimizer import get_optimizer
    args = _args(adapt_iter=1, log_iter=8)
    Trans = _trans(dev, args)
    opt = get_optimizer(args, [dict(params=list(Trans.parameters()), lr=args["trans_lr"])])
    one = _loader((16,))
    loader = one * 20
    lines = []
    g = torch.Generator().manual_seed(5)
    W_base = (0.3 * torch.randn(NTR, C, generator=g)).to(dev)
    recs = []
    train_epoch(args, loader, _StubModel(H, dev), Trans, W_base, opt, get_scheduler(args, opt, 20), 1,
                log=lines.append, records=recs, val_hook=lambda: calls.append(1))
    assert recs[0]["W"].shape == (NTR + 1, C)   # idx_cls = 16: a 17-row classifier
    ep = [ln for ln in lines if ln.startswith("Ep1/20 IoUf0 ")]
    assert len(ep) == 1 and " loss0 " in ep[0] and " lr " in ep[0] and "auxL " in ep[0]
    cmp_lines = [ln for ln in lines if ln.startswith("------Ep1/") and "FG IoU1 compared to IoU0 win" in ln]
    assert [ln.split()[0] for ln in cmp_lines] == ["------Ep1/1", "------Ep1/9", "------Ep1/17"]
    assert len(calls) == 3
    assert "win 0/1" in cmp_lines[0] or "win 1/1" in cmp_lines[0]
    assert "/8 avg diff" in cmp_lines[1]


def test_validate_epoch_pred_q2(dev):
    from few_shot_seg_cwt_amd.incremental import validate_epoch
    args = _args()
    net = _trans(dev, args).eval()
    loader = _loader((3, 7, 3), seed=78)
    g = torch.Generator().manual_seed(5)
    W_base = (0.3 * torch.randn(NTR, C, generator=g)).to(dev)
    eps = []
    res = validate_epoch(args, loader, _StubModel(H, dev), W_base, net, episodes_out=eps)
    assert len(eps) == 3 and all("iut2" in e for e in eps)
    iut = [e["iut2"].cpu().double()[0] for e in eps]
    want = {3: float((iut[0][0, 1] + iut[2][0, 1]) / (iut[0][1, 1] + iut[2][1, 1] + 1e-10)),
            7: float(iut[1][0, 1] / (iut[1][1, 1] + 1e-10))}
    assert res["class_iou2"] == pytest.approx(want, rel=1e-12)
    assert res["mIoU2"] == pytest.approx(np.mean(list(want.values())), rel=1e-12)
    # iut2 is the float64 mix mask of the episode's own pred_q0 and pred_q1 (near-ties apart)
    for e, batch in zip(eps, loader):
        hi0, hi1 = R.upsample(e["pred_q0"].cpu().double(), S), R.upsample(e["pred_q1"].cpu().double(), S)
        near, ties = R.mix_gap_share(R.mix(hi0, hi1, 0.2))
        if near == 0.0 and ties == 0.0:
            assert torch.equal(e["iut2"].cpu().double(), R.iut_of_mask(R.mix_mask(hi0, hi1, 0.2, NTR), batch[1]))


def test_loss_shot_sum_is_refused(dev):
    from few_shot_seg_cwt_amd.incremental import train_step
    args = _args(loss_shot="sum")
    with pytest.raises(NotImplementedError, match="loss_shot"):
        train_step(args, _StubModel(H, dev), None, None, None, _loader((3,))[0], torch.zeros(NTR, C, device=dev), dev)
