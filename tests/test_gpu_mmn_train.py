"""The MMN trainer's step and validation on the device (few_shot_seg_cwt_amd/mmn_train.py;
src/train_kshot.py:119-192, 254-356) on the synthetic R50 state at S = 65 (h = 9), 2 shots.

Teacher-forced: from the device's own features, mid features and adapted W of each episode the
step is recomputed in float64 -- oracle/match_oracle.mmn_forward -> tests/seg_loss_ref.head_loss
-> autograd -> torch.optim.SGD + CosineAnnealingLR on a copy of the parameters.  Bars: the
project's (tests/test_gpu_match_bwd.py): 1e-4 relative (max-norm) on every parameter, 1e-5 on
loss values; 2e-5 on the heads' forward logits (tests/test_gpu_match.py)."""
import itertools

import numpy as np
import pytest
import torch

import seg_loss_ref as R

TOL, LOSS_TOL, FWD_TOL = 1e-4, 1e-5, 2e-5
S, SHOT = 65, 2


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _args(**kw):
    a = dict(layers=50, rmid="l34", all_lr="l", shot=SHOT, image_size=S, cls_lr=0.1, adapt_iter=20, batch_size=1,
             loss_type="wt_dc", loss_shot="avg", aux=0.5, scheduler="cosine", epochs=1, att_wt=0.2, temp=20.0,
             conv4d="red", att_drop=0.0, proj_drop=0.0, main_optim="SGD", trans_lr=0.05, momentum=0.9, nesterov=True,
             weight_decay=1e-4, log_iter=0, test_num=3)
    a.update(kw)
    return a


def test_scheduler_cosine_matches_torch():
    """get_scheduler 'cosine' over 10 steps against CosineAnnealingLR on a CPU optimiser."""
    from few_shot_seg_cwt_amd.mmn_train import get_scheduler

    class Opt:
        lr = 0.05
    opt = Opt()
    sch = get_scheduler(dict(scheduler="cosine", epochs=2), opt, batches=5)
    p = torch.nn.Parameter(torch.zeros(1))
    topt = torch.optim.SGD([p], lr=0.05)
    tsch = torch.optim.lr_scheduler.CosineAnnealingLR(topt, 10, eta_min=1e-6)
    for _ in range(10):
        topt.step()
        tsch.step()
        sch.step()
        want = topt.param_groups[0]["lr"]
        assert abs(opt.lr - want) <= 1e-9 * want, (opt.lr, want)
    assert get_scheduler(dict(scheduler=None), opt, 5) is None


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def model(dev):
    from few_shot_seg_cwt_amd import PSPNet
    from few_shot_seg_cwt_amd import synthetic as syn
    net = PSPNet(dict(layers=50, rmid="l34", all_lr="l"))
    net.load_state_dict(syn.make_pspnet_state(50, 2021))
    return net


def _trans(dev, args):
    from few_shot_seg_cwt_amd.match import MMN, init_match_params
    net = MMN(args, agg="cat", wa=True, device=dev)
    init_match_params(net, seed=5)
    with torch.no_grad():   # keep the one-channel last layer's ReLU open somewhere (a live gradient)
        net.corr_net.NeighConsensus.conv[4].conv1.bias.add_(0.2)
    return net


def _train(dev, model, args, n_steps=2, seed=11):
    from few_shot_seg_cwt_amd.episode import SyntheticEpisodes
    from few_shot_seg_cwt_amd.mmn_train import get_scheduler, train_epoch
    from few_shot_seg_cwt_amd.optimizer import get_optimizer
    torch.manual_seed(seed)
    Trans = _trans(dev, args)
    start = {k: v.detach().cpu().double().clone() for k, v in Trans.state_dict().items()}
    opt = get_optimizer(args, [dict(params=list(Trans.parameters()), lr=args["trans_lr"])])
    sch = get_scheduler(args, opt, n_steps)
    recs, lines = [], []
    train_epoch(args, SyntheticEpisodes(n_steps, S=S, shot=SHOT), model, Trans, opt, sch, 1, log=lines.append,
                records=recs)
    return Trans, start, recs, lines


@pytest.mark.gpu
def test_teacher_forced_step(dev, model):
    from oracle import match_oracle as M
    args = _args()
    Trans, start, recs, lines = _train(dev, model, args)
    assert len(recs) == 2 and lines and "Epoch 1" in lines[-1]
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
        W, ql = d(r["W"]), r["q_label"].cpu()
        l1, _ = R.head_loss(W, att_fq, ql, "wt_dc")
        l, _ = R.head_loss(W, fq, ql, "wt_dc")
        f1, f0 = float(l1.detach()), float(l.detach())
        e1, e = abs(float(r["q_loss1"]) - f1), abs(float(r["q_loss"]) - f0)
        print(f"step {step + 1}: q_loss1 {float(r['q_loss1']):.7f} (ref {f1:.7f}), q_loss {float(r['q_loss']):.7f} "
              f"(ref {f0:.7f})")
        assert e1 < LOSS_TOL and e < LOSS_TOL
        opt.zero_grad()
        (l1 + 0.5 * l).backward()
        opt.step()
        sch.step()
    got = dict(Trans.named_parameters())
    errs = {n: rel(got[n], sd[n]) for n in names}
    moved = {n: rel(sd[n], start[n]) for n in names}
    print("parameters after step 2: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(moved.values()) > 1e-3          # the step moved the parameters
    assert max(errs.values()) < TOL, errs


@pytest.mark.gpu
def test_dropouts_change_the_step_and_repeat_bitwise(dev, model, monkeypatch):
    import few_shot_seg_cwt_amd.match as match

    def run(p):
        c = itertools.count(7)
        monkeypatch.setattr(match, "dropout_seed", lambda: next(c))
        Trans, _, recs, _ = _train(dev, model, _args(att_drop=p, proj_drop=p))
        return {k: v.detach().clone() for k, v in Trans.state_dict().items()}, recs

    plain, _ = run(0.0)
    a, recs = run(0.5)
    b, _ = run(0.5)
    assert all(np.isfinite(float(r["q_loss1"])) and np.isfinite(float(r["q_loss"])) for r in recs)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert any(not torch.equal(a[k], plain[k]) for k in a)


@pytest.mark.gpu
def test_validate_epoch(dev, model):
    from few_shot_seg_cwt_amd.episode import EpisodeEngine, SyntheticEpisodes
    from few_shot_seg_cwt_amd.mmn_train import validate_epoch
    from few_shot_seg_cwt_amd import MultiHeadAttentionOne
    from oracle import match_oracle as M
    args = _args()
    Net = _trans(dev, args)
    loader = SyntheticEpisodes(3, S=S, shot=SHOT)
    eps, lines = [], []
    torch.manual_seed(3)
    mIoU, mIoU1, loss = validate_epoch(args, loader, model, Net, episodes_out=eps, log=lines.append)
    assert len(eps) == 3 and np.isfinite(loss)
    # the returned mIoUs are those of the records' counts
    for key, want in (("iut", mIoU), ("iut1", mIoU1)):
        inter, union = {}, {}
        for r in eps:
            inter[r["cls"]] = inter.get(r["cls"], 0.0) + float(r[key][0, 0, 1])
            union[r["cls"]] = union.get(r["cls"], 0.0) + float(r[key][0, 1, 1])
        assert want == float(np.mean([inter[c] / (union[c] + 1e-10) for c in union]))
    # pred_q1 / pred_q against the oracle chain on the device's own features and adapted W
    sd = {k: t.detach().cpu().double() for k, t in Net.state_dict().items()}
    wa = {b: M.wa_params_from_state(sd, f"wa_{b}.") for b in (3, 4)}
    layers = M.layers_from_state(sd, prefix="corr_net.NeighConsensus.conv.")
    d = lambda t: t.detach().double().cpu()  # noqa: E731
    engine = EpisodeEngine(model, MultiHeadAttentionOne(4, 512, 512, 512, dropout=0.5).eval(), args)
    torch.manual_seed(3)   # after the CWT's own parameter draws: the W0 sequence validate_epoch saw
    it = iter(loader)
    for i, r in enumerate(eps):
        qry_img, q_label, spt_imgs, s_label = it.next()[:4]
        imgs = torch.cat([spt_imgs[0], qry_img], 0).to(dev)
        f_all, lst = model.extract_features(imgs)
        fqo, atto = M.mmn_forward({k: d(v[0][SHOT:]) for k, v in lst.items()}, {k: d(v[0][:SHOT]) for k, v in lst.items()},
                                  d(f_all[SHOT:]), d(f_all[:SHOT]), [3, 4], wa, layers, 20.0, 0.2)
        e1 = rel(r["pred_q1"], R.head_logits(r["W"].double(), atto))
        e = rel(r["pred_q"], R.head_logits(r["W"].double(), fqo))
        print(f"validate_epoch episode {i}: pred_q1 {e1:.1e} pred_q {e:.1e}")
        assert e1 < FWD_TOL and e < FWD_TOL
        # pred_q0's counts are the inference engine's baseline counts (same W0 draw from the host RNG)
        from few_shot_seg_cwt_amd.episode import new_binary_classifier_weight
        W0 = new_binary_classifier_weight().to(dev)
        out = engine.run(imgs, s_label[0].to(dev).long(), q_label.to(dev).long(), W0)
        assert torch.equal(out["iut0"].cpu(), r["iut0"])
