"""MMN over every bottleneck's features (mmn.py:42-71 with all_lr naming layers: one correlation channel
per (layer, block) pair, the deepest layer first, its blocks ascending; one wa_ / rd_ module per layer,
shared by the layer's blocks) and the MMN trainer's step on them.  Against a float64 loop written here
from oracle/match_oracle.py's weight_average and corr_forward.  Bars: the project's for the same
quantities -- 2e-5 forward (tests/test_gpu_match.py), 1e-4 gradients (tests/test_gpu_match_bwd.py), and
for the trainer 1e-4 on the parameters after two steps, 1e-5 on the losses (tests/test_gpu_mmn_train.py)."""
import pytest
import torch
import torch.nn.functional as F

import seg_loss_ref as R

pytestmark = pytest.mark.gpu

FWD_TOL, TOL, LOSS_TOL = 2e-5, 1e-4, 1e-5
CH = {2: 512, 3: 1024, 4: 2048}
NB50 = {2: 4, 3: 6, 4: 3}


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _rand(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g, dtype=torch.float64) * (hi - lo) + lo


def mmn_oracle(fq_lst, fs_lst, f_q, f_s, bid_lst, wa, layers, temp, att_wt, agg="cat", rdw=None):
    """mmn.py:42-71 in float64 over lists of features per layer."""
    from oracle import match_oracle as M
    B, ch, h, w = f_s.shape
    corrs = []
    for idx in bid_lst[::-1]:
        for lr in range(len(fq_lst[idx])):
            fq, fs = fq_lst[idx][lr].expand(B, -1, -1, -1), fs_lst[idx][lr]
            if rdw is not None:
                fq, fs = torch.relu(F.conv2d(fq, rdw[idx])), torch.relu(F.conv2d(fs, rdw[idx]))
            if wa is not None:
                fq, fs = M.weight_average(fq, wa[idx]), M.weight_average(fs, wa[idx])
            bq = F.normalize(fq.reshape(B, fq.shape[1], h * w), dim=1)
            bs = F.normalize(fs.reshape(B, fs.shape[1], h * w), dim=1)
            corrs.append(torch.bmm(bq.transpose(1, 2), bs).reshape(B, 1, h, w, h, w))
    corr4d = torch.cat(corrs, 1)
    if agg == "sum":
        corr4d = torch.sum(corr4d, dim=1, keepdim=True)
    _, att = M.corr_forward(corr4d, f_s, layers, temp, True)
    att = att.mean(dim=0, keepdim=True)
    return f_q * (1 - att_wt) + att * att_wt, att, corr4d.shape[1]


def _oracle_params(sd, red_dim):
    from oracle import match_oracle as M
    wa = {b: M.wa_params_from_state(sd, f"wa_{b}.") for b in (3, 4)}
    rdw = {b: sd[f"rd_{b}.0.weight"] for b in (3, 4)} if red_dim else None
    return wa, rdw, M.layers_from_state(sd, prefix="corr_net.NeighConsensus.conv.")


def _net(dev, agg, red_dim, seed, att_wt=0.2):
    from few_shot_seg_cwt_amd.match import MMN, init_match_params
    args = dict(rmid="l34", layers=50, all_lr="34", temp=20.0, att_wt=att_wt, conv4d="red")
    net = MMN(args, agg=agg, wa=True, red_dim=red_dim, device=dev)
    init_match_params(net, seed=seed)
    with torch.no_grad():   # keep the one-channel last layer's ReLU open somewhere (a live gradient)
        net.corr_net.NeighConsensus.conv[4].conv1.bias.add_(0.2)
    return net


def _feats(h, B, seed):
    """Random layer features as test_mmn_forward's: six blocks of layer3, three of layer4."""
    fq = {k: [_rand((1, CH[k], h, h), seed + 10 * k + b) for b in range(NB50[k])] for k in (3, 4)}
    fs = {k: [_rand((B, CH[k], h, h), seed + 100 + 10 * k + b) for b in range(NB50[k])] for k in (3, 4)}
    return fq, fs, _rand((1, 512, h, h), seed + 1), _rand((B, 512, h, h), seed + 2)


def _to(dev, lst, grad=False):
    return {k: [t.float().to(dev).requires_grad_(grad) for t in v] for k, v in lst.items()}


@pytest.mark.parametrize("agg,red_dim", [("cat", False), ("sum", False), ("cat", 64)])
def test_mmn_forward_every_block(dev, agg, red_dim):
    net = _net(dev, agg, red_dim, seed=5)
    assert net.corr_net.in_channel == (1 if agg == "sum" else 9)
    h, B = 6, 2
    fq0, fs0, f_q, f_s = _feats(h, B, 23)
    with torch.no_grad():
        fq, att_fq = net(_to(dev, fq0), _to(dev, fs0), f_q.float().to(dev), f_s.float().to(dev))
    sd = {k: t.detach().cpu().double() for k, t in net.state_dict().items()}
    wa, rdw, layers = _oracle_params(sd, red_dim)
    fqo, atto, L = mmn_oracle(fq0, fs0, f_q, f_s, [3, 4], wa, layers, 20.0, 0.2, agg, rdw)
    assert L == net.corr_net.in_channel
    errs = dict(fq=rel(fq, fqo), att_fq=rel(att_fq, atto))
    print(f"MMN.forward every block agg={agg} red_dim={red_dim}: {errs}")
    assert max(errs.values()) < FWD_TOL, errs


def test_mmn_backward_every_block(dev):
    """Gradients of a linear functional of (fq, att_fq) with respect to every MMN parameter -- wa_3's
    receive six blocks' worth, wa_4's three -- the support feature map f_s and the layer features; the
    no-grad forward gives the autograd forward's bits."""
    net = _net(dev, "cat", False, seed=9, att_wt=0.3)
    h, B = 6, 2
    fq0, fs0, f_q0, f_s0 = _feats(h, B, 31)
    G1, G2 = _rand((1, 512, h, h), 37, -1, 1), _rand((1, 512, h, h), 38, -1, 1)
    fq_d, fs_d = _to(dev, fq0, True), _to(dev, fs0, True)
    f_q, f_s = f_q0.float().to(dev), f_s0.float().to(dev).requires_grad_(True)
    fq, att_fq = net(fq_d, fs_d, f_q, f_s)
    ((fq * G1.float().to(dev)).sum() + (att_fq * G2.float().to(dev)).sum()).backward()
    with torch.no_grad():
        plain = net(_to(dev, fq0), _to(dev, fs0), f_q, f_s.detach())
    for a, b in zip(plain, (fq, att_fq)):
        assert torch.equal(a, b.detach())
    sd = {k: t.detach().cpu().double().requires_grad_(True) for k, t in net.state_dict().items()}
    wa, _, layers = _oracle_params(sd, False)
    fq_o = {k: [t.clone().requires_grad_(True) for t in v] for k, v in fq0.items()}
    fs_o = {k: [t.clone().requires_grad_(True) for t in v] for k, v in fs0.items()}
    f_so = f_s0.clone().requires_grad_(True)
    fqo, atto, _ = mmn_oracle(fq_o, fs_o, f_q0, f_so, [3, 4], wa, layers, 20.0, 0.3)
    ((fqo * G1).sum() + (atto * G2).sum()).backward()
    errs = dict(fq=rel(fq, fqo), att_fq=rel(att_fq, atto), d_f_s=rel(f_s.grad, f_so.grad))
    for k in (3, 4):
        for b in range(NB50[k]):
            errs[f"d_fq{k}.{b}"] = rel(fq_d[k][b].grad, fq_o[k][b].grad)
            errs[f"d_fs{k}.{b}"] = rel(fs_d[k][b].grad, fs_o[k][b].grad)
    names = [n for n, _ in net.named_parameters()]
    assert any(n.startswith("wa_3.") for n in names) and any(n.startswith("wa_4.") for n in names)
    for n, p in net.named_parameters():
        assert float(sd[n].grad.abs().max()) > 0, n
        errs[n] = rel(p.grad, sd[n].grad)
    print("MMN backward every block: " + ", ".join(f"{k} {e:.1e}" for k, e in errs.items()))
    assert max(errs.values()) < TOL, errs


# ---- the trainer (mmn_train.train_step) at S = 65, R50, rmid l34, all_lr '4': 3 + 1 = 4 channels, one shot ----
S, SHOT = 65, 1


def _args(**kw):
    a = dict(layers=50, rmid="l34", all_lr="4", shot=SHOT, image_size=S, cls_lr=0.1, adapt_iter=20, batch_size=1,
             loss_type="wt_dc", loss_shot="avg", aux=0.5, scheduler="cosine", epochs=1, att_wt=0.2, temp=20.0,
             conv4d="red", att_drop=0.0, proj_drop=0.0, main_optim="SGD", trans_lr=0.05, momentum=0.9, nesterov=True,
             weight_decay=1e-4, log_iter=0, test_num=3)
    a.update(kw)
    return a


@pytest.fixture(scope="module")
def model(dev):
    from few_shot_seg_cwt_amd import PSPNet
    from few_shot_seg_cwt_amd import synthetic as syn
    net = PSPNet(dict(layers=50, rmid="l34", all_lr="4"))
    net.load_state_dict(syn.make_pspnet_state(50, 2021))
    return net


@pytest.mark.parametrize("loss_shot", ["avg", "sum"])
def test_trainer_two_steps_every_block(dev, model, loss_shot):
    """Two train_step calls recomputed in float64 from the device's own features and adapted W, as
    tests/test_gpu_mmn_train.py does ('sum' with one shot: the per-shot slicing over a multi-block list
    gives the same losses)."""
    from few_shot_seg_cwt_amd.episode import SyntheticEpisodes
    from few_shot_seg_cwt_amd.match import MMN, init_match_params
    from few_shot_seg_cwt_amd.mmn_train import get_scheduler, train_epoch
    from few_shot_seg_cwt_amd.optimizer import get_optimizer
    from oracle import match_oracle as M
    args = _args(loss_shot=loss_shot)
    torch.manual_seed(11)
    Trans = MMN(args, agg="cat", wa=True, device=dev)
    assert Trans.corr_net.in_channel == 4
    init_match_params(Trans, seed=5)
    with torch.no_grad():
        Trans.corr_net.NeighConsensus.conv[4].conv1.bias.add_(0.2)
    start = {k: v.detach().cpu().double().clone() for k, v in Trans.state_dict().items()}
    opt = get_optimizer(args, [dict(params=list(Trans.parameters()), lr=args["trans_lr"])])
    sch = get_scheduler(args, opt, 2)
    recs = []
    train_epoch(args, SyntheticEpisodes(2, S=S, shot=SHOT), model, Trans, opt, sch, 1, log=lambda s: None, records=recs)
    assert len(recs) == 2
    assert {k: len(v) for k, v in recs[0]["fq_lst"].items()} == {2: 1, 3: 1, 4: 3}
    names = [n for n, _ in Trans.named_parameters()]
    sd = {k: v.clone().requires_grad_(k in names) for k, v in start.items()}
    ropt = torch.optim.SGD([sd[n] for n in names], lr=args["trans_lr"], momentum=0.9, nesterov=True, weight_decay=1e-4)
    rsch = torch.optim.lr_scheduler.CosineAnnealingLR(ropt, 2 * args["epochs"], eta_min=1e-6)
    d = lambda t: t.detach().double().cpu()  # noqa: E731
    for step, r in enumerate(recs):
        wa = {b: M.wa_params_from_state(sd, f"wa_{b}.") for b in (3, 4)}
        layers = M.layers_from_state(sd, prefix="corr_net.NeighConsensus.conv.")
        fq, att_fq, L = mmn_oracle({k: [d(t) for t in v] for k, v in r["fq_lst"].items()},
                                   {k: [d(t) for t in v] for k, v in r["fs_lst"].items()}, d(r["f_q"]), d(r["f_s"]),
                                   [3, 4], wa, layers, 20.0, 0.2)
        assert L == 4
        W, ql = d(r["W"]), r["q_label"].cpu()
        l1, _ = R.head_loss(W, att_fq, ql, "wt_dc")
        l, _ = R.head_loss(W, fq, ql, "wt_dc")
        f1, f0 = float(l1.detach()), float(l.detach())
        e1, e = abs(float(r["q_loss1"]) - f1), abs(float(r["q_loss"]) - f0)
        print(f"{loss_shot} step {step + 1}: q_loss1 {float(r['q_loss1']):.7f} (ref {f1:.7f}, err {e1:.1e}), "
              f"q_loss {float(r['q_loss']):.7f} (ref {f0:.7f}, err {e:.1e})")
        assert e1 < LOSS_TOL and e < LOSS_TOL
        ropt.zero_grad()
        (l1 + 0.5 * l).backward()
        ropt.step()
        rsch.step()
    got = dict(Trans.named_parameters())
    errs = {n: rel(got[n], sd[n]) for n in names}
    moved = {n: rel(sd[n], start[n]) for n in names}
    print(f"{loss_shot}: parameters after step 2: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(moved.values()) > 1e-3          # the step moved the parameters
    assert max(errs.values()) < TOL, errs
