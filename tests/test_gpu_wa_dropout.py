"""WeightAverage's training-mode dropouts on the device (cwt_weight_average_train_drop /
cwt_weight_average_backward_drop; src/model/msm/msm_func.py:63-64,90,100) against the float64
restatement tests/seg_loss_ref.weight_average_drop with both masks drawn by tests/dropout_ref.py
(att_drop: stream 6, index ((n h + y) w + x) 9 + r; proj_drop: stream 7, the NHWC linear index).
Bar: 1e-4 relative (max-norm), the project's gradient bar (tests/test_gpu_match_bwd.py)."""
import itertools

import pytest
import torch

import seg_loss_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-4
SHAPES = [(2, 64, 5, 7), (1, 128, 2, 3)]   # the second: every pixel touches the replicate border
NAMES = ["conv_theta.weight", "conv_theta.bias", "conv_phi.weight", "conv_phi.bias", "conv_g.weight",
         "conv_g.bias", "conv_back.weight", "conv_back.bias"]


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


@pytest.fixture
def seeds(monkeypatch):
    """few_shot_seg_cwt_amd.match.dropout_seed -> 7, 8, 9, ..."""
    import few_shot_seg_cwt_amd.match as match
    c = itertools.count(7)
    monkeypatch.setattr(match, "dropout_seed", lambda: next(c))


def _rand(shape, seed, lo=0.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g, dtype=torch.float64) * (hi - lo) + lo


def _module(dev, C, h, args):
    from few_shot_seg_cwt_amd.match import WeightAverage, init_match_params
    m = WeightAverage(C, args, device=dev)
    init_match_params(m, seed=C + h)
    return m


@pytest.mark.parametrize("N,C,h,w", SHAPES)
def test_forward_backward_with_both_masks(dev, seeds, N, C, h, w):
    m = _module(dev, C, h, dict(att_drop=0.5, proj_drop=0.5)).train()
    x0 = _rand((N, C, h, w), C)
    G = _rand((N, C, h, w), C + 1, -1, 1)
    x = x0.float().to(dev).requires_grad_(True)
    y = m(x)
    assert m.last_seed == 7
    (y * G.float().to(dev)).sum().backward()
    ma, mp = R.wa_masks(N, C, h, w, 0.5, 0.5, 7)
    # both masks are active: something dropped and something kept in each
    for name, mk in (("att", ma), ("proj", mp)):
        kept = float((mk > 0).double().mean())
        print(f"{name} mask kept fraction {kept:.3f}")
        assert 0.0 < kept < 1.0
    sd = {k: t.detach().cpu().double().requires_grad_(True) for k, t in m.state_dict().items()}
    xo = x0.clone().requires_grad_(True)
    yo = R.weight_average_drop(xo, tuple(sd[n] for n in NAMES), ma, mp)
    (yo * G).sum().backward()
    params = dict(m.named_parameters())
    errs = dict(y=rel(y, yo), dx=rel(x.grad, xo.grad))
    for n in NAMES:
        errs[n] = rel(params[n].grad, sd[n].grad)
    print(f"WeightAverage dropouts N={N} C={C} {h}x{w}: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) < TOL, errs
    # the masks change the result
    yn = R.weight_average_drop(x0, tuple(sd[n].detach() for n in NAMES), torch.ones_like(ma), torch.ones_like(mp))
    assert rel(y, yn) > 1e-3


@pytest.mark.parametrize("N,C,h,w", SHAPES)
def test_unchanged_paths(dev, seeds, N, C, h, w):
    """eval() with p = 0.5 is the p = 0 module bit for bit; train() with p = 0 is _WeightAverageFn."""
    from few_shot_seg_cwt_amd.match import _WeightAverageFn
    from few_shot_seg_cwt_amd.transformer import as_tokens
    md = _module(dev, C, h, dict(att_drop=0.5, proj_drop=0.5)).eval()
    m0 = _module(dev, C, h, dict(att_drop=0.0, proj_drop=0.0))
    x = _rand((N, C, h, w), C).float().to(dev)
    with torch.no_grad():
        assert torch.equal(md(x), m0.eval()(x))
    xg = x.clone().requires_grad_(True)
    y_eval_grad = md(xg)                      # eval under autograd: the no-dropout autograd path
    y_train0 = m0.train()(xg)
    ps = [getattr(getattr(m0, c), p) for c in ("conv_theta", "conv_phi", "conv_g", "conv_back")
          for p in ("weight", "bias")]
    want = _WeightAverageFn.apply(as_tokens(xg), *ps)
    assert torch.equal(y_train0, want) and torch.equal(y_eval_grad, want)
    assert m0.last_seed is None and md.last_seed is None      # no draw on either path


def test_host_rng_untouched(dev, N=2, C=64, h=5, w=7):
    """The real util.dropout_seed: the forward draws nothing from the host generator (the W0 stream)."""
    m = _module(dev, C, h, dict(att_drop=0.5, proj_drop=0.5)).train()
    x = _rand((N, C, h, w), C).float().to(dev)
    before = torch.get_rng_state()
    m(x)
    assert torch.equal(torch.get_rng_state(), before)
    assert m.last_seed is not None


def test_mmn_constructs_with_the_reference_config(dev, seeds):
    """config_files/pascal_mmn.yaml: wa True, att_drop 0.5, proj_drop 0.5 -> builds, and runs forward
    and backward at h = 6."""
    from few_shot_seg_cwt_amd.match import MMN, init_match_params
    args = dict(rmid="l34", layers=50, all_lr="l", att_wt=0.2, temp=20.0, conv4d="red", att_drop=0.5, proj_drop=0.5)
    net = MMN(args, agg="cat", wa=True, device=dev)
    init_match_params(net, 3)
    with torch.no_grad():   # keep the one-channel last layer's ReLU open somewhere (a live gradient)
        net.corr_net.NeighConsensus.conv[4].conv1.bias.add_(0.2)
    net.train()
    h = 6
    fq_lst = {3: [_rand((1, 1024, h, h), 1).float().to(dev)], 4: [_rand((1, 2048, h, h), 2).float().to(dev)]}
    fs_lst = {3: [_rand((1, 1024, h, h), 3).float().to(dev)], 4: [_rand((1, 2048, h, h), 4).float().to(dev)]}
    f_q, f_s = _rand((1, 512, h, h), 5).float().to(dev), _rand((1, 512, h, h), 6).float().to(dev)
    fq, att_fq = net(fq_lst, fs_lst, f_q, f_s)
    (fq.sum() + att_fq.sum()).backward()
    assert torch.isfinite(fq).all() and torch.isfinite(att_fq).all()
    g = net.wa_4.conv_back.weight.grad
    assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0
    assert net.wa_4.last_seed is not None and net.wa_3.last_seed is not None
