"""cwt_seg_head_loss (csrc/seg_loss.hip; few_shot_seg_cwt_amd/seg_loss.py): the classifier, the
bilinear align_corners upsample, SegLoss and the gradient to the feature map in one call, against
the float64 restatement tests/seg_loss_ref.py (src/model/pspnet.py:183-187,
src/model/model_util.py:9-73, src/train_kshot.py:168-183) differentiated by autograd.

Bars (the project's, tests/test_gpu_match_bwd.py): 1e-5 on loss values, 1e-4 relative (max-norm)
on gradients.  fp32 torch against float64 at these shapes is 1.5e-7 on the loss and 6e-7 on d_f,
so the bars leave room for another summation order and no more."""
import math

import pytest
import torch

import seg_loss_ref as R

pytestmark = pytest.mark.gpu

LOSS_TOL = 1e-5
GRAD_TOL = 1e-4
SHAPES = [(1, 512, 5, 33), (2, 64, 7, 49), (1, 512, 6, 50), (1, 512, 9, 65)]   # the third: S - 1 != 8 (h - 1)
LOSS_TYPES = ["wt_ce", "wt_dc", "ce"]


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _inputs(B, C, h, S, seed=0):
    g = torch.Generator().manual_seed(1000 * C + 10 * S + B + seed)
    W = (torch.rand(2, C, generator=g, dtype=torch.float64) * 2 - 1) / math.sqrt(C)
    f = torch.relu(torch.randn(B, C, h, h, generator=g, dtype=torch.float64))
    tgt = torch.randint(0, 2, (B, S, S), generator=g, dtype=torch.int64)
    tgt[:, 3:6, :] = 255
    return W, f, tgt


_REF = {}


def _ref(B, C, h, S, lt):
    """float64 loss, logits and d_f of one case (computed once)."""
    key = (B, C, h, S, lt)
    if key not in _REF:
        W, f, tgt = _inputs(B, C, h, S)
        fo = f.clone().requires_grad_(True)
        loss, lg = R.head_loss(W, fo, tgt, lt)
        loss.backward()
        _REF[key] = (loss.detach(), lg.detach(), fo.grad)
    return _REF[key]


def _run(dev, W, f, tgt, lt):
    from few_shot_seg_cwt_amd.seg_loss import seg_head_loss
    fd = f.float().to(dev).requires_grad_(True)
    loss, logits = seg_head_loss(W.float().to(dev), fd, tgt.to(dev), lt, return_logits=True)
    loss.backward()
    return loss.detach(), logits, fd.grad


@pytest.mark.parametrize("lt", LOSS_TYPES)
@pytest.mark.parametrize("B,C,h,S", SHAPES)
def test_parity(dev, B, C, h, S, lt):
    from few_shot_seg_cwt_amd.episode import classify
    W, f, tgt = _inputs(B, C, h, S)
    loss, logits, d_f = _run(dev, W, f, tgt, lt)
    lo, lgo, dfo = _ref(B, C, h, S, lt)
    fd = f.float().to(dev).contiguous(memory_format=torch.channels_last)
    want_lg = classify(W.float().to(dev).unsqueeze(0).expand(B, 2, C), fd)
    e_loss, e_df, e_lg = abs(float(loss) - float(lo)), rel(d_f, dfo), rel(logits, lgo)
    print(f"seg_head_loss {lt} B={B} C={C} h={h} S={S}: loss {float(loss):.7f} (ref {float(lo):.7f}, "
          f"err {e_loss:.1e}), d_f rel {e_df:.1e}, logits rel {e_lg:.1e}")
    assert torch.equal(logits, want_lg)          # the logits are cwt_classify's, bit for bit
    assert e_lg < GRAD_TOL
    assert e_loss < LOSS_TOL
    assert float(dfo.abs().max()) > 0 and e_df < GRAD_TOL


def test_names_map_to_the_reference_dispatch(dev):
    """SegLoss.forward (model_util.py:16-24): 'dc' is 'wt_dc'; an unknown name is 'wt_ce'."""
    from few_shot_seg_cwt_amd.seg_loss import SegLoss, seg_head_loss
    W, f, tgt = _inputs(1, 512, 5, 33)
    Wd, fd, td = W.float().to(dev), f.float().to(dev), tgt.to(dev)
    assert torch.equal(SegLoss("dc")(Wd, fd, td), seg_head_loss(Wd, fd, td, "wt_dc"))
    assert torch.equal(SegLoss("focal")(Wd, fd, td), seg_head_loss(Wd, fd, td, "wt_ce"))
    assert not torch.equal(SegLoss("ce")(Wd, fd, td), seg_head_loss(Wd, fd, td, "wt_ce"))


def test_dice_all_ignored_label(dev):
    """Every pixel 255: t = 0 in both channels, I = 0 -> loss exactly 2.0 and no gradient."""
    W, f, tgt = _inputs(1, 512, 5, 33)
    tgt[:] = 255
    loss, _, d_f = _run(dev, W, f, tgt, "wt_dc")
    assert float(loss) == 2.0
    assert float(d_f.abs().max()) == 0.0


def test_dice_no_foreground(dev):
    W, f, tgt = _inputs(1, 512, 5, 33)
    tgt[tgt == 1] = 0
    loss, _, d_f = _run(dev, W, f, tgt, "wt_dc")
    fo = f.clone().requires_grad_(True)
    lo, _ = R.head_loss(W, fo, tgt, "wt_dc")
    lo.backward()
    print(f"dice, no foreground: loss {float(loss):.7f} ref {float(lo):.7f}, d_f rel {rel(d_f, fo.grad):.1e}")
    assert math.isfinite(float(loss)) and abs(float(loss) - float(lo)) < LOSS_TOL
    assert rel(d_f, fo.grad) < GRAD_TOL


def test_dice_saturated_logits_hit_the_clamp(dev):
    """W = -40 |W|, f + 5, all-255 label: p underflows to 0, D = 0 < 1e-8 -> loss 2.0, zero gradient."""
    W, f, tgt = _inputs(1, 512, 5, 33)
    tgt[:] = 255
    loss, _, d_f = _run(dev, -40 * W.abs(), f + 5, tgt, "wt_dc")
    assert float(loss) == 2.0
    assert float(d_f.abs().max()) == 0.0


@pytest.mark.parametrize("lt", LOSS_TYPES)
def test_deterministic(dev, lt):
    W, f, tgt = _inputs(2, 64, 7, 49)
    l1, _, g1 = _run(dev, W, f, tgt, lt)
    l2, _, g2 = _run(dev, W, f, tgt, lt)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


def test_argument_errors(dev):
    from few_shot_seg_cwt_amd._lib import CwtError
    from few_shot_seg_cwt_amd.seg_loss import seg_head_loss
    tgt = torch.zeros((1, 33, 33), dtype=torch.int64, device=dev)
    with pytest.raises(CwtError):
        seg_head_loss(torch.zeros(2, 48, device=dev), torch.zeros(1, 48, 5, 5, device=dev), tgt, "wt_dc")
    with pytest.raises(CwtError):
        seg_head_loss(torch.zeros(2, 64, device=dev), torch.zeros(9, 64, 5, 5, device=dev),
                      tgt.expand(9, 33, 33).contiguous(), "wt_dc")
