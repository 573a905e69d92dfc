"""cwt_seg_head_loss_nway (csrc/seg_loss_nway.hip; few_shot_seg_cwt_amd/seg_loss.py): the N-way
classifier, the bilinear align_corners upsample, compress_pred, SegLoss(., 'pb') and the gradient
to the feature map in one call (src/train_cca.py:177-198), against the float64 restatement
tests/cca_loss_ref.py differentiated by autograd.

Bars (the project's, tests/test_gpu_seg_head_loss.py, tests/test_gpu_match_bwd.py): 1e-5 on loss
values, 1e-4 relative (max-norm) on gradients, 2e-5 on forward logits.  fp32 torch of the same
formula stays within 1.5e-7 on the loss and 2.5e-6 on d_f at these shapes and logit scales
(tests/test_cca_loss_ref_cpu.py asserts the bars for it), so the bars leave room for another
summation order and no more.  The draws are clear of p = 0.5 by 1e-4 in float64, so the iut counts
are demanded exactly."""
import math

import pytest
import torch

import cca_loss_ref as R

pytestmark = pytest.mark.gpu

LOSS_TOL, GRAD_TOL, FWD_TOL = 1e-5, 1e-4, 2e-5


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _run(dev, W, f, tgt, idx, lt):
    from few_shot_seg_cwt_amd.seg_loss import seg_head_loss_nway
    fd = f.float().to(dev).requires_grad_(True)
    loss, logits, iut = seg_head_loss_nway(W.float().to(dev), fd, tgt.to(dev), idx, lt, return_logits=True,
                                           return_iut=True)
    loss.backward()
    return loss.detach(), logits, fd.grad, iut


@pytest.mark.parametrize("lt", R.LOSS_TYPES)
@pytest.mark.parametrize("scale", R.SCALES)
@pytest.mark.parametrize("case", R.CASES)
def test_parity(dev, case, scale, lt):
    from few_shot_seg_cwt_amd.incremental import classify_nway
    B, N, idx, C, h, S = case
    W, f, tgt = R.inputs(case, scale)
    loss, logits, d_f, iut = _run(dev, W, f, tgt, idx, lt)
    lo, lgo, dfo, iuto = R.reference(case, scale, lt)
    want_lg = classify_nway(W.float().to(dev), f.float().to(dev).contiguous(memory_format=torch.channels_last))
    e_loss, e_df, e_lg = abs(float(loss) - float(lo)), rel(d_f, dfo), rel(logits, lgo)
    print(f"seg_head_loss_nway {lt} {case} scale {scale}: loss {float(loss):.7f} (ref {float(lo):.7f}, "
          f"err {e_loss:.1e}), d_f rel {e_df:.1e}, logits rel {e_lg:.1e}")
    assert torch.equal(logits, want_lg)          # the logits are cwt_linear's, bit for bit
    assert e_lg < FWD_TOL
    assert e_loss < LOSS_TOL
    assert float(dfo.abs().max()) > 0 and e_df < GRAD_TOL
    assert torch.equal(iut.cpu().double(), iuto)


def test_no_grad_call_and_alias(dev):
    """Without autograd: the same loss, logits and iut, no gradient buffer; compress_pred_loss is the
    same function; each optional output can be asked for alone."""
    from few_shot_seg_cwt_amd.seg_loss import compress_pred_loss, seg_head_loss_nway
    case = R.CASES[1]
    W, f, tgt = R.inputs(case, 8.0)
    loss, logits, _, iut = _run(dev, W, f, tgt, case[2], "wt_dc")
    Wd, fd, td = W.float().to(dev), f.float().to(dev), tgt.to(dev)
    l2, lg2, iut2 = compress_pred_loss(Wd, fd, td, case[2], "wt_dc", return_logits=True, return_iut=True)
    assert torch.equal(l2, loss) and torch.equal(lg2, logits) and torch.equal(iut2, iut)
    assert torch.equal(seg_head_loss_nway(Wd, fd, td, case[2], "dc"), loss)
    l3, iut3 = seg_head_loss_nway(Wd, fd, td, case[2], "wt_dc", return_iut=True)
    assert torch.equal(l3, loss) and torch.equal(iut3, iut)


def test_backward_scales_the_kept_gradient(dev):
    from few_shot_seg_cwt_amd.seg_loss import seg_head_loss_nway
    case = R.CASES[0]
    W, f, tgt = R.inputs(case, 8.0)
    _, _, g1, _ = _run(dev, W, f, tgt, case[2], "wt_dc")
    fd = f.float().to(dev).requires_grad_(True)
    (0.5 * seg_head_loss_nway(W.float().to(dev), fd, tgt.to(dev), case[2], "wt_dc")).backward()
    assert torch.equal(fd.grad, 0.5 * g1)


@pytest.mark.parametrize("lt", R.LOSS_TYPES)
def test_all_ignored_label(dev, lt):
    """Every pixel 255.  Dice: t = 0 in both channels, I = 0 -> loss exactly 2.0 and no gradient.
    CE: 0 / 0 -> a NaN loss and a zero gradient, as torch returns them."""
    case = R.CASES[0]
    W, f, tgt = R.inputs(case, 8.0)
    tgt = torch.full_like(tgt, 255)
    loss, _, d_f, iut = _run(dev, W, f, tgt, case[2], lt)
    if lt == "wt_dc":
        assert float(loss) == 2.0
    else:
        assert math.isnan(float(loss))
    assert float(d_f.abs().max()) == 0.0
    assert float(iut.abs().max()) == 0.0


@pytest.mark.parametrize("lt", ["wt_dc", "wt_ce"])
def test_no_foreground(dev, lt):
    """No pixel labelled 1: a finite loss within the bars; under wt_ce the weight multiplies nothing."""
    case = R.CASES[0]
    W, f, tgt = R.inputs(case, 8.0)
    tgt = tgt.clone()
    tgt[tgt == 1] = 0
    loss, _, d_f, _ = _run(dev, W, f, tgt, case[2], lt)
    fo = f.clone().requires_grad_(True)
    lo, _ = R.head_loss(W, fo, tgt, case[2], lt)
    lo.backward()
    print(f"{lt}, no foreground: loss {float(loss):.7f} ref {float(lo.detach()):.7f}, d_f rel {rel(d_f, fo.grad):.1e}")
    assert math.isfinite(float(loss)) and abs(float(loss) - float(lo.detach())) < LOSS_TOL
    assert rel(d_f, fo.grad) < GRAD_TOL
    if lt == "wt_ce":
        l_ce, _, g_ce, _ = _run(dev, W, f, tgt, case[2], "ce")
        assert torch.equal(l_ce, loss) and torch.equal(g_ce, d_f)


@pytest.mark.parametrize("lt", R.LOSS_TYPES)
@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[3]])
def test_saturated(dev, case, lt):
    """scale = 200: p rounds to 0 or 1 almost everywhere; the loss and every d_f element stay finite."""
    W, f, tgt = R.inputs(case, 1.0)
    loss, _, d_f, _ = _run(dev, 200.0 * W, f, tgt, case[2], lt)
    assert math.isfinite(float(loss))
    assert bool(torch.isfinite(d_f).all())


@pytest.mark.parametrize("lt", R.LOSS_TYPES)
def test_deterministic(dev, lt):
    case = R.CASES[1]
    W, f, tgt = R.inputs(case, 8.0)
    l1, lg1, g1, i1 = _run(dev, W, f, tgt, case[2], lt)
    l2, lg2, g2, i2 = _run(dev, W, f, tgt, case[2], lt)
    assert torch.equal(l1, l2) and torch.equal(g1, g2) and torch.equal(lg1, lg2) and torch.equal(i1, i2)


def test_argument_errors(dev):
    from few_shot_seg_cwt_amd._lib import CwtError
    from few_shot_seg_cwt_amd.seg_loss import seg_head_loss_nway
    tgt = torch.zeros((1, 33, 33), dtype=torch.int64, device=dev)
    z = lambda *s: torch.zeros(*s, device=dev)   # noqa: E731
    with pytest.raises(CwtError):
        seg_head_loss_nway(z(1, 64), z(1, 64, 5, 5), tgt, 0, "wt_dc")            # N = 1
    with pytest.raises(CwtError):
        seg_head_loss_nway(z(65, 64), z(1, 64, 5, 5), tgt, 0, "wt_dc")           # N = 65
    with pytest.raises(CwtError):
        seg_head_loss_nway(z(16, 64), z(1, 64, 5, 5), tgt, 16, "wt_dc")          # idx_cls = N
    with pytest.raises(CwtError):
        seg_head_loss_nway(z(16, 48), z(1, 48, 5, 5), tgt, 3, "wt_dc")           # C = 48
    with pytest.raises(CwtError):
        seg_head_loss_nway(z(16, 64), z(9, 64, 5, 5), tgt.expand(9, 33, 33).contiguous(), 3, "wt_dc")   # B = 9
