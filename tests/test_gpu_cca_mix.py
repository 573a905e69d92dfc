"""cwt_seg_metrics_nway_mix (csrc/nway_pixel.hip; incremental.pred_mix_metrics): pred_q2 of
src/train_cca.py:347, 353 -- pred2bmask(softmax(z0) (1 - att_wt) + softmax(z1) att_wt) counted
against the target -- against the float64 mask of tests/cca_loss_ref.py.  The draws have no top-two
gap of the mix within 1e-4 in float64 (tests/test_cca_loss_ref_cpu.py), exact ties apart, so the
counts are demanded exactly; where N > 3 an exact tie of classes 0 and N - 1 at hi-res pixel (0, 0)
pins the first-index rule."""
import pytest
import torch

import cca_loss_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _want(case, att_wt, idx):
    z0, z1, tgt = R.draw_mix(case)
    S = case[3]
    return R.iut_of_mask(R.mix_mask(R.upsample(z0.double(), S), R.upsample(z1.double(), S), att_wt, idx), tgt)


@pytest.mark.parametrize("att_wt", R.MIX_WTS)
@pytest.mark.parametrize("case", R.MIX_CASES)
def test_mix_counts(dev, case, att_wt):
    from few_shot_seg_cwt_amd.incremental import pred_mix_metrics
    B, N, h, S = case
    z0, z1, tgt = R.draw_mix(case)
    for idx in sorted({0, 1, N - 1}):   # 0 and N - 1: the two sides of the pinned tie
        got = pred_mix_metrics(z0.to(dev), z1.to(dev), att_wt, tgt.to(dev), idx)
        want = _want(case, att_wt, idx)
        assert torch.equal(got.cpu().double(), want), (idx, got.cpu(), want)
        again = pred_mix_metrics(z0.to(dev), z1.to(dev), att_wt, tgt.to(dev), idx)
        assert torch.equal(got, again)
    if N > 3:   # the tie pixel is labelled 1: it is an intersection of class 1 for idx 0 alone
        assert float(_want(case, att_wt, 0)[0, 0, 1]) >= 1


@pytest.mark.parametrize("case", R.MIX_CASES)
def test_zero_weight_is_the_plain_metric(dev, case):
    from few_shot_seg_cwt_amd.incremental import pred2bmask_metrics, pred_mix_metrics
    B, N, h, S = case
    z0, z1, tgt = R.draw_mix(case)
    for idx in (0, N - 1):
        got = pred_mix_metrics(z0.to(dev), z1.to(dev), 0.0, tgt.to(dev), idx)
        plain, _ = pred2bmask_metrics(z0.to(dev), tgt.to(dev), idx, with_ce=False)
        assert torch.equal(got, plain)
        assert torch.equal(got.cpu().double(), _want(case, 0.0, idx))


def test_argument_errors(dev):
    from few_shot_seg_cwt_amd import _lib
    lib, ctx = _lib.lib(), _lib.ctx(0)
    z = torch.zeros((1, 3, 2, 2), device=dev)
    lbl = torch.zeros((1, 9, 9), dtype=torch.int64, device=dev)
    iut = torch.zeros((1, 3, 2), device=dev)
    call = lambda N, h, idx, a: lib.cwt_seg_metrics_nway_mix(   # noqa: E731
        ctx, _lib.ptr(z), _lib.ptr(z), a, _lib.ptr(lbl), 1, N, h, 2, 9, idx, _lib.ptr(iut), None)
    assert call(3, 2, 3, 0.2) == 1001
    assert call(1, 2, 0, 0.2) == 1001
    assert call(65, 2, 0, 0.2) == 1001
    assert call(3, 1, 0, 0.2) == 1001
    assert call(3, 2, 0, 1.5) == 1001
    assert call(3, 2, 1, 0.2) == 0
