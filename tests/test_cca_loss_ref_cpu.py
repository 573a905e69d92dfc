"""What the GPU tests of the compressed N-way loss head (tests/test_gpu_cca_loss.py,
tests/test_gpu_cca_mix.py) rely on, proved on the CPU with tests/cca_loss_ref.py alone: the three
loss types are three different functions on the test draws, the N = 2 compressed loss is not the
2-way sigmoid head's, the 'ce' branch is F.cross_entropy on the probabilities, the p > 0.5 mask is
not pred2bmask's, fp32 torch meets the bars at every GPU case, every case has a live gradient, and
the draws are clear of the decision edges."""
import pytest
import torch
import torch.nn.functional as F

import cca_loss_ref as R
import seg_loss_ref as R2

LOSS_TOL, GRAD_TOL, FWD_TOL = 1e-5, 1e-4, 2e-5


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("scale", R.SCALES)
@pytest.mark.parametrize("case", R.CASES)
def test_loss_types_differ(case, scale):
    out = {lt: R.reference(case, scale, lt) for lt in R.LOSS_TYPES}
    for a, b in (("wt_ce", "wt_dc"), ("wt_ce", "ce"), ("wt_dc", "ce")):
        assert abs(float(out[a][0]) - float(out[b][0])) > 10 * LOSS_TOL, (a, b)
        assert rel(out[a][2], out[b][2]) > 10 * GRAD_TOL, (a, b)


def test_two_way_compressed_is_not_the_sigmoid_head():
    case = (1, 2, 1, 512, 6, 50)
    for scale in R.SCALES:
        W, f, tgt = R.inputs(case, scale)
        for lt in R.LOSS_TYPES:
            l2, _ = R2.head_loss(W, f, tgt, lt)
            assert abs(float(l2) - float(R.reference(case, scale, lt)[0])) > 10 * LOSS_TOL, (scale, lt)


def test_ce_branch_is_cross_entropy_on_the_probabilities():
    case = R.CASES[0]
    W, f, tgt = R.inputs(case, 8.0)
    q = R.compress_pred(R.upsample(R.head_logits(W, f), case[5]), case[2])
    ce = R.seg_loss_pb(q, tgt, "ce")
    assert float((ce - F.cross_entropy(q, tgt, ignore_index=255)).abs()) < 1e-12
    assert float((ce - F.nll_loss(torch.log(q), tgt, ignore_index=255)).abs()) > 1e-2   # not on their logs
    fg, bg = (tgt == 1).sum().double(), (tgt == 0).sum().double()
    wce = F.cross_entropy(q, tgt, weight=torch.stack([torch.ones(()).double(), bg / fg]), ignore_index=255)
    assert float((R.seg_loss_pb(q, tgt, "wt_ce") - wce).abs()) < 1e-12
    # 'dc' is 'wt_dc'; any other name is 'wt_ce' (model_util.py:16-24)
    assert float(R.seg_loss_pb(q, tgt, "dc")) == float(R.seg_loss_pb(q, tgt, "wt_dc"))
    assert float(R.seg_loss_pb(q, tgt, "focal")) == float(R.seg_loss_pb(q, tgt, "wt_ce"))


def test_half_mask_is_not_the_argmax_mask():
    differ = 0
    for case in R.CASES:
        for scale in R.SCALES:
            W, f, tgt = R.inputs(case, scale)
            hi = R.upsample(R.head_logits(W, f), case[5])
            differ += int(not torch.equal(R.iut_half(hi, tgt, case[2]), R.iut_argmax(hi, tgt, case[2])))
    assert differ >= 1


@pytest.mark.parametrize("lt", R.LOSS_TYPES)
@pytest.mark.parametrize("scale", R.SCALES)
@pytest.mark.parametrize("case", R.CASES)
def test_fp32_torch_meets_the_bars(case, scale, lt):
    W, f, tgt = R.inputs(case, scale)
    lo, lgo, dfo, _ = R.reference(case, scale, lt)
    f32 = f.float().requires_grad_(True)
    loss, lg = R.head_loss(W.float(), f32, tgt, case[2], lt)
    loss.backward()
    assert float(dfo.abs().max()) > 0
    assert abs(float(loss.detach()) - float(lo)) < LOSS_TOL
    assert rel(f32.grad, dfo) < GRAD_TOL
    assert rel(lg, lgo) < FWD_TOL


@pytest.mark.parametrize("case", R.CASES)
def test_loss_draws_are_clear_of_one_half(case):
    for scale in R.SCALES:
        W, f, tgt = R.inputs(case, scale)
        assert R.half_share(R.upsample(R.head_logits(W, f), case[5]), case[2]) == 0.0
        assert int((tgt == 0).sum()) != int((tgt == 1).sum()) and int((tgt == 1).sum()) > 0


@pytest.mark.parametrize("case", R.MIX_CASES)
def test_mix_draws_are_clear_of_ties(case):
    z0, z1, tgt = R.draw_mix(case)
    S, N = case[3], case[1]
    hi0, hi1 = R.upsample(z0.double(), S), R.upsample(z1.double(), S)
    for a in [0.0] + R.MIX_WTS:
        m = R.mix(hi0, hi1, a)
        near, ties = R.mix_gap_share(m)
        assert near == 0.0
        if N > 3:   # the pinned tie: classes 0 and N - 1 at hi-res (0, 0), the first index wins
            assert ties > 0 and float(m[0, 0, 0, 0]) == float(m[0, N - 1, 0, 0]) and int(m[0, :, 0, 0].argmax()) == 0
            assert int(R.mix_mask(hi0, hi1, a, 0)[0, 0, 0]) == 1 and int(R.mix_mask(hi0, hi1, a, N - 1)[0, 0, 0]) == 0
    # the mix at 0.5 is not either input's argmax everywhere
    assert not torch.equal(R.mix_mask(hi0, hi1, 0.5, 1), (hi0.argmax(1) == 1).long())
