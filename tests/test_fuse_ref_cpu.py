"""What the fusion trainer's GPU tests rely on, asserted on the CPU: the float64 reference of
tests/fuse_ref.py is the reference's arithmetic (against the oracle's layer at stride 1 and against a
loop over the definition at stride 2), each plausible wrong reading of it lies further from it than
SEPARATION, the fixtures exercise both sides of every ReLU with almost no unit near zero, and the
package's surface (state_dict names, ctypes prototypes) is there."""
import pytest
import torch

import fuse_ref as R
from oracle import match_oracle as M


def sep(a, b):
    """how far the wrong variant a lies from b, as a fraction of max|b|"""
    return R.rel(a, b)


def test_strided_layer_at_stride_1_is_the_oracles():
    x = R.rand((2, 3, 4, 5, 6, 3), 1, -1, 1)
    g = torch.Generator().manual_seed(3)
    w1, w2 = R._uniform((5, 3, 3, 3), g, 0.3), R._uniform((5, 3, 3, 3), g, 0.3)
    b1, b2 = R._uniform((5,), g, 0.3), R._uniform((5,), g, 0.3)
    assert R.rel(R.cp4d_strided(x, w1, b1, w2, b2, 1), M.center_pivot_conv4d(x, w1, b1, w2, b2)) < 1e-14


@pytest.mark.parametrize("hb", [3, 4])
def test_strided_layer_at_stride_2_is_the_definition(hb):
    x = R.rand((1, 2, 3, 3, hb, hb), 2, -1, 1)
    g = torch.Generator().manual_seed(4)
    w1, w2 = R._uniform((4, 2, 3, 3), g, 0.3), R._uniform((4, 2, 3, 3), g, 0.3)
    b1, b2 = R._uniform((4,), g, 0.3), R._uniform((4,), g, 0.3)
    got = R.cp4d_strided(x, w1, b1, w2, b2, 2)
    assert got.shape[-2:] == ((hb + 1) // 2, (hb + 1) // 2)
    assert R.rel(got, R.cp4d_direct(x, w1, b1, w2, b2, 2)) < 1e-14


@pytest.mark.parametrize("shape", [(5, 7, 8, 8), (4, 5, 6, 6)])
def test_wrong_prune_and_padding_separate(shape):
    x, p, _ = R.stack_case(shape, 5)
    pre1 = R.cp4d_strided(x.unsqueeze(1), *p[:4], stride=2)
    odd = R.cp4d_strided(x.unsqueeze(1), *p[:4], stride=2, prune_from=1)
    assert sep(odd, pre1) > R.SEPARATION
    nopad = R.cp4d_strided(x.unsqueeze(1), *p[:4], stride=2, pad=0)
    assert nopad.shape == pre1.shape and sep(nopad, pre1) > R.SEPARATION


def test_swapped_mask_and_pd_columns_separate():
    c = R.head_case((4, 5, 5, 5), 32)
    wt = R.fusenet1(c["corr"], c["s_mask"], c["pd"], c["sd"])
    bad = R.fusenet1(c["corr"], c["s_mask"], c["pd"], c["sd"], swap_mask_pd=True)
    assert sep(bad, wt) > R.SEPARATION


def test_ignored_pixels_left_out_of_the_denominator_separate():
    q, q0, q1, lbl = R.loss_case(5, 33, "edge")
    assert sep(R.fuse_loss(q, q0, q1, lbl, count_ignored=False), R.fuse_loss(q, q0, q1, lbl)) > R.SEPARATION


def test_flipped_align_corners_separates():
    lbl = R.label_case(57, 0)
    for pool in (False, True):
        assert sep(R.support_mask(lbl, 4, False, pool), R.support_mask(lbl, 4, True, pool)) > R.SEPARATION


@pytest.mark.parametrize("shape", R.STACK_SHAPES + [R.BIG_SHAPE])
def test_fixtures_exercise_both_relu_sides_away_from_zero(shape):
    x, p, _ = R.stack_case(shape)
    pre1, pre2 = R.stack_pre(x, p)
    alive = float((pre2 > 0).double().mean())
    assert 0.2 <= alive <= 0.9, alive
    assert 0.05 <= float((pre1 > 0).double().mean()) <= 0.95
    for pre in (pre1, pre2):
        near = int((pre.abs() < R.TOL_FWD * pre.abs().max()).sum())
        assert near <= R.NEAR_CAP * pre.numel(), (near, pre.numel())


@pytest.mark.parametrize("shape", R.STACK_SHAPES)
@pytest.mark.parametrize("mid", [32, 256])
def test_attention_hidden_units_stay_away_from_zero(shape, mid):
    c = R.head_case(shape, mid)
    pre = []
    R.fusenet1(c["corr"], c["s_mask"], c["pd"], c["sd"], hidden_out=pre)
    pre = pre[0]
    near = int((pre.abs() < R.TOL_FWD * pre.abs().max()).sum())
    assert near <= R.NEAR_CAP * pre.numel(), (near, pre.numel())
    assert 0.05 <= float((pre > 0).double().mean()) <= 0.95


def test_sided_stack_without_sides_is_the_stack():
    x, p, _ = R.stack_case((4, 5, 5, 5))
    pre1, pre2 = R.stack_pre(x, p)
    info = []
    y = R.stack_sided(x, p, (pre1 > 0, pre2 > 0), info)
    assert torch.equal(y, R.stack(x, p))
    assert all(bad == 0 for _, bad, _ in info)


def test_loss_fixtures_hold_what_their_names_say():
    q, q0, q1, lbl = R.loss_case(3, 17, "ignored")
    assert bool((lbl == 255).all()) and float(R.fuse_loss(q, q0, q1, lbl)) == 0.0
    q, q0, q1, lbl = R.loss_case(5, 33, "agree")
    assert R.fuse_counts(q, q0, q1, lbl)[1] == 0
    q, q0, q1, lbl = R.loss_case(8, 57, "edge")
    assert int((lbl != 255).sum()) == 2 * 57 - 1 and int(lbl[0, -1, -1]) != 255
    q, q0, q1, lbl = R.loss_case(8, 57, "mixed")
    assert R.fuse_counts(q, q0, q1, lbl)[1] > 100 and int((lbl == 255).sum()) > 0


def test_fusenet1_state_dict_is_the_references():
    from few_shot_seg_cwt_amd.transformer import FuseNet1
    sd = FuseNet1(im_size=30, mid_dim=256, device="cpu").state_dict()
    want = {"conv4d.0.conv1.weight": (16, 1, 3, 3), "conv4d.0.conv1.bias": (16,),
            "conv4d.0.conv2.weight": (16, 1, 3, 3), "conv4d.0.conv2.bias": (16,),
            "conv4d.2.conv1.weight": (1, 16, 3, 3), "conv4d.2.conv1.bias": (1,),
            "conv4d.2.conv2.weight": (1, 16, 3, 3), "conv4d.2.conv2.bias": (1,),
            "att.0.weight": (256, 2704, 1, 1), "att.0.bias": (256,), "att.2.weight": (2, 256, 1, 1),
            "att.2.bias": (2,)}
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert list(sd) == list(want)   # the reference's order too


def test_fusenet1_draws_its_init_from_the_host_rng_like_the_reference():
    from few_shot_seg_cwt_amd.transformer import FuseNet1
    torch.manual_seed(5)
    a = FuseNet1(im_size=3, mid_dim=8, device="cpu").state_dict()
    torch.manual_seed(5)
    convs = [torch.nn.Conv2d(1, 16, 3, padding=1) for _ in range(2)] + [torch.nn.Conv2d(16, 1, 3, padding=1) for _ in range(2)]
    convs += [torch.nn.Conv2d(31, 8, 1), torch.nn.Conv2d(8, 2, 1)]
    for (k, v), ref in zip(list(a.items())[::2], convs):
        assert torch.equal(v, ref.weight), k


def test_new_symbols_have_prototypes():
    from few_shot_seg_cwt_amd import _lib
    for n in ("cwt_fuse_stack", "cwt_fuse_stack_saved_floats", "cwt_fuse_stack_backward", "cwt_fuse_support_mask",
              "cwt_fuse_mask_bias", "cwt_fuse_mask_bias_backward", "cwt_fuse_softmax2", "cwt_fuse_softmax2_backward",
              "cwt_fuse_blend", "cwt_fuse_blend_backward", "cwt_fuse_loss_head"):
        assert n in _lib.SIGNATURES, n


def test_big_shape_makes_the_backward_grid_stride():
    hA, wA, hB, wB = R.BIG_SHAPE
    assert hA * wA * ((hB + 1) // 2) * ((wB + 1) // 2) > 1024 * 16   # FUSE_MAXBLK workgroups x 16 positions


def test_argument_checks_come_before_any_device_call():
    """Every refusal of cwt_fuse_stack / cwt_fuse_stack_backward, reached without a context (the entries
    check their arguments before they look at it) and so without a device."""
    import ctypes as C
    from few_shot_seg_cwt_amd import _lib
    L = _lib.load_library()
    buf = (C.c_float * 4096)()
    ptr = C.cast(buf, C.c_void_p)

    def stack(B=1, sides=(4, 4, 4, 4), corr=ptr, w=ptr, X=ptr, ldx=8, col=0):
        return L.cwt_fuse_stack(None, corr, B, *sides, *([w] * 8), None, X, ldx, col, None)

    def refused(rc, word):
        assert rc == 1001 and word.encode() in L.cwt_last_error(), (rc, L.cwt_last_error())

    refused(stack(), "ctx")                       # nothing else wrong: only then the context is looked at
    refused(stack(B=0), "B must")
    refused(stack(B=65), "B must")
    refused(stack(sides=(1, 4, 4, 4)), "sides")
    refused(stack(sides=(4, 4, 4, 1)), "sides")
    refused(stack(sides=(4, 4, 600, 4)), "sides")
    refused(stack(corr=None), "NULL")
    refused(stack(X=None), "NULL")
    refused(stack(w=None), "parameter is NULL")
    refused(stack(ldx=3), "ldx")                  # 4 columns needed
    refused(stack(ldx=5, col=2), "ldx")
    refused(stack(col=-1), "ldx")
    bwd = lambda **k: L.cwt_fuse_stack_backward(None, ptr, 1, 4, 4, 4, 4, k.get("w2", ptr), ptr, k.get("y1", ptr), ptr,   # noqa: E731
                                                k.get("dX", ptr), k.get("ldx", 8), 0, 0, *([k.get("g", ptr)] * 8), None)
    refused(bwd(), "ctx")
    refused(bwd(y1=None), "y1_saved")
    refused(bwd(dX=None), "d_X")
    refused(bwd(g=None), "NULL")
    refused(bwd(ldx=2), "ldx")
    refused(L.cwt_fuse_support_mask(None, ptr, 1, 8, 4, 1, 0, ptr, None), "H, W")
    refused(L.cwt_fuse_mask_bias(None, ptr, 4, 2, ptr, 4, ptr, 8, ptr, None), "ldw")
    refused(L.cwt_fuse_loss_head(None, ptr, ptr, ptr, 1, 4, ptr, 17, ptr, None, ptr, ptr, None), "h, w")
    refused(L.cwt_fuse_loss_head(None, ptr, ptr, ptr, 4, 4, None, 17, ptr, None, ptr, ptr, None), "NULL")
    assert L.cwt_fuse_stack_saved_floats(1, 60, 60, 60, 60) == 3600 * 900 * 16
    assert L.cwt_fuse_stack_saved_floats(1, 1, 60, 60, 60) == 0
