"""The GEMM-shaped body of conv_igemm_x6 (conv_body.h PF bit 256: every launch with kh = kw = 1 and
pad = 0 -- 1x1 convs of any stride, the two-source forms, the Winograd products) against the general
body it replaces.  CWT_X6_GEMM_BODY is read at every launch, so each case runs twice in one process:
the two outputs must be equal bit for bit (torch.equal), and the knob-on output meets the bar of
every x6 plan against a float64 conv (tests/test_gpu_conv_s.py: 1e-5 of max |y|).

Shapes where this code can go wrong, not the workload's: fewer K-tiles than ring stages, an odd tile
count on the two-stage ring, the partial-plane epilogue of a split-K plan; M = 25 (one tile, whole
waves past M) and M = 162 (the second 128-row tile holds 34 rows: one wave full, one with 2 rows, two
with none); stride 2 (the prologue keeps its divisions); both orders of the two sources' K-tile
counts; Winograd products with 9 valid rows per batch."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from few_shot_seg_cwt_amd import synthetic as syn  # noqa: E402
from test_gpu_conv_dual import ref_dual, run_dual  # noqa: E402
from test_gpu_conv_s import TOL_X6, ref_conv, run_conv_f32d  # noqa: E402

KNOB = "CWT_X6_GEMM_BODY"
# bm = 1000 * var + rows: every tile with a GEMM-shaped body (conv_forms.h CWT_CONV_GEMM_ROWS_X6);
# Co = bn, so the grid holds the tile itself and no case is skipped
FORMS = [(5128, 128), (3128, 128), (5064, 128), (5128, 64), (3064, 64), (4128, 128), (64, 64)]
form_id = lambda f: f"{f[0]}x{f[1]}"  # noqa: E731


class knob:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.saved = os.environ.get(KNOB)
        os.environ[KNOB] = self.value

    def __exit__(self, *exc):
        if self.saved is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = self.saved
        return False


def both(run):
    """run() with the GEMM-shaped body and with the general one"""
    with knob("1"):
        y1 = run()
    with knob("0"):
        y0 = run()
    return y1, y0


def check(y1, y0, ref):
    assert torch.equal(y1, y0), float((y1.double() - y0.double()).abs().max())
    err = float((y1.double() - ref).abs().max() / ref.abs().max())
    assert err < TOL_X6, err


_CASES = {}


def conv_case(N, Ci, Co, Hi, k, stride, dil, has_res):
    """One draw per shape and its float64 reference, shared by the forms' cases"""
    key = (N, Ci, Co, Hi, k, stride, dil, has_res)
    if key not in _CASES:
        tag = "g" + "_".join(map(str, key))
        pad = dil if k == 3 else 0
        Ho = (Hi + 2 * pad - dil * (k - 1) - 1) // stride + 1
        x = torch.from_numpy(syn.normal(5, "x" + tag, (N, Ci, Hi, Hi), 1.0))
        w = torch.from_numpy(syn.normal(5, "w" + tag, (Co, Ci, k, k), (2.0 / (Ci * k * k)) ** 0.5))
        scale = torch.from_numpy(syn.uniform(5, "s" + tag, (Co,), 0.5, 1.5))
        shift = torch.from_numpy(syn.normal(5, "b" + tag, (Co,), 0.1))
        res = torch.from_numpy(syn.normal(5, "r" + tag, (N, Co, Ho, Ho), 1.0)) if has_res else None
        ops = (x, w, scale, shift, stride, pad, dil, res)
        _CASES[key] = (ops, ref_conv(*ops, relu=has_res))
    return _CASES[key]


def run_both(ops, relu, bm, bn, nsplit, entry="cwt_debug_conv_x6"):
    return both(lambda: run_conv_f32d(*ops, relu=relu, bm=bm, bn=bn, nsplit=nsplit, entry=entry))


@pytest.mark.parametrize("Ci,nsplit", [(32, 1), (96, 1), (128, 2)], ids=["Ci32", "Ci96", "Ci128s2"])
@pytest.mark.parametrize("form", FORMS, ids=form_id)
def test_ring_edges(form, Ci, nsplit):
    """One K-tile (fewer than any ring holds), three (odd on the two-stage ring), and four over a
    split-K of 2 (each workgroup's partial plane, then the reduction)."""
    ops, ref = conv_case(2, Ci, form[1], 9, 1, 1, 1, True)
    check(*run_both(ops, True, form[0], form[1], nsplit), ref)


@pytest.mark.parametrize("N,Hi", [(1, 5), (2, 9)], ids=["M25", "M162"])
@pytest.mark.parametrize("has_res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("form", FORMS, ids=form_id)
def test_row_edges(form, has_res, N, Hi):
    ops, ref = conv_case(N, 64, form[1], Hi, 1, 1, 1, has_res)
    check(*run_both(ops, has_res, form[0], form[1], 1), ref)


@pytest.mark.parametrize("has_res", [False, True], ids=["plain", "res_relu"])
@pytest.mark.parametrize("form", FORMS, ids=form_id)
def test_stride2_1x1(form, has_res):
    """Hi = 9 -> Ho = 5: row m's pixel is not m, the prologue keeps its divisions."""
    ops, ref = conv_case(2, 64, form[1], 9, 1, 2, 1, has_res)
    check(*run_both(ops, has_res, form[0], form[1], 1), ref)


def test_library_plan():
    """bm = bn = 0: the plan the library picks for the shape, whatever row that is"""
    ops, ref = conv_case(2, 96, 256, 9, 1, 1, 1, True)
    check(*run_both(ops, True, 0, 0, 0), ref)


DUAL_FORMS = [(4128, 128), (5128, 128), (5128, 64), (5064, 128)]


@pytest.mark.parametrize("stride2", [2, 1], ids=["s2", "s1"])
@pytest.mark.parametrize("K1,K2", [(32, 64), (64, 32)], ids=["32+64", "64+32"])
@pytest.mark.parametrize("form", DUAL_FORMS, ids=form_id)
def test_two_sources(form, K1, K2, stride2):
    """Ho = 5, M = 50; the source switch after the first K-tile (inside the ring's prologue) and
    before the last one; the second source read at stride 2 (divisions) and 1 (none)."""
    N, Ho, Co = 2, 5, form[1]
    key = ("dual", K1, K2, Co, stride2)
    if key not in _CASES:
        tag = "d" + "_".join(map(str, key[1:]))
        Hi2 = (Ho - 1) * stride2 + 1
        ops = (torch.from_numpy(syn.normal(5, "t" + tag, (N, K1, Ho, Ho), 1.0)),
               torch.from_numpy(syn.normal(5, "x" + tag, (N, K2, Hi2, Hi2), 1.0)), stride2,
               torch.from_numpy(syn.normal(5, "w3" + tag, (Co, K1), (2.0 / K1) ** 0.5)),
               torch.from_numpy(syn.uniform(5, "s3" + tag, (Co,), 0.5, 1.5)),
               torch.from_numpy(syn.normal(5, "b3" + tag, (Co,), 0.1)),
               torch.from_numpy(syn.normal(5, "wd" + tag, (Co, K2), (2.0 / K2) ** 0.5)),
               torch.from_numpy(syn.uniform(5, "sd" + tag, (Co,), 0.5, 1.5)),
               torch.from_numpy(syn.normal(5, "bd" + tag, (Co,), 0.1)))
        _CASES[key] = (ops, ref_dual(*ops))
    ops, ref = _CASES[key]
    check(*both(lambda: run_dual(*ops, bm=form[0], bn=form[1], nsplit=1)), ref)


@pytest.mark.parametrize("Hi,dil", [(5, 1), (6, 2)], ids=["H5d1", "H6d2"])
@pytest.mark.parametrize("form", [(5128, 128), (4128, 128), (3128, 128)], ids=form_id)
def test_winograd_products(form, Hi, dil):
    """F(2x2, 3x3): 3 x 3 = 9 tiles at H = 5, d = 1 and 4 sub-grids of 2 x 2 = 16 tiles at H = 6,
    d = 2 -- one M-tile of 9 or 16 valid rows in each of the 16 batched GEMMs, three of its four
    waves past M."""
    ops, ref = conv_case(1, 32, 128, Hi, 3, 1, dil, True)
    check(*run_both(ops, True, form[0], form[1], 2, entry="cwt_debug_conv_x6w"), ref)


def test_whole_extractor():
    """R50 at S = 33 on the x6 path: the features with the knob on and off are the same bits."""
    from few_shot_seg_cwt_amd import get_model
    dev = torch.device("cuda", 0)
    m = get_model(syn.cfg_defaults(layers=50, dropout=0.0))
    m.load_state_dict(syn.make_pspnet_state(50, 2021))
    x = torch.from_numpy(syn.make_episode(2021, 7, 33, 2)["spprt_imgs"][0]).to(dev)

    def run():
        f, _ = m.extract_features(x)
        torch.cuda.synchronize()
        return f.clone()

    f1, f0 = both(run)
    assert torch.isfinite(f1).all()
    assert torch.equal(f1, f0), float((f1.double() - f0.double()).abs().max())
