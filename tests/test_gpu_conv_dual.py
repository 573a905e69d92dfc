"""The two-source 1x1 conv of the x6 extractor (cwt_debug_conv_x6_dual: a bottleneck block's conv3 + BN
and downsample conv + BN folded into ONE GEMM over the concatenated K, conv_body.h PF bit 128) against
float64 relu(conv1x1(t) * s3 + b3 + conv1x1_stride(x) * sd + bd), at the bar of every x6 plan
(tests/test_gpu_conv_s.py: 1e-5 of max |y|).

Shapes where it can go wrong, not the workload's: M = 2 * 9 * 9 = 162 rows (no multiple of any tile
height, two 128-row tiles or three 64-row ones), the second source 17 x 17 read at stride 2 and 9 x 9
at stride 1, and K-tile counts (K1 / 32, K2 / 32) = (1, 2), (2, 1), (1, 1), (3, 5): the source switch
inside the LDS ring's prologue, on the last tile, with a single tile per source, and deep in the loop."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from few_shot_seg_cwt_amd import synthetic as syn  # noqa: E402

TOL_X6 = 1e-5   # tests/test_gpu_conv_s.py's bar of the x6 conv
N, HO = 2, 9
KS = [(32, 64), (64, 32), (32, 32), (96, 160)]
# bm = 1000 * variant + rows names the loop; every instantiated two-source form (conv_forms.h) and the
# library's own plan (0, 0)
FORMS = [(0, 0), (4128, 128), (5128, 128), (5128, 64), (5064, 128)]


def _lib():
    from few_shot_seg_cwt_amd import _lib as L
    return L


def run_dual(t, x, stride2, w3, s3, b3, wd, sd, bd, relu=True, bm=0, bn=0, nsplit=0):
    """t [N][K1][Ho][Ho], x [N][K2][Hi2][Hi2] (NCHW, CPU) -> y [N][Co][Ho][Ho] (CPU)"""
    L = _lib()
    dev = torch.device("cuda", 0)
    n, K1, Ho, _ = t.shape
    _, K2, Hi2, _ = x.shape
    Co = w3.shape[0]
    td = t.permute(0, 2, 3, 1).contiguous().to(dev)
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    dv = [v.contiguous().to(dev) for v in (w3, s3, b3, wd, sd, bd)]
    y = torch.full((n, Ho, Ho, Co), float("nan"), device=dev)
    rc = L.lib().cwt_debug_conv_x6_dual(L.ctx(0), L.ptr(td), n, Ho, Ho, K1, L.ptr(xd), Hi2, Hi2, K2, stride2,
                                        *[L.ptr(v) for v in dv], Co, int(relu), L.ptr(y), bm, bn, nsplit,
                                        L.stream_ptr())
    L.check(rc, "cwt_debug_conv_x6_dual")
    torch.cuda.synchronize()
    return y.cpu().permute(0, 3, 1, 2)


def ref_dual(t, x, stride2, w3, s3, b3, wd, sd, bd, relu=True):
    c = lambda v: v.double()[None, :, None, None]  # noqa: E731
    y = F.conv2d(t.double(), w3.double()[:, :, None, None]) * c(s3) + c(b3)
    y = y + F.conv2d(x.double(), wd.double()[:, :, None, None], None, stride2) * c(sd) + c(bd)
    return F.relu(y) if relu else y


_OPERANDS = {}


def operands(K1, K2, Co, stride2):
    """One draw per shape, shared by the forms' cases (with its float64 reference)"""
    key = (K1, K2, Co, stride2)
    if key not in _OPERANDS:
        tag = "_".join(map(str, key))
        Hi2 = (HO - 1) * stride2 + 1
        ops = (torch.from_numpy(syn.normal(3, "t" + tag, (N, K1, HO, HO), 1.0)),
               torch.from_numpy(syn.normal(3, "x" + tag, (N, K2, Hi2, Hi2), 1.0)), stride2,
               torch.from_numpy(syn.normal(3, "w3" + tag, (Co, K1), (2.0 / K1) ** 0.5)),
               torch.from_numpy(syn.uniform(3, "s3" + tag, (Co,), 0.5, 1.5)),
               torch.from_numpy(syn.normal(3, "b3" + tag, (Co,), 0.1)),
               torch.from_numpy(syn.normal(3, "wd" + tag, (Co, K2), (2.0 / K2) ** 0.5)),
               torch.from_numpy(syn.uniform(3, "sd" + tag, (Co,), 0.5, 1.5)),
               torch.from_numpy(syn.normal(3, "bd" + tag, (Co,), 0.1)))
        _OPERANDS[key] = (ops, ref_dual(*ops))
    return _OPERANDS[key]


FORM_CASES = [(s, ks, Co, f) for s in (2, 1) for ks in KS for Co in (64, 256) for f in FORMS if not (f[1] and Co % f[1])]


@pytest.mark.parametrize("stride2,ks,Co,form", FORM_CASES,
                         ids=[f"s{s}-{k[0]}+{k[1]}-Co{c}-{f[0]}x{f[1]}" for s, k, c, f in FORM_CASES])
def test_conv_dual_forms(stride2, ks, Co, form):
    bm, bn = form
    ops, ref = operands(ks[0], ks[1], Co, stride2)
    y = run_dual(*ops, bm=bm, bn=bn, nsplit=1 if bm else 0)
    err = float((y.double() - ref).abs().max() / ref.abs().max())
    assert err < TOL_X6, err


@pytest.mark.parametrize("ks,nsplit", [((32, 64), 3), ((64, 32), 2), ((96, 160), 2), ((96, 160), 4)],
                         ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("form", FORMS[1:], ids=lambda p: f"{p[0]}x{p[1]}")
def test_conv_dual_splitk(ks, nsplit, form):
    """Split-K over the concatenated K: a split may begin in either source (K-tile ranges 1|1|1, 2|1,
    4|4 with the switch at 3, 2|2|2|2 with it inside the second split)."""
    ops, ref = operands(ks[0], ks[1], 256, 2)
    y = run_dual(*ops, bm=form[0], bn=form[1], nsplit=nsplit)
    err = float((y.double() - ref).abs().max() / ref.abs().max())
    assert err < TOL_X6, err


def test_conv_dual_zero_last_bn():
    """s3 = 0 (a zero-initialised last BN of the residual branch): the first source's rows fold to
    zeros and the output is the downsample branch plus b3."""
    (t, x, s2, w3, s3, b3, wd, sd, bd), _ = operands(96, 160, 256, 2)
    s3 = torch.zeros_like(s3)
    y = run_dual(t, x, s2, w3, s3, b3, wd, sd, bd)
    ref = ref_dual(t, x, s2, w3, s3, b3, wd, sd, bd)
    err = float((y.double() - ref).abs().max() / ref.abs().max())
    assert err < TOL_X6, err


def test_conv_dual_wide_range_operands():
    """Operands spanning 2^-30 .. 2^30 in both sources (every split level populated), as
    test_conv_x6_wide_range_operands: element by element against float64, relative to sum |a||w| over
    both sources.  Per product: the dropped split terms (< 2^-23), the fold's one rounding of s * w
    (2^-24); plus the worst-case fp32 accumulation of K terms (K * 2^-24) and one rounding of the
    shift add."""
    g = torch.Generator().manual_seed(7)
    K1, K2, Co = 64, 96, 64

    def wide(shape):
        mant = torch.rand(shape, generator=g) + 0.5
        expo = torch.randint(-30, 31, shape, generator=g).float()
        return (mant * torch.pow(2.0, expo) * torch.sign(torch.randn(shape, generator=g))).float()

    t, x = wide((N, K1, HO, HO)), wide((N, K2, 17, 17))
    w3, wd = torch.randn((Co, K1), generator=g) * 0.05, torch.randn((Co, K2), generator=g) * 0.05
    s3, sd = torch.rand(Co, generator=g) + 0.5, torch.rand(Co, generator=g) + 0.5
    b3, bd = torch.randn(Co, generator=g) * 0.1, torch.randn(Co, generator=g) * 0.1
    y = run_dual(t, x, 2, w3, s3, b3, wd, sd, bd, relu=False)
    ref = ref_dual(t, x, 2, w3, s3, b3, wd, sd, bd, relu=False)
    c = lambda v: v.double().abs()[None, :, None, None]  # noqa: E731
    absref = (F.conv2d(t.double().abs(), w3.double().abs()[:, :, None, None]) * c(s3) +
              F.conv2d(x.double().abs(), wd.double().abs()[:, :, None, None], None, 2) * c(sd) + c(b3) + c(bd))
    K = K1 + K2
    bound = (2.0 * 2.0 ** -24 + 2.0 ** -24 + K * 2.0 ** -24 + 2.0 * 2.0 ** -24) * absref
    ratio = float(((y.double() - ref).abs() / absref).max())
    print("dual x6 max err / sum|a||w|:", ratio)
    assert bool(((y.double() - ref).abs() <= bound).all()), ratio
