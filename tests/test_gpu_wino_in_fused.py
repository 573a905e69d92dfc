"""The Winograd input transform with the split-K combine fused in (wino.hip, cwt_debug_wino_in with
nsplit > 0): V must be bit-identical (torch.equal) to V from the split-K epilogue kernel
(conv_s_splitk_epilogue, cwt_debug_splitk_epilogue) followed by the plain transform -- the same
operations in the same order, so there is no tolerance.

H = W = 7: with output tiles of 2 and 4 and dilation 1, 2, 4 the edge tiles are ragged and half
empty.  C = 36 is no multiple of the epilogue kernel's 8-channel groups: its reference runs that
kernel over the same floats viewed as [M / 2][72] with scale and shift repeated twice (elementwise
kernel, M = 2 * 49 even), which are the same operations per element."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N, H = 2, 7
M = N * H * H


def _lib():
    from few_shot_seg_cwt_amd import _lib as L
    return L


def wino_in(x, nsplit, scale, shift, relu, C, d, m):
    L = _lib()
    ty = ((H + d - 1) // d + m - 1) // m
    T = N * d * d * ty * ty
    V = torch.full(((m + 2) ** 2, T, C), float("nan"), device=x.device)
    L.check(L.lib().cwt_debug_wino_in(L.ctx(0), L.ptr(x), nsplit, L.ptr(scale), L.ptr(shift), int(relu), N, H, H, C,
                                      d, m, L.ptr(V), L.stream_ptr()), "cwt_debug_wino_in")
    torch.cuda.synchronize()
    return V


def epilogue(part, nsplit, scale, shift, relu, C):
    L = _lib()
    rows, cols, sc, sh = M, C, scale, shift
    if C % 8:
        rows, cols, sc, sh = M // 2, 2 * C, scale.repeat(2).contiguous(), shift.repeat(2).contiguous()
    y = torch.full((M, C), float("nan"), device=part.device)
    L.check(L.lib().cwt_debug_splitk_epilogue(L.ctx(0), L.ptr(part), nsplit, rows, cols, L.ptr(sc), L.ptr(sh),
                                              int(relu), L.ptr(y), L.stream_ptr()), "cwt_debug_splitk_epilogue")
    return y


@pytest.mark.parametrize("m", [2, 4], ids=lambda v: f"F{v}")
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "lin"])
@pytest.mark.parametrize("C", [32, 36])
@pytest.mark.parametrize("d", [1, 2, 4], ids=lambda v: f"d{v}")
@pytest.mark.parametrize("nsplit", [2, 4], ids=lambda v: f"ns{v}")
def test_fused_transform_is_bit_identical(nsplit, d, C, relu, m):
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(100 * nsplit + C)
    part = torch.randn((nsplit, M, C), generator=g).to(dev)
    scale = (torch.rand(C, generator=g) + 0.5).to(dev)
    shift = (torch.randn(C, generator=g) * 0.3).to(dev)
    t1 = epilogue(part, nsplit, scale, shift, relu, C)
    ref = wino_in(t1, 0, scale, shift, relu, C, d, m)
    got = wino_in(part, nsplit, scale, shift, relu, C, d, m)
    assert not torch.isnan(ref).any() and not torch.isnan(got).any()
    assert relu == bool((t1 >= 0).all())  # the ReLU flag reached the epilogue
    assert torch.equal(got, ref), float((got - ref).abs().max())
