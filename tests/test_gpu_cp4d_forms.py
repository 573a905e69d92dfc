"""The consensus layer's forms as the plan (csrc/cp4d_plan.h) names them, at small shapes.

Forward: cwt_debug_cp4d_layer variant 0 (the automatic choice) is the kernel cwt_debug_cp4d_plan names, so
its output equals, bit for bit, that of the variant which forces that kernel on the same input -- with the
default environment and with CWT_CP4D_ROLL=0 set before the call (the knobs are read per launch).

Input gradient: every form of cwt_debug_cp4d_dgrad -- rolling window, tile MFMA (variant 1: the form a
641^2 head runs, which no other test reaches), scalar, chunked -- against float64 autograd through the two
2-D convolutions of the layer (tests/test_gpu_cp4d_roll.py's ref_layer without bias and ReLU).  Bar:
max|dx - ref| / max|ref| < 2e-5, the project's forward bar (tests/test_gpu_match_nch.py derives it: an output
is an fp32 sum of at most 18 * 10 products, 2^-24 * 180 = 1.1e-5 at worst); the input gradient is the same
cross-shaped convolution with at most 18 * 10 products per output."""
import ctypes as C
import importlib.util
import os

import pytest
import torch

from few_shot_seg_cwt_amd import _lib

pytestmark = pytest.mark.gpu

TOL_FWD = 2e-5
_spec = importlib.util.spec_from_file_location(
    "cp4d_roll_cases", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_cp4d_roll.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)
FWD_CASES = R.test_roll_layer_small.pytestmark[0].args[1]
FORM_NAMES = ["scalar", "tile_mfma", "tile_c1", "persist_mfma", "persist_c1", "roll", "roll_c1", "nc_fwd", "nc_dgrad"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def planned_form(d, shape, cin, cout, variant):
    out = (C.c_int * 16)()
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    _lib.check(_lib.lib().cwt_debug_cp4d_plan(d, *shape, cin, cout, variant, cu, 1, out), "cwt_debug_cp4d_plan")
    return FORM_NAMES[out[1]]


@pytest.mark.parametrize("roll_env", [None, "0"])
@pytest.mark.parametrize("B,hA,wA,hB,wB,cin,cout", FWD_CASES)
def test_forward_automatic_choice_is_the_planned_kernel(dev, monkeypatch, roll_env, B, hA, wA, hB, wB, cin, cout):
    monkeypatch.delenv("CWT_CP4D_ROLL", raising=False)
    if roll_env is not None:
        monkeypatch.setenv("CWT_CP4D_ROLL", roll_env)
    form = planned_form(0, (B, hA, wA, hB, wB), cin, cout, 0)
    # these shapes fit the rolling window: it is the choice unless the knob forbids it
    assert form.startswith("roll") == (roll_env is None), form
    g = torch.Generator().manual_seed(hA * 100 + wB)
    x = (torch.rand(B, hA * wA, hB * wB, cin, generator=g) - 0.3).to(dev)
    p = [t.float().contiguous() for t in R.params(cin, cout, cin + cout, dev)]
    forced = 2 if form.startswith("roll") else 1
    assert planned_form(0, (B, hA, wA, hB, wB), cin, cout, forced) == form
    y0 = R.run(x, B, hA, wA, hB, wB, cin, cout, *p, 0)
    yf = R.run(x, B, hA, wA, hB, wB, cin, cout, *p, forced)
    assert float(y0.abs().max()) > 0 and torch.equal(y0, yf), (form, float((y0 - yf).abs().max()))


def lin_layer(x, B, hA, wA, hB, wB, Wa, Wb):
    """ref_layer without bias and ReLU"""
    Cc = x.shape[-1]
    NA, NB = hA * wA, hB * wB
    F = torch.nn.functional
    xa = x.view(B, hA, wA, NB, Cc).permute(0, 3, 4, 1, 2).reshape(B * NB, Cc, hA, wA)
    ya = F.conv2d(xa, Wa, None, padding=1).view(B, NB, -1, hA, wA).permute(0, 3, 4, 1, 2).reshape(B, NA, NB, -1)
    xb = x.view(B * NA, hB, wB, Cc).permute(0, 3, 1, 2)
    return ya + F.conv2d(xb, Wb, None, padding=1).permute(0, 2, 3, 1).reshape(B, NA, NB, -1)


_refs = {}


def dgrad_case(dev, shape, gin, gout):
    """g [B][NA][NB][gin], the filters [gin][gout][3][3] and the float64 gradient, made once per case"""
    key = (shape, gin, gout)
    if key not in _refs:
        B, hA, wA, hB, wB = shape
        gen = torch.Generator().manual_seed(1000 * gin + 10 * gout + hA)
        mk = lambda *sh: torch.rand(*sh, generator=gen, dtype=torch.float64) * 2 - 1  # noqa: E731
        g64 = mk(B, hA * wA, hB * wB, gin).to(dev)
        Wa, Wb = (mk(gin, gout, 3, 3) * (9 * gout) ** -0.5).to(dev), (mk(gin, gout, 3, 3) * (9 * gout) ** -0.5).to(dev)
        r0 = mk(B, hA * wA, hB * wB, gout).float().to(dev)   # what accum = 1 adds to
        x = torch.zeros(B, hA * wA, hB * wB, gout, dtype=torch.float64, device=dev, requires_grad=True)
        (ref,) = torch.autograd.grad(lin_layer(x, *shape, Wa, Wb), x, g64)
        _refs[key] = (g64.float().contiguous(), Wa.float().contiguous(), Wb.float().contiguous(), r0, ref.detach())
    return _refs[key]


@pytest.mark.parametrize("accum", [0, 1])
@pytest.mark.parametrize("form,gin,gout,variant", [("roll", 1, 10, 0), ("roll", 10, 10, 0), ("tile_mfma", 1, 10, 1),
                                                   ("tile_mfma", 10, 10, 1), ("scalar", 10, 1, 0), ("scalar", 10, 2, 0),
                                                   ("nc_dgrad", 10, 3, 0), ("nc_dgrad", 10, 9, 0)])
@pytest.mark.parametrize("shape", [(2, 9, 13, 11, 7), (1, 3, 2, 5, 3)])   # no multiple of a tile; smaller than any
def test_input_gradient_every_form(dev, monkeypatch, shape, form, gin, gout, variant, accum):
    for k in ("CWT_CP4D_ROLL", "CWT_DGRAD_SCALAR"):
        monkeypatch.delenv(k, raising=False)
    assert planned_form(1, shape, gin, gout, variant) == form
    g, Wa, Wb, r0, ref = dgrad_case(dev, shape, gin, gout)
    dx = r0.clone() if accum else torch.full_like(r0, float("nan"))
    _lib.check(_lib.lib().cwt_debug_cp4d_dgrad(_lib.ctx(dev.index), _lib.ptr(g), *shape, gin, gout, _lib.ptr(Wa),
                                               _lib.ptr(Wb), _lib.ptr(dx), accum, variant, _lib.stream_ptr(dev)),
               "cwt_debug_cp4d_dgrad")
    torch.cuda.synchronize()
    got = dx.double() - r0.double() if accum else dx.double()
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"cp4d dgrad {gin}->{gout} {form} shape={shape} accum={accum}: {err:.2e}")
    assert float(ref.abs().max()) > 0
    assert err < TOL_FWD, (form, err)
