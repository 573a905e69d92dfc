"""The match head's backward past one workgroup pass, against tests/match_ref.py (float64, the tie rule
written out).  Every other backward test stops at 12 x 12 = 144 positions per side, where the second
trip of every `for (j = t; j < NB; j += 256)` loop of csrc/match_bwd.hip never runs and a weight-gradient
workgroup (csrc/cp4d.hip) sees two tiles at most.

Working shape h x w = 15 x 19: NA = NB = 285 = 256 + 29 (a second, partial trip of every 256-stride
loop) = 17 * 16 + 13 (ragged against the 16-row blocks) = 4 * 64 + 29 (against the 64-column blocks);
ld32(285) = 288 (three pad columns in the readout); both sides ragged against the 4 x 4 and the 2 x 8
tiles.  The direct MutualMatching / readout cases use NB = 300 so that rows and columns differ.

Bars, all the project's own: 2e-5 forward (tests/test_gpu_match.py), 1e-6 MutualMatching's forward
(test_mutual_matching), 1e-4 every gradient (tests/test_gpu_match_bwd.TOL), each measured per tensor as
max|HIP - ref| / max|ref| and printed.

Weight gradient, every form through cwt_debug_cp4d_wgrad: B is chosen so that the kernel's own tile count
(4 x 4 by 4 x 4 tiles for wgrad_mfma and nc_wgrad, 2 x 8 by 2 x 8 for wgrad_scalar) is at least twice the
plan's G, read back from cwt_debug_cp4d_plan and asserted before the launch: every workgroup strides over
two tiles or more with its sums in the accumulators.  (wgrad_scalar needs B = 2 at 10 -> 10 and B = 8 at the
thin widths for that: 1,152 >= 2 * 512 and 4,608 >= 2 * 2,048.)  x and gm are uniform in [0, 1) there, so
nothing cancels and a dropped or doubled tile moves every element by about 1 / tiles (8e-4 at 1,200 tiles);
the outputs are pre-filled with a random r0 the entry accumulates onto.  One signed case per width and form
at B = 1 covers the filter-flip and index logic.
"""
import ctypes as C
import functools

import pytest
import torch

import match_ref as R
from few_shot_seg_cwt_amd import _lib

pytestmark = pytest.mark.gpu

H, W = 15, 19
NA, NBX = H * W, 300
WG_CAPS = dict(wide=512, thin=2048, nc=256)   # csrc/cp4d_plan.h: WG_G_WIDE, WG_G_THIN, WG_G_NC


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def cdiv(a, b):
    return (a + b - 1) // b


def cp4d_plan(d, shape, cin, cout):
    """cwt_debug_cp4d_plan under the environment as it is -> form name, grid, G, n"""
    out = (C.c_int * 16)()
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    _lib.check(_lib.lib().cwt_debug_cp4d_plan(d, *shape, cin, cout, 0, cu, 1, out), "cwt_debug_cp4d_plan")
    buf = C.create_string_buffer(256)
    _lib.check(_lib.lib().cwt_debug_cp4d_form(out[1], buf, len(buf)), "cwt_debug_cp4d_form")
    return dict(form=buf.value.decode().split("\t")[0], gx=out[6], gy=out[7], gz=out[8], G=out[14], n=out[15])


def match_bwd_plan(B, L, h, w, sym):
    """cwt_debug_match_plan of the backward -> the plan line's fields, and tensor -> (offset, floats) in `saved`"""
    buf = C.create_string_buffer(1 << 14)
    _lib.check(_lib.lib().cwt_debug_match_plan(1, B, L, h, w, int(sym), 0, 1, 1, 1, 1, buf, len(buf)),
               "cwt_debug_match_plan")
    lines = [ln.split("\t") for ln in buf.value.decode().splitlines()]
    kept = {f[1]: (int(f[3]), int(f[4])) for f in lines if f[0] == "buf" and f[2] == "saved"}
    return dict(kv.split("=") for kv in lines[0][2:]), kept


def device_sides(corr2d, kept, B, h, w, sym):
    """[branch][layer] -> the device's own ReLU output > 0, [B, C, h, w, h, w], from the activations its
    training forward kept for the backward (channels-last [B][NA][NB][C] at the plan's offsets)"""
    saved = corr2d.grad_fn.saved_tensors[3]
    sides = []
    for br in range(2 if sym else 1):
        row = []
        for l in range(3):
            off, n = kept[f"o{br}{l}"]
            o = saved[off:off + n].reshape(B, h * w, h * w, -1).permute(0, 3, 1, 2)
            row.append((o > 0).cpu().reshape(B, -1, h, w, h, w))
        sides.append(row)
    return sides


# ---- the chain ----
def _net(dev, L, sym, temp, seed):
    from few_shot_seg_cwt_amd.match import MatchNet, init_match_params
    net = MatchNet(temp=temp, in_channel=L, sym_mode=sym, device=dev)
    init_match_params(net, seed)
    with torch.no_grad():   # keep the one-channel last layer's ReLU open somewhere (a live gradient)
        net.NeighConsensus.conv[4].conv1.bias.add_(0.2)
    return net


@pytest.mark.parametrize("B,L,sym", [(1, 1, True), (2, 2, True), (1, 9, False)])
def test_corr_forward_backward_285(dev, monkeypatch, B, L, sym):
    """match.py:142-163 at 285 positions per side: corr2d, weighted v, d_corr, d_v and the twelve
    NeighConsensus gradients of <G1, corr2d> + <G2, weighted_v>; inputs as
    test_gpu_match_bwd.test_corr_forward_backward builds them.

    The reference is match_ref.corr_forward_sided: float64 autograd of the chain, in which the ReLU units
    whose float64 pre-activation lies within the forward bar of 0 (a few of 1e4 of them) take the side the
    device's own forward took, read from the activations it kept; every other unit must agree with float64
    (asserted).  Without that, (B, L, sym) = (2, 2, True) measures d_corr 3.4e-3, layer 0 / 2 weights 4e-4 /
    8e-4 with every kernel form alike: one unit of branch 1's second layer sits at +1.9e-8 in float64 and
    at or below 0 in fp32, and that one flip in float64 reproduces those figures exactly.

    Measured on an MI355X: forward 5.5e-7 .. 1.2e-6, every gradient 9.5e-8 .. 2.5e-6 in the three cases; 275 /
    458 / 111 of 3.4 M / 6.8 M / 1.7 M units took the device's side, none outside the margin disagreed."""
    for k in ("CWT_CP4D_ROLL", "CWT_DGRAD_SCALAR", "CWT_WGRAD_SCALAR", "CWT_MM_FUSE", "CWT_MATCH_BRANCH_STREAMS"):
        monkeypatch.delenv(k, raising=False)
    h, w, temp = H, W, 20.0
    shape = (B, h, w, h, w)
    # the plans this case is there for, before it is relied on
    p, kept = match_bwd_plan(B, L, h, w, sym)
    assert (p["branches"], p["d_corr"], p["d_v"], p["readout"], p["clast"]) == \
        (str(2 if sym else 1), "1", "1", "1", str(int(L > 1))), p
    assert cp4d_plan(1, shape, 10, 10)["form"] == "roll" and cp4d_plan(1, shape, 1, 10)["form"] == "roll"
    wide = cp4d_plan(2, shape, 10, 10)
    tiles44 = B * cdiv(h, 4) ** 2 * cdiv(w, 4) ** 2
    assert (wide["form"], wide["G"]) == ("wgrad_mfma", WG_CAPS["wide"]), wide   # at its cap
    first = cp4d_plan(2, shape, L, 10)
    if L == 9:    # the chunked first layer, its G at the cap and every workgroup striding
        assert (first["form"], first["G"], first["gy"]) == ("nc_wgrad", WG_CAPS["nc"], 2) and tiles44 > first["G"], first
    else:
        assert first["form"] == "wgrad_mfma", first
    if B == 2:    # more 4 x 4 tiles than workgroups: the 10 -> 10 weight gradient strides
        assert tiles44 > wide["G"]
    net = _net(dev, L, sym, temp, seed=11 + L + h)
    c0 = R.rand((B, L, h, w, h, w), 5 * h + w, -0.2, 1.0)
    v0 = R.rand((B, 64, h, w), 13)
    G1 = R.rand((B, h * w, h * w), 17, -1, 1)
    G2 = R.rand((B, 64, h, w), 19, -1, 1)
    corr = c0.float().to(dev).requires_grad_(True)
    v = v0.float().to(dev).requires_grad_(True)
    G1d, G2d = G1.float().to(dev), G2.float().to(dev)
    corr2d, wv = net.corr_forward(corr, v, ret_attn=True)
    sides = device_sides(corr2d, kept, B, h, w, sym)     # before the backward frees them
    ((corr2d * G1d).sum() + (wv * G2d).sum()).backward()
    sd = {k: t.detach().cpu().double() for k, t in net.state_dict().items()}
    info = []
    ref = R.chain_grads(dict(corr=c0, v=v0, G1=G1, G2=G2, sd=sd, temp=temp, sym=sym),
                        functools.partial(R.corr_forward_sided, sides=sides, info=info))
    units = sum(s_.numel() for row in sides for s_ in row)
    near, bad = sum(n for n, _ in info), sum(b for _, b in info)
    print(f"ReLU units {units}: {near} within the forward bar of 0 take the device's side, {bad} others disagree")
    assert bad == 0 and near < 1e-3 * units, info
    params = dict(net.named_parameters())
    assert float(ref["d_corr"].abs().max()) > 0 and float(ref["4.conv2.bias"].abs().max()) > 0   # not a dead stack
    fwd = dict(corr2d=R.rel(corr2d, ref["corr2d"]), wv=R.rel(wv, ref["wv"]))
    errs = dict(d_corr=R.rel(corr.grad, ref["d_corr"]), d_v=R.rel(v.grad, ref["d_v"]))
    for n in R.PARAM_NAMES:
        errs[n.replace("NeighConsensus.conv.", "")] = R.rel(params[n].grad, ref[n.replace("NeighConsensus.conv.", "")])
    print(f"corr_forward backward B={B} L={L} {h}x{w} sym={sym}: "
          + ", ".join(f"{k} {e:.1e}" for k, e in {**fwd, **errs}.items()))
    assert max(fwd.values()) < R.TOL_FWD, fwd
    assert max(errs.values()) < R.TOL_GRAD, errs
    if (B, L) == (1, 1):   # fixed-order reductions: a second backward gives the same bits
        g1 = [corr.grad.clone(), v.grad.clone()] + [p_.grad.clone() for p_ in net.parameters()]
        net.zero_grad()
        corr.grad, v.grad = None, None
        corr2d, wv = net.corr_forward(corr, v, ret_attn=True)
        ((corr2d * G1d).sum() + (wv * G2d).sum()).backward()
        for a, b in zip(g1, [corr.grad, v.grad] + [p_.grad for p_ in net.parameters()]):
            assert torch.equal(a, b)


# ---- MutualMatching and the readout alone ----
_mm = {}


def mm_case(Cc):
    """x, dy [2, C, 285, 300] and the float64 forward / first-index backward, once per C"""
    if Cc not in _mm:
        x = R.rand((2, Cc, NA, NBX), 100 + Cc, -1, 1).float().double()
        dy = R.rand((2, Cc, NA, NBX), 200 + Cc, -1, 1).float().double()
        xr = x.clone().requires_grad_(True)
        y = R.mutual_matching_first(xr.reshape(2, Cc, NA, 1, NBX, 1)).reshape(2, Cc, NA, NBX)
        (dx,) = torch.autograd.grad(y, xr, dy)
        _mm[Cc] = (x, dy, y.detach(), dx)
    return _mm[Cc]


def clast(t, dev):
    return t.permute(0, 2, 3, 1).contiguous().float().to(dev)   # [B][NA][NB][C]


@pytest.mark.parametrize("Cc", [1, 2, 3, 10])
def test_mutual_matching_285x300(dev, Cc):
    x, _, y_ref, _ = mm_case(Cc)
    xd = clast(x, dev)
    y = torch.full_like(xd, float("nan"))
    _lib.check(_lib.lib().cwt_mutual_matching(_lib.ctx(dev.index), _lib.ptr(xd), 2, NA, NBX, Cc, _lib.ptr(y),
                                              _lib.stream_ptr(dev)), "cwt_mutual_matching")
    e = R.rel(y.permute(0, 3, 1, 2), y_ref)
    print(f"MutualMatching 285x300 C={Cc}: {e:.2e}")
    assert e < R.TOL_MM


@pytest.mark.parametrize("Cc", [1, 2, 3, 10])
def test_mutual_matching_backward_285x300(dev, Cc):
    x, dy, _, dx_ref = mm_case(Cc)
    xd, dyd = clast(x, dev), clast(dy, dev)
    dx = torch.full_like(xd, float("nan"))
    _lib.check(_lib.lib().cwt_debug_mutual_matching_bwd(_lib.ctx(dev.index), _lib.ptr(xd), _lib.ptr(dyd), 2, NA, NBX, Cc,
                                                        _lib.ptr(dx), _lib.stream_ptr(dev)),
               "cwt_debug_mutual_matching_bwd")
    e = R.rel(dx.permute(0, 3, 1, 2), dx_ref)
    print(f"MutualMatching backward 285x300 C={Cc}: {e:.2e}")
    assert float(dx_ref.abs().max()) > 0 and e < R.TOL_GRAD


def test_readout_and_backward_285x300(dev):
    """cwt_match_readout / cwt_match_readout_backward at B = 2, NA = 285, NB = 300 (ld32 = 320), Cv = 48,
    temp = 20; d_corr2d is added into a random r0."""
    B, Cv, temp = 2, 48, 20.0
    c = R.rand((B, NA, NBX), 301, -0.2, 1.0).float().double()
    v = R.rand((B, NBX, Cv), 302, -1, 1).float().double()
    d = R.rand((B, NA, Cv), 303, -1, 1).float().double()
    r0 = R.rand((B, NA, NBX), 304, -1, 1).float()
    _, wv_ref, dc_ref, dv_ref = R.readout_fwd_bwd(c, v, temp, d)
    cd, vd, dd = c.float().to(dev), v.float().to(dev), d.float().to(dev)
    wv = torch.full((B, NA, Cv), float("nan"), device=dev)
    st = _lib.stream_ptr(dev)
    _lib.check(_lib.lib().cwt_match_readout(_lib.ctx(dev.index), _lib.ptr(cd), B, NA, NBX, temp, _lib.ptr(vd), Cv,
                                            _lib.ptr(wv), st), "cwt_match_readout")
    dc = r0.to(dev)
    dv = torch.full((B, NBX, Cv), float("nan"), device=dev)
    _lib.check(_lib.lib().cwt_match_readout_backward(_lib.ctx(dev.index), _lib.ptr(cd), B, NA, NBX, temp, _lib.ptr(vd), Cv,
                                                     _lib.ptr(dd), None, _lib.ptr(dc), _lib.ptr(dv), st),
               "cwt_match_readout_backward")
    errs = dict(wv=R.rel(wv, wv_ref), d_corr2d=R.rel(dc.double().cpu() - r0.double(), dc_ref), d_v=R.rel(dv, dv_ref))
    print(f"readout 285x300 Cv={Cv}: " + ", ".join(f"{k} {e:.1e}" for k, e in errs.items()))
    assert errs["wv"] < R.TOL_FWD and max(errs["d_corr2d"], errs["d_v"]) < R.TOL_GRAD, errs


# ---- the weight gradient, every form ----
# (form, cin, cout, B of the non-negative strided case)
WGRAD = [("wgrad_mfma", 10, 10, 3), ("wgrad_mfma", 1, 10, 11), ("wgrad_mfma", 2, 10, 11), ("wgrad_mfma", 10, 1, 11),
         ("nc_wgrad", 3, 10, 2), ("nc_wgrad", 9, 10, 2), ("nc_wgrad", 32, 10, 2),
         ("wgrad_scalar", 10, 10, 2), ("wgrad_scalar", 1, 10, 8), ("wgrad_scalar", 2, 10, 8), ("wgrad_scalar", 10, 1, 8)]
_wg = {}


def wgrad_case(cin, cout, B, signed):
    """x, gm, the four pre-filled outputs and the float64 gradients; the B = 1 cases, which two forms share,
    are kept"""
    key = (cin, cout, B, signed)
    if key not in _wg:
        lo = -1.0 if signed else 0.0
        x = R.rand((B, NA, NA, cin), 1000 * cin + cout + B, lo, 1.0).float()
        gm = R.rand((B, NA, NA, cout), 2000 * cin + cout + B, lo, 1.0).float()
        r0 = [R.rand(s, 3000 + i + cin, -1, 1).float() for i, s in enumerate([(cout, cin, 3, 3)] * 2 + [(cout,)] * 2)]
        dWa, dWb, db = R.cp4d_wgrad_ref(x.double(), gm.double(), (B, H, W, H, W))
        if B > 1:
            return x, gm, r0, [dWa, dWb, db, db]
        _wg[key] = (x, gm, r0, [dWa, dWb, db, db])
    return _wg[key]


@pytest.mark.parametrize("signed", [False, True], ids=["strided", "signed"])
@pytest.mark.parametrize("form,cin,cout,B", WGRAD)
def test_weight_gradient_every_form(dev, monkeypatch, form, cin, cout, B, signed):
    """Measured on an MI355X, worst of dWa / dWb per case: non-negative (strided) 1.0e-6 .. 2.1e-6 for wgrad_mfma,
    7.6e-7 .. 9.3e-7 for nc_wgrad, 1.1e-6 .. 2.0e-6 for wgrad_scalar; signed 3.1e-7 .. 8.5e-7; the double-summed
    biases 1.4e-8 .. 4.8e-8.  A dropped or doubled tile would show as 2e-4 (4,608 tiles) to 1.3e-3 (800).  The
    bar stays the project's 1e-4."""
    monkeypatch.delenv("CWT_WGRAD_SCALAR", raising=False)
    if form == "wgrad_scalar":
        monkeypatch.setenv("CWT_WGRAD_SCALAR", "1")   # read per launch
    B = 1 if signed else B
    shape = (B, H, W, H, W)
    p = cp4d_plan(2, shape, cin, cout)
    t = (2, 8) if form == "wgrad_scalar" else (4, 4)      # the kernel's own tiling, not the plan's
    tiles = B * (cdiv(H, t[0]) * cdiv(W, t[1])) ** 2
    cap = WG_CAPS["nc" if form == "nc_wgrad" else "wide" if cin * cout >= 100 else "thin"]
    assert p["form"] == form and p["n"] == 18 * cin * cout + cout and p["gx"] == p["G"], p
    if not signed:   # every workgroup strides: two tiles each at the least, G at its cap
        assert p["G"] == cap and tiles >= 2 * p["G"], (p, tiles)
    x, gm, r0, ref = wgrad_case(cin, cout, B, signed)
    xd, gd = x.to(dev), gm.to(dev)
    out = [r.clone().to(dev) for r in r0]
    _lib.check(_lib.lib().cwt_debug_cp4d_wgrad(_lib.ctx(dev.index), _lib.ptr(xd), _lib.ptr(gd), *shape, cin, cout,
                                               *[_lib.ptr(o) for o in out], _lib.stream_ptr(dev)), "cwt_debug_cp4d_wgrad")
    torch.cuda.synchronize()
    errs = {k: R.rel(o.double().cpu() - r.double(), g) for k, o, r, g in zip(("dWa", "dWb", "db1", "db2"), out, r0, ref)}
    print(f"cp4d wgrad {cin}->{cout} {form} B={B} tiles={tiles} G={p['G']} {'signed' if signed else 'non-negative'}: "
          + ", ".join(f"{k} {e:.1e}" for k, e in errs.items()))
    assert min(float(g.abs().max()) for g in ref) > 0
    assert max(errs.values()) < R.TOL_GRAD, errs
