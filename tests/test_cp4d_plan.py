"""The consensus layer's launch plan (csrc/cp4d_plan.h) through the side-effect-free exports
cwt_debug_cp4d_plan / cwt_debug_cp4d_form (no GPU needed): every row of the form table worked by hand at
two shapes, the rolling window's refusal boundary, every knob's effect inside one process, the persistent
grid, every refusal with its message, the weight gradient's workspace bound, and the kernels and grids
the launchers this plan replaced ran on the MI355X (tests/golden/cp4d_plan_parent.json; its header says
how)."""
import ctypes as C
import json
import os

import pytest

from few_shot_seg_cwt_amd import _lib, build

EARG = 1001
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "cp4d_plan_parent.json")
KNOBS = ["CWT_CP4D_MFMA", "CWT_CP4D_ROLL", "CWT_CP4D_PERSIST", "CWT_CP4D_ORDER", "CWT_CP4D_DBG", "CWT_CP4D_RDBG",
         "CWT_CP4D_WC", "CWT_CP4D_PF", "CWT_DGRAD_SCALAR", "CWT_WGRAD_SCALAR"]
FWD, DGRAD, WGRAD = 0, 1, 2
FIELDS = ["rc", "form", "cin", "cout", "mode", "pf", "gx", "gy", "gz", "wc", "nsa", "ntiles", "order", "dbg", "G", "n"]
# (B, hA, wA, hB, wB): no multiple of any tile; the MMN geometry
ODD = (2, 9, 13, 11, 7)
H60 = (1, 60, 60, 60, 60)
# worked by hand: the grids of each tiling at the two shapes
#   4 x 4 by 4 x 4 tiles (matrix-core, C1, chunked): (ceil(hB/4) ceil(wB/4), ceil(hA/4) ceil(wA/4), B)
TILE = {ODD: (3 * 2, 3 * 4, 2), H60: (225, 225, 1)}
#   2 x 8 by 2 x 8 (scalar): (ceil(hB/2) ceil(wB/8), ceil(hA/2) ceil(wA/8), B)
SCAL = {ODD: (6 * 1, 5 * 2, 2), H60: (240, 240, 1)}
#   rolling window: (ceil(hB/4) ceil(wB/12), ceil(wA/wc), B ceil(hA/4)), wc = min(30, wA)
ROLL = {ODD: (3 * 1, 1, 2 * 3), H60: (15 * 5, 2, 15)}
WC = {ODD: 13, H60: 30}
NSA = {ODD: 3, H60: 15}
NTILES = {ODD: 144, H60: 50625}          # the 4 x 4 tiles: 6 * 12 * 2, 225 * 225
WG_TILES = {ODD: 120, H60: 57600}        # the weight gradient's 2 x 8 tiles: 6 * 10 * 2, 240 * 240

MSG_NC = "cp4d layer: the channel-chunked form takes 1..32 -> 10 channels"
MSG_ROLL = "cp4d layer: no rolling-window form for this shape"
MSG_FWD = "cp4d layer: channels (1|2 -> 10, 10 -> 10, 10 -> 1) only"
MSG_DG_NC = "cp4d input gradient: 10 -> 1..32 channels"
MSG_DG_ROLL = "cp4d input gradient: no rolling-window form for this shape"
MSG_DG = "cp4d input gradient: channels (1 -> 10, 10 -> 10, 10 -> 1..32) only"
MSG_WG = "cp4d wgrad: channels (1..32 -> 10, 10 -> 10, 10 -> 1) only"
MSG_WG_SCALAR = "cp4d wgrad: channels (1|2 -> 10, 10 -> 10, 10 -> 1) only"


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load_library()


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def forms(lib):
    """form number -> (name, kernel, [template argument fields]); name -> number"""
    out, buf = {}, C.create_string_buffer(256)
    for f in range(12):
        assert lib.cwt_debug_cp4d_form(f, buf, len(buf)) == 0
        name, kernel, targs = buf.value.decode().split("\t")
        out[f] = (name, kernel, [t for t in targs.split(",") if t])
        out[name] = f
    assert lib.cwt_debug_cp4d_form(12, buf, len(buf)) == EARG and lib.cwt_debug_cp4d_form(-1, buf, len(buf)) == EARG
    return out


def plan(lib, d, shape, cin, cout, variant=0, cu=256, occ=1):
    out = (C.c_int * 16)()
    rc = lib.cwt_debug_cp4d_plan(d, *shape, cin, cout, variant, cu, occ, out)
    p = dict(zip(FIELDS, out))
    assert rc == p["rc"]
    p["msg"] = lib.cwt_last_error().decode() if rc else None
    p["grid"] = (p["gx"], p["gy"], p["gz"])
    return p


def check(lib, forms, d, shape, cin, cout, form, grid, variant=0, **want):
    p = plan(lib, d, shape, cin, cout, variant, want.pop("cu", 256), want.pop("occ", 1))
    key = (d, shape, cin, cout, variant)
    assert p["rc"] == 0, (key, p["msg"])
    assert forms[p["form"]][0] == form and p["grid"] == tuple(grid), (key, forms[p["form"]][0], p["grid"])
    assert (p["cin"], p["cout"]) == (cin, cout), key
    for k, v in want.items():
        assert p[k] == v, (key, k, p[k], v)
    return p


def refused(lib, d, shape, cin, cout, variant, msg):
    p = plan(lib, d, shape, cin, cout, variant)
    assert p["rc"] == EARG and p["msg"] == msg, ((d, shape, cin, cout, variant), p["rc"], p["msg"])


def test_form_table(forms):
    assert [forms[f][:2] for f in range(12)] == [
        ("scalar", "cp4d_layer_kernel"), ("tile_mfma", "cp4d_mfma_kernel"), ("tile_c1", "cp4d_c1_kernel"),
        ("persist_mfma", "cp4d_mfma_persist_kernel"), ("persist_c1", "cp4d_c1_persist_kernel"),
        ("roll", "cp4d_roll_kernel"), ("roll_c1", "cp4d_c1_roll_kernel"), ("nc_fwd", "cp4d_nc_fwd_kernel"),
        ("nc_dgrad", "cp4d_nc_dgrad_kernel"), ("nc_wgrad", "cp4d_nc_wgrad_kernel"),
        ("wgrad_mfma", "cp4d_wgrad_mfma_kernel"), ("wgrad_scalar", "cp4d_wgrad_kernel")]


@pytest.mark.parametrize("shape", [ODD, H60])
def test_forward_rows(lib, forms, monkeypatch, shape):
    ck = lambda *a, **k: check(lib, forms, FWD, shape, *a, **k)  # noqa: E731
    roll = dict(wc=WC[shape], nsa=NSA[shape], pf=2, mode=0)
    # chunked: variant 3 at any width, or a width with no instantiated kernel
    for cin, variant in ((1, 3), (2, 3), (10, 3), (3, 0), (9, 0), (9, 3), (32, 0)):
        ck(cin, 10, "nc_fwd", TILE[shape], variant)
    # the rolling window: the default for every instantiated width, and variant 2
    for variant in (0, 2):
        for cin in (1, 2, 10):
            ck(cin, 10, "roll", ROLL[shape], variant, **roll)
        ck(10, 1, "roll_c1", ROLL[shape], variant, **roll)
    # variant 1 (never the rolling window): persistent for 10 -> 10, else the tile forms
    G = min(NTILES[shape], 256)
    ck(10, 10, "persist_mfma", (G, 1, 1), 1, ntiles=NTILES[shape], order=1, dbg=0)
    ck(1, 10, "tile_mfma", TILE[shape], 1, mode=0)
    ck(2, 10, "tile_mfma", TILE[shape], 1, mode=0)
    ck(10, 1, "tile_c1", TILE[shape], 1)
    # CWT_CP4D_MFMA=0: the scalar kernel (variant 2 still the rolling window)
    monkeypatch.setenv("CWT_CP4D_MFMA", "0")
    for variant in (0, 1):
        for cin, cout in ((1, 10), (2, 10), (10, 10), (10, 1)):
            ck(cin, cout, "scalar", SCAL[shape], variant, mode=0)
    ck(10, 10, "roll", ROLL[shape], 2, **roll)
    ck(9, 10, "nc_fwd", TILE[shape], 0)


@pytest.mark.parametrize("shape", [ODD, H60])
def test_dgrad_rows(lib, forms, monkeypatch, shape):
    ck = lambda *a, **k: check(lib, forms, DGRAD, shape, *a, **k)  # noqa: E731
    roll = dict(wc=WC[shape], nsa=NSA[shape], pf=2, mode=1)
    for gout in (3, 9, 32):
        ck(10, gout, "nc_dgrad", TILE[shape], 0, mode=1)
    ck(10, 9, "nc_dgrad", TILE[shape], 3, mode=1)
    for gin in (1, 10):
        ck(gin, 10, "roll", ROLL[shape], 0, **roll)
        ck(gin, 10, "roll", ROLL[shape], 2, **roll)
        ck(gin, 10, "tile_mfma", TILE[shape], 1, mode=1)
    for gout in (1, 2):
        ck(10, gout, "scalar", SCAL[shape], 0, mode=1)
        ck(10, gout, "scalar", SCAL[shape], 1, mode=1)
    monkeypatch.setenv("CWT_CP4D_ROLL", "0")
    for gin in (1, 10):
        ck(gin, 10, "tile_mfma", TILE[shape], 0, mode=1)
    monkeypatch.delenv("CWT_CP4D_ROLL")
    monkeypatch.setenv("CWT_DGRAD_SCALAR", "1")
    for gin in (1, 10):
        ck(gin, 10, "scalar", SCAL[shape], 0, mode=1)
    ck(10, 9, "nc_dgrad", TILE[shape], 0, mode=1)


@pytest.mark.parametrize("shape", [ODD, H60])
def test_wgrad_rows(lib, forms, monkeypatch, shape):
    ck = lambda *a, **k: check(lib, forms, WGRAD, shape, *a, **k)  # noqa: E731
    for cin in (3, 9, 26, 32):   # chunked: G = min(256, 4 x 4 tiles), one grid column per chunk of 8 channels
        G = min(256, NTILES[shape])
        ck(cin, 10, "nc_wgrad", (G, (cin + 7) // 8, 1), G=G, n=180 * cin + 10)
    for env, form in ((None, "wgrad_mfma"), ("1", "wgrad_scalar")):
        if env:
            monkeypatch.setenv("CWT_WGRAD_SCALAR", env)
        for cin, cout, cap, n in ((10, 10, 512, 1810), (2, 10, 2048, 370), (1, 10, 2048, 190), (10, 1, 2048, 181)):
            G = min(cap, WG_TILES[shape])
            ck(cin, cout, form, (G, 1, 1), G=G, n=n)


def test_rolling_window_boundary(lib, forms):
    """The window takes a shape while hA wA hB wB * 40 bytes <= 2^30: 26,843,545 pairs yes (1,073,741,800),
    26,843,546 no; 71^4 yes (1,016,467,240), 72^4 no (1,074,954,240)."""
    thin = lambda n: (1, 1, 1, 1, n)  # noqa: E731
    cube = lambda h: (1, h, h, h, h)  # noqa: E731
    for d in (FWD, DGRAD):
        p = check(lib, forms, d, thin(26843545), 10, 10, "roll", (2236963, 1, 1), wc=1, nsa=1)
        p = check(lib, forms, d, cube(71), 10, 10, "roll", (18 * 6, 3, 18), wc=30, nsa=18)
    t72, t81 = (18 * 18, 18 * 18, 1), (21 * 21, 21 * 21, 1)
    check(lib, forms, FWD, thin(26843546), 10, 10, "persist_mfma", (256, 1, 1), ntiles=6710887)
    check(lib, forms, FWD, cube(72), 10, 10, "persist_mfma", (256, 1, 1), ntiles=18 ** 4)
    check(lib, forms, DGRAD, thin(26843546), 10, 10, "tile_mfma", (6710887, 1, 1), mode=1)
    check(lib, forms, DGRAD, cube(72), 10, 10, "tile_mfma", t72, mode=1)
    for d, msg in ((FWD, MSG_ROLL), (DGRAD, MSG_DG_ROLL)):
        refused(lib, d, thin(26843546), 10, 10, 2, msg)
        refused(lib, d, cube(72), 10, 10, 2, msg)
    # a 641^2 head (h = 81) with the default environment: none of its layers is a rolling window
    check(lib, forms, FWD, cube(81), 10, 10, "persist_mfma", (256, 1, 1), ntiles=21 ** 4, order=1)
    check(lib, forms, FWD, cube(81), 2, 10, "tile_mfma", t81, mode=0)
    check(lib, forms, FWD, cube(81), 1, 10, "tile_mfma", t81, mode=0)
    check(lib, forms, FWD, cube(81), 10, 1, "tile_c1", t81)
    check(lib, forms, DGRAD, cube(81), 10, 10, "tile_mfma", t81, mode=1)
    check(lib, forms, DGRAD, cube(81), 1, 10, "tile_mfma", t81, mode=1)


def test_knobs_in_one_process(lib, forms, monkeypatch):
    fw = lambda *a, **k: check(lib, forms, FWD, ODD, *a, **k)  # noqa: E731
    fw(10, 10, "roll", ROLL[ODD])
    monkeypatch.setenv("CWT_CP4D_ROLL", "0")    # never
    fw(10, 10, "persist_mfma", (144, 1, 1))
    fw(2, 10, "tile_mfma", TILE[ODD])
    fw(10, 1, "tile_c1", TILE[ODD])
    fw(10, 10, "roll", ROLL[ODD], 2)            # variant 2 forces it all the same
    monkeypatch.setenv("CWT_CP4D_PERSIST", "0")
    fw(10, 10, "tile_mfma", TILE[ODD])
    monkeypatch.setenv("CWT_CP4D_PERSIST", "2")
    for cin in (1, 2, 10):
        fw(cin, 10, "persist_mfma", (144, 1, 1), ntiles=144)
    fw(10, 1, "persist_c1", (144, 1, 1), ntiles=144)
    monkeypatch.setenv("CWT_CP4D_ORDER", "0")
    monkeypatch.setenv("CWT_CP4D_DBG", "3")
    fw(10, 10, "persist_mfma", (144, 1, 1), order=0, dbg=3)
    monkeypatch.setenv("CWT_CP4D_ROLL", "1")    # the 10-output layers only
    fw(10, 10, "roll", ROLL[ODD])
    fw(2, 10, "roll", ROLL[ODD])
    fw(10, 1, "persist_c1", (144, 1, 1))
    monkeypatch.delenv("CWT_CP4D_PERSIST")
    fw(10, 1, "tile_c1", TILE[ODD])
    check(lib, forms, DGRAD, ODD, 10, 10, "roll", ROLL[ODD])   # any value but 0 lets the input gradient roll
    monkeypatch.delenv("CWT_CP4D_ROLL")
    monkeypatch.setenv("CWT_CP4D_WC", "5")
    monkeypatch.setenv("CWT_CP4D_PF", "1")
    monkeypatch.setenv("CWT_CP4D_RDBG", "2")
    for d in (FWD, DGRAD):
        check(lib, forms, d, ODD, 10, 10, "roll", (3, 3, 6), wc=5, pf=1, dbg=2)
    fw(10, 1, "roll_c1", (3, 3, 6), wc=5, pf=1, dbg=2)
    monkeypatch.setenv("CWT_CP4D_WC", "0")      # clamped to 1 .. wA
    fw(10, 10, "roll", (3, 13, 6), wc=1)
    monkeypatch.setenv("CWT_CP4D_WC", "99")
    fw(10, 10, "roll", (3, 1, 6), wc=13)
    monkeypatch.setenv("CWT_CP4D_PF", "3")      # anything but 1 is depth 2
    fw(10, 10, "roll", (3, 1, 6), pf=2)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    fw(10, 10, "roll", ROLL[ODD], wc=13, pf=2, dbg=0)   # and back, in the same process
    monkeypatch.setenv("CWT_CP4D_MFMA", "0")
    fw(10, 10, "scalar", SCAL[ODD])
    check(lib, forms, DGRAD, ODD, 10, 10, "roll", ROLL[ODD])   # the forward's knob only
    monkeypatch.delenv("CWT_CP4D_MFMA")
    monkeypatch.setenv("CWT_DGRAD_SCALAR", "1")
    check(lib, forms, DGRAD, ODD, 10, 10, "scalar", SCAL[ODD], mode=1)
    check(lib, forms, DGRAD, ODD, 10, 10, "roll", ROLL[ODD], 2, mode=1)
    check(lib, forms, WGRAD, ODD, 10, 10, "wgrad_mfma", (120, 1, 1))
    monkeypatch.setenv("CWT_WGRAD_SCALAR", "1")
    check(lib, forms, WGRAD, ODD, 10, 10, "wgrad_scalar", (120, 1, 1))


@pytest.mark.parametrize("cu,occ,want60,want_odd", [(256, 1, 256, 144), (256, 2, 512, 144), (8, 1, 8, 8)])
def test_persistent_grid(lib, forms, cu, occ, want60, want_odd):
    """G = max(1, min(ntiles, max(1, occ) cu))"""
    check(lib, forms, FWD, H60, 10, 10, "persist_mfma", (want60, 1, 1), 1, cu=cu, occ=occ, ntiles=50625)
    check(lib, forms, FWD, ODD, 10, 10, "persist_mfma", (want_odd, 1, 1), 1, cu=cu, occ=occ, ntiles=144)
    check(lib, forms, FWD, H60, 10, 10, "persist_mfma", (max(1, cu), 1, 1), 1, cu=cu, occ=0)   # occ 0 counts as 1
    check(lib, forms, FWD, H60, 10, 10, "persist_mfma", (1, 1, 1), 1, cu=0, occ=occ)


@pytest.mark.parametrize("shape", [ODD, H60])
def test_refusals(lib, monkeypatch, shape):
    for cin, cout, variant in ((2, 1, 3), (10, 1, 3), (0, 10, 0), (33, 10, 0), (33, 10, 3), (9, 10, 1), (9, 10, 2),
                               (9, 1, 0), (9, 9, 0)):
        refused(lib, FWD, shape, cin, cout, variant, MSG_NC)
    for cin, cout in ((2, 1), (1, 1), (10, 2), (10, 9)):
        refused(lib, FWD, shape, cin, cout, 2, MSG_ROLL)
        for variant in (0, 1):
            refused(lib, FWD, shape, cin, cout, variant, MSG_FWD)
    for gin, gout, variant in ((10, 0, 0), (10, 33, 0), (10, 33, 3), (10, 9, 1), (10, 9, 2), (1, 10, 3), (2, 9, 3)):
        refused(lib, DGRAD, shape, gin, gout, variant, MSG_DG_NC)
    for gin, gout in ((2, 10), (1, 1), (1, 2), (5, 3), (9, 10)):
        refused(lib, DGRAD, shape, gin, gout, 0, MSG_DG)
        refused(lib, DGRAD, shape, gin, gout, 1, MSG_DG)
    for gin, gout in ((2, 10), (10, 1), (10, 2)):
        refused(lib, DGRAD, shape, gin, gout, 2, MSG_DG_ROLL)
    for cin, cout in ((0, 10), (33, 10), (5, 1), (10, 2), (9, 9), (1, 1)):
        refused(lib, WGRAD, shape, cin, cout, 0, MSG_WG)
    monkeypatch.setenv("CWT_WGRAD_SCALAR", "1")   # no chunked scalar form: the parent refused it the same way
    for cin, cout in ((9, 10), (33, 10), (5, 1)):
        refused(lib, WGRAD, shape, cin, cout, 0, MSG_WG_SCALAR)


def test_wgrad_workspace_covers_every_plan(lib, monkeypatch):
    part = lib.cwt_debug_cp4d_wgrad_part_floats()
    assert part == 1477120 == max(512 * 1810, 2048 * 370, 256 * 5770)
    big = (4, 100, 100, 100, 100)
    for scalar in (None, "1"):
        if scalar:
            monkeypatch.setenv("CWT_WGRAD_SCALAR", scalar)
        n = 0
        for shape in (ODD, H60, big):
            for cin, cout in [(c, 10) for c in range(1, 33)] + [(10, 1)]:
                p = plan(lib, WGRAD, shape, cin, cout)
                if p["rc"] == 0:
                    n += 1
                    assert p["n"] == 18 * cin * cout + cout and p["G"] * p["n"] <= part, (shape, cin, cout, p)
        assert n == (3 * 4 if scalar else 3 * 33)


def kernel_name(forms, p):
    _, kernel, targs = forms[p["form"]]
    return kernel + ("<" + ", ".join(str(p[t]) for t in targs) + ">" if targs else "")


def test_plan_names_the_launches_of_the_replaced_dispatch(lib, forms, monkeypatch):
    """MatchNet's forward runs the three layers L -> 10 -> 10 -> 1 once per symmetric branch (one stream
    each); its backward, per branch and from the last layer down, the weight gradient (its kernel, then
    cp4d_wgrad_reduce_kernel over ceil(n / 256) workgroups) and the input gradient of each layer."""
    d = json.load(open(GOLDEN))
    cu, shape = d["cu"], (d["B"],) + (d["h"],) * 4
    assert len(d["settings"]) == 10
    for name, s in d["settings"].items():
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in s["env"].items():
            monkeypatch.setenv(k, v)
        for L, run in s["runs"].items():
            ch = [int(L), 10, 10, 1]
            fwd = [(FWD, ch[i], ch[i + 1]) for i in range(3)]
            bwd = [c for _ in range(2) for i in (2, 1, 0) for c in ((WGRAD, ch[i], ch[i + 1]), (DGRAD, ch[i + 1], ch[i]))]
            main, aux = run["streams"]
            for calls, rec in ((fwd + bwd, main), (fwd, aux)):
                rec, error = list(rec), None
                for dr, cin, cout in calls:
                    p = plan(lib, dr, shape, cin, cout, 0, cu, 1)
                    key = (name, L, dr, cin, cout)
                    if p["rc"]:
                        error = p["msg"]
                        break
                    got, grid = rec.pop(0), list(p["grid"])
                    if forms[p["form"]][0].startswith("persist"):   # G = min(ntiles, k cu), k an integer >= 1
                        ks = [k for k in range(1, 17) if min(p["ntiles"], k * cu) == got[1][0]]
                        assert ks, (key, got, p["ntiles"])
                        grid = list(plan(lib, dr, shape, cin, cout, 0, cu, ks[0])["grid"])
                    assert got == [kernel_name(forms, p), grid], (key, got, kernel_name(forms, p), grid)
                    if dr == WGRAD:
                        assert rec.pop(0) == ["cp4d_wgrad_reduce_kernel", [(p["n"] + 255) // 256, 1, 1]], key
                assert rec == [], (name, L, rec)
                if calls is not fwd:
                    assert (run["error"] is None) == (error is None), (name, L, run["error"], error)
                    assert error is None or run["error"].endswith(error), (name, L, run["error"], error)
