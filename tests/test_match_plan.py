"""The match pass's plan (csrc/match_plan.h) through the side-effect-free export cwt_debug_match_plan (no
GPU needed): the packed parameter table and the saved-activation layout worked by hand, every decision row
with each knob changed inside one process, the buffer table, and every refusal with its code and message."""
import ctypes as C

import pytest

from few_shot_seg_cwt_amd import _lib, build

EARG = 1001
KNOBS = ["CWT_MM_FUSE", "CWT_MATCH_BRANCH_STREAMS"]
FWD, BWD = 0, 1
MSG_ARGS = "bad argument: bad arguments (in_channel 1 .. CWT_MATCH_MAX_L = 32)"
MSG_CV4 = "bad argument: Conv4d ('cv4') layers take in_channel 1 or 2 only (CenterPivotConv4d: up to 32)"
MSG_TRAIN_CV4 = "bad argument: the training forward keeps CenterPivotConv4d ('red') activations only"


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load_library()


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def export(lib, d, B, L, h, w, sym=1, cv4=0, train=0, readout=1, d_corr=1, d_v=1, cap=1 << 14):
    buf = C.create_string_buffer(cap)
    rc = lib.cwt_debug_match_plan(d, B, L, h, w, sym, cv4, train, readout, d_corr, d_v, buf, cap)
    return rc, buf.value.decode()


def plan(lib, d, B, L, h, w, **kw):
    """-> dict(plan: the decisions, param: [(layer, name, offset, floats)], total, role: {(branch, layer):
    (Wa, ba, Wb, bb)}, buf: {tensor: (where, offset, floats, per)}, saved: total or None)"""
    rc, text = export(lib, d, B, L, h, w, **kw)
    assert rc == 0, lib.cwt_last_error().decode()
    p = dict(param=[], role={}, buf={}, saved=None)
    for f in (line.split("\t") for line in text.splitlines()):
        if f[0] == "plan":
            p["plan"] = dict(dir=f[1], **dict(kv.split("=") for kv in f[2:]))
        elif f[0] == "param" and f[1] == "total":
            p["total"] = int(f[2])
        elif f[0] == "param":
            p["param"].append((int(f[1]), f[2], int(f[3]), int(f[4])))
        elif f[0] == "role":
            p["role"][(int(f[1]), int(f[2]))] = tuple(int(x) for x in f[3:])
        elif f[0] == "buf":
            assert f[1] not in p["buf"]
            p["buf"][f[1]] = (f[2], int(f[3]), int(f[4]), f[5])
        else:
            assert f[:2] == ["saved", "total"], f
            p["saved"] = int(f[2])
    return p


def refused(lib, msg, *a, **kw):
    rc, _ = export(lib, *a, **kw)
    assert rc == EARG and lib.cwt_last_error().decode() == msg, (a, kw, rc, lib.cwt_last_error().decode())


# ---- the parameter table, worked by hand ----
def red_entries(L):
    """param_list()'s order: per layer conv1.weight [co][ci][3][3], conv1.bias, conv2.weight, conv2.bias"""
    out, off = [], 0
    for l, (ci, co) in enumerate(zip((L, 10, 10), (10, 10, 1))):
        for name, n in (("conv1.weight", 9 * ci * co), ("conv1.bias", co), ("conv2.weight", 9 * ci * co), ("conv2.bias", co)):
            out.append((l, name, off, n))
            off += n
    return out, off


@pytest.mark.parametrize("L,total", [(1, 2202), (2, 2382), (9, 2 * (9 * 9 * 10 + 10 + 900 + 10 + 90 + 1))])
def test_param_table_red(lib, L, total):
    want, off = red_entries(L)
    assert off == total
    for d in (FWD, BWD):
        p = plan(lib, d, 2, L, 5, 7, train=1)
        assert p["param"] == want and p["total"] == total
        # branch 0: conv1 over a, conv2 over b; branch 1: the two exchanged
        at = {(l, name): o for l, name, o, _ in want}
        for l in range(3):
            c1, c2 = (at[l, "conv1.weight"], at[l, "conv1.bias"]), (at[l, "conv2.weight"], at[l, "conv2.bias"])
            assert p["role"][0, l] == c1 + c2 and p["role"][1, l] == c2 + c1
    assert set(plan(lib, FWD, 2, L, 5, 7, sym=0)["role"]) == {(0, 0), (0, 1), (0, 2)}


def test_param_table_l9_by_hand(lib):
    # 2 * (9 * 9 * 10 + 10) = 1,640; 2 * (9 * 10 * 10 + 10) = 1,820; 2 * (9 * 10 * 1 + 1) = 182
    assert plan(lib, FWD, 1, 9, 6, 6)["total"] == 1640 + 1820 + 182 == 3642


@pytest.mark.parametrize("L,total", [(1, 81 * 10 + 10 + 8110 + 811), (2, 10551)])
def test_param_table_cv4(lib, L, total):
    p = plan(lib, FWD, 1, L, 5, 5, cv4=1)
    want, off = [], 0
    for l, (ci, co) in enumerate(zip((L, 10, 10), (10, 10, 1))):
        want += [(l, "weight", off, 81 * ci * co), (l, "bias", off + 81 * ci * co, co)]
        off += 81 * ci * co + co
    assert p["param"] == want and p["total"] == off == total and p["role"] == {}
    assert p["plan"]["layers"] == "cv4d"


# ---- the saved layout, worked by hand: E = B (hw)^2; x0 = E L, 21 E per branch, y = E, attn = B hw ld32(hw) ----
@pytest.mark.parametrize("B,L,h,w", [(2, 2, 5, 7), (1, 9, 6, 6)])
@pytest.mark.parametrize("sym", [0, 1])
@pytest.mark.parametrize("readout", [0, 1])
def test_saved_layout(lib, B, L, h, w, sym, readout):
    hw = h * w
    E, ld = B * hw * hw, (hw + 31) // 32 * 32
    want, off = {}, 0
    for name, n in ([("x0", E * L)] + [(f"o{br}{l}", E * c) for br in range(1 + sym) for l, c in enumerate((10, 10, 1))]
                    + [("y", E)] + ([("attn", B * hw * ld)] if readout else [])):
        want[name] = ("saved", off, n, "1")
        off += n
    assert off == E * L + (1 + sym) * 21 * E + E + readout * B * hw * ld
    if (B, L, h, w, sym, readout) == (2, 2, 5, 7, 1, 1):
        assert (E * L, 2 * 21 * E, E, B * hw * ld) == (4900, 102900, 2450, 4480) and off == 114730
    n = C.c_int64()
    assert lib.cwt_match_corr_saved_floats(B, L, h, w, sym, readout, C.byref(n)) == 0 and n.value == off
    f = plan(lib, FWD, B, L, h, w, sym=sym, train=1, readout=readout)
    assert {k: v for k, v in f["buf"].items() if v[0] == "saved"} == want and f["saved"] == off
    b = plan(lib, BWD, B, L, h, w, sym=sym, readout=readout, d_v=readout)
    assert {k: v for k, v in b["buf"].items() if v[0] == "saved"} == want and b["saved"] == off


# ---- every decision row, each knob on and off inside one process ----
def want_plan(L, sym, cv4, train, readout, fuse, streams):
    return dict(dir="fwd", mm1="direct" if L == 1 else "planar2" if fuse and L == 2 else "clast",
                layers="cv4d" if cv4 else "cp4d", branches=str(1 + sym), fork=str(int(sym and streams and not cv4)),
                mm2="plain" if not sym else "sum" if fuse and not train else "add", readout=str(readout),
                train=str(train))


def test_decisions(lib, monkeypatch):
    seen = set()
    for fuse, streams in ((0, 1), (1, 1), (0, 0), (1, 0), (0, 1)):   # and back to the default, in the same process
        for k, on, v in (("CWT_MM_FUSE", fuse, "1"), ("CWT_MATCH_BRANCH_STREAMS", not streams, "0")):
            monkeypatch.setenv(k, v) if on else monkeypatch.delenv(k, raising=False)
        for L in (1, 2, 9):
            for sym in (0, 1):
                for cv4, train in ((0, 0), (0, 1), (1, 0)):
                    if cv4 and L > 2:
                        continue
                    for readout in (0, 1):
                        p = plan(lib, FWD, 2, L, 9, 13, sym=sym, cv4=cv4, train=train, readout=readout)["plan"]
                        assert p == want_plan(L, sym, cv4, train, readout, fuse, streams), (L, sym, cv4, train, fuse)
                        seen.add((p["mm1"], p["mm2"], p["fork"]))
    assert {s[0] for s in seen} == {"direct", "planar2", "clast"} and {s[1] for s in seen} == {"plain", "add", "sum"}


def test_knobs_change_the_plan_exactly_where_stated(lib, monkeypatch):
    def grid():
        return {(L, sym, train): plan(lib, FWD, 1, L, 6, 6, sym=sym, train=train)["plan"]
                for L in (1, 2, 9) for sym in (0, 1) for train in (0, 1)}
    base = grid()
    assert all(p["fork"] == str(sym) for (L, sym, train), p in base.items())   # no fork without the symmetric mode
    monkeypatch.setenv("CWT_MM_FUSE", "1")
    fused = grid()
    for key, p in fused.items():
        L, sym, train = key
        diff = {k for k in p if p[k] != base[key][k]}
        assert diff == ({"mm1"} if L == 2 else set()) | ({"mm2"} if sym and not train else set()), (key, diff)
    monkeypatch.setenv("CWT_MM_FUSE", "2")   # on for '1' only
    assert grid() == base
    monkeypatch.delenv("CWT_MM_FUSE")
    monkeypatch.setenv("CWT_MATCH_BRANCH_STREAMS", "0")
    for key, p in grid().items():
        assert {k for k in p if p[k] != base[key][k]} == ({"fork"} if key[1] else set()), key
    monkeypatch.setenv("CWT_MATCH_BRANCH_STREAMS", "1")   # off for '0' only
    assert grid() == base


def test_backward_decisions(lib):
    for L in (1, 2, 9):
        for sym in (0, 1):
            for d_corr, d_v, readout in ((0, 0, 0), (1, 0, 0), (1, 1, 1), (0, 0, 1), (0, 1, 1)):
                p = plan(lib, BWD, 2, L, 5, 7, sym=sym, d_corr=d_corr, d_v=d_v, readout=readout)
                assert p["plan"] == dict(dir="bwd", branches=str(1 + sym), d_corr=str(d_corr), d_v=str(d_v),
                                         readout=str(readout), clast=str(int(L > 1)))
                E = 2 * 35 * 35
                ws = {k: v for k, v in p["buf"].items() if v[0] != "saved"}
                want = dict(g2d=("mb.g2d", 0, E, "1"), dy=("mb.dy", 0, E, "1"), gA=("mb.gA", 0, 10 * E, "1"),
                            gm=("mb.gm", 0, 10 * E, "1"), dx0=("mb.dx0", 0, E * L, "1"),
                            part=("mb.part", 0, lib.cwt_debug_cp4d_wgrad_part_floats(), "1"))
                if d_corr and L > 1:   # the channels-last round trip of the first MutualMatching's backward
                    want.update(xcl=("mb.xcl", 0, E * L, "1"), dxcl=("mb.dxcl", 0, E * L, "1"))
                assert ws == want


# ---- the buffer table ----
def test_buffer_table(lib, monkeypatch):
    B, L, h, w = 2, 2, 9, 13
    hw = h * w
    E, ld = B * hw * hw, (hw + 31) // 32 * 32
    vt = ("match.vt", 0, B * ld, "Cv")
    # training: x0, every layer output, y and attn in saved; no workspace but vt
    t = plan(lib, FWD, B, L, h, w, train=1)["buf"]
    assert set(t) == {"x0", "y", "attn", "vt"} | {f"o{br}{l}" for br in (0, 1) for l in (0, 1, 2)}
    assert {k for k, v in t.items() if v[0] != "saved"} == {"vt"} and t["vt"] == vt
    # inference with a fork: branch 1 in buffers of its own
    f = plan(lib, FWD, B, L, h, w)["buf"]
    assert f == dict(x0=("match.x0", 0, E * L, "1"), o00=("match.x1", 0, 10 * E, "1"), o01=("match.x2", 0, 10 * E, "1"),
                     o02=("match.y1", 0, E, "1"), o10=("match.x1b", 0, 10 * E, "1"), o11=("match.x2b", 0, 10 * E, "1"),
                     o12=("match.y2", 0, E, "1"), y=("match.y1", 0, E, "1"), attn=("match.attn", 0, B * hw * ld, "1"), vt=vt)
    # inference without one: the branches one after the other through the same two buffers
    monkeypatch.setenv("CWT_MATCH_BRANCH_STREAMS", "0")
    s = plan(lib, FWD, B, L, h, w)["buf"]
    assert s == dict(f, o10=f["o00"], o11=f["o01"])
    assert plan(lib, FWD, B, L, h, w, cv4=1)["buf"] == s   # the Conv4d stack never forks
    monkeypatch.delenv("CWT_MATCH_BRANCH_STREAMS")
    assert plan(lib, FWD, B, L, h, w, cv4=1)["buf"] == s
    one = plan(lib, FWD, B, L, h, w, sym=0, readout=0)["buf"]
    assert one == {k: f[k] for k in ("x0", "o00", "o01", "o02", "y")}
    assert not any(v[0] in ("match.x1b", "match.x2b") for p in (t, s, one) for v in p.values())


# ---- refusals ----
def test_refusals(lib):
    for d in (FWD, BWD):
        for B, L, h, w in ((0, 1, 5, 5), (1, 0, 5, 5), (1, 33, 5, 5), (1, 1, 0, 5), (1, 1, 5, 0), (1, -1, 5, 5)):
            refused(lib, MSG_ARGS, d, B, L, h, w)
            refused(lib, MSG_ARGS, d, B, L, h, w, cv4=1, train=1)   # the range first
    for L in (3, 9, 32):
        refused(lib, MSG_CV4, FWD, 1, L, 5, 5, cv4=1)
        refused(lib, MSG_CV4, FWD, 1, L, 5, 5, cv4=1, train=1)
    for L in (1, 2):
        refused(lib, MSG_TRAIN_CV4, FWD, 1, L, 5, 5, cv4=1, train=1)
        assert export(lib, FWD, 1, L, 5, 5, cv4=1)[0] == 0
    assert export(lib, FWD, 1, 32, 5, 5)[0] == 0 and export(lib, BWD, 1, 32, 5, 5, cv4=1)[0] == 0   # ignored there
    rc, _ = export(lib, 2, 1, 1, 5, 5)
    assert rc == EARG
    rc, _ = export(lib, FWD, 1, 1, 5, 5, cap=64)
    assert rc == EARG and lib.cwt_last_error().decode() == "bad argument: text buffer too small"
