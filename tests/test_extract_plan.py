"""The extractor's plan (csrc/extract_plan.h, csrc/backbone_arch.h) through the side-effect-free exports
cwt_debug_extract_plan / cwt_debug_extract_mode / cwt_debug_backbone_arch (no GPU needed): the profile
records of the run_extract this plan replaced, recorded on the MI355X
(tests/golden/extract_plan_parent.json; its header says how), rows worked by hand, every knob's effect,
the mode traits and the architecture's key list."""
import ctypes as C
import json
import os
import re

import pytest

from few_shot_seg_cwt_amd import _lib, build

EARG = 1001
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "extract_plan_parent.json")
KNOBS = ["CWT_CONV_F32D", "CWT_WINO", "CWT_FUSE_DOWN", "CWT_FUSE_SPLITK_WINO", "CWT_PPM_SPLITK"]
FP32, BF16 = 0, 1                 # CWT_CONV_FP32 / CWT_CONV_BF16
X3S, F32, X6 = 0, 1, 2            # CWT_CONV_ARITH_*
# the golden's mode -> (precision, conv_arith, train_bn); f32 is f32d with CWT_CONV_F32D=0 in its env
MODES = {"x6": (FP32, X6, 0), "f32d": (FP32, F32, 0), "f32": (FP32, F32, 0), "x3s": (FP32, X3S, 0),
         "b16": (BF16, X6, 0), "train": (FP32, X6, 1)}


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load_library()


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def export(lib, layers, N, S, mode="x6", mid=False):
    """-> [(level, name, flops, bytes)] in order, {workspace: floats}, {form name: value}"""
    prec, arith, tb = MODES[mode]
    buf = C.create_string_buffer(1 << 18)
    assert lib.cwt_debug_extract_plan(layers, N, S, prec, arith, tb, int(mid), buf, len(buf)) == 0, lib.cwt_last_error()
    recs, ws, forms = [], {}, {}
    for line in buf.value.decode().splitlines():
        f = line.split("\t")
        if f[0] == "ws":
            ws[f[1]] = int(f[2])
        elif f[0] == "form":
            forms[f[1]] = f[2]
        else:
            recs.append((int(f[0]), f[1], float(f[2]), float(f[3])))
    return recs, ws, forms


def records(lib, *a, level=3, **k):
    return [list(r[1:]) for r in export(lib, *a, **k)[0] if r[0] <= level]


def golden():
    return json.load(open(GOLDEN))


def test_records_equal_the_replaced_run_extract(lib, monkeypatch):
    d = golden()
    assert d["columns"] == ["name", "flops", "bytes"]
    seen = set()
    for c in d["configs"]:
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in c["env"].items():
            monkeypatch.setenv(k, v)
        got = records(lib, c["layers"], c["N"], c["S"], c["mode"], c["mid"], level=c["level"])
        want = [d["records"][i] for i in c["records"]]
        key = (c["layers"], c["N"], c["S"], c["mode"], tuple(sorted(c["env"].items())), c["mid"], c["level"])
        # names as strings, FLOPs and bytes as floats, all with ==
        assert got == want, (key, [(g, w) for g, w in zip(got, want) if g != w][:3], len(got), len(want))
        seen.add(key)
    # the issue's table: workload (x6, b16) x (R50, R101) x 5 shapes; small: 6 modes + 5 knob settings at 2 shapes; mid
    for layers in (50, 101):
        for N, S in ((1, 473), (2, 473), (5, 473), (1, 641), (5, 641)):
            for mode in ("x6", "b16"):
                assert (layers, N, S, mode, (), False, 3) in seen
    for N, S in ((2, 33), (2, 65)):
        for mode in ("x6", "f32d", "x3s", "b16", "train"):
            assert (50, N, S, mode, (), False, 3) in seen
        assert (50, N, S, "f32", (("CWT_CONV_F32D", "0"),), False, 3) in seen
        for env in ({"CWT_FUSE_DOWN": "0"}, {"CWT_FUSE_SPLITK_WINO": "0"}, {"CWT_FUSE_DOWN": "0", "CWT_FUSE_SPLITK_WINO": "0"},
                    {"CWT_WINO": "0"}, {"CWT_PPM_SPLITK": "1"}):
            assert (50, N, S, "x6", tuple(sorted(env.items())), False, 3) in seen
    assert (50, 2, 33, "x6", (), True, 3) in seen


def wino_in_nsplit(N, name, nbytes, d):
    """The partial planes a wino_in record's bytes account for: bytes = 4 N H W Ci nsplit + 4 P T Ci (F(2x2): P = 16,
    T = N d^2 ceil(ceil(H / d) / 2)^2 tiles)."""
    Ci, H = map(int, re.match(r"wino_in (\d+)@(\d+)", name).groups())
    t = -(-(-(-H // d)) // 2)
    T = N * d * d * t * t
    n, rem = divmod(nbytes - 4.0 * 16 * T * Ci, 4.0 * N * H * H * Ci)
    assert rem == 0 and n >= 1, (name, nbytes)
    return int(n)


def test_golden_is_not_vacuous():
    """The small shapes (2, 33) and (2, 65) of the x6 pass already hold all four: a split-K conv, a two-source
    conv, a Winograd conv and a Winograd input transform that sums split-K partials (no further shape was needed)."""
    d = golden()
    for S in (33, 65):
        c = next(c for c in d["configs"] if (c["N"], c["S"], c["mode"], c["env"], c["mid"], c["level"]) ==
                 (2, S, "x6", {}, False, 3))
        R = [d["records"][i] for i in c["records"]]
        names = [r[0] for r in R]
        assert any("+splitk" in n for n in names)
        assert any(re.search(r"> \d+\+\d+x\d+k1", n) for n in names)
        assert any(n.startswith("conv_igemm_x6w<") for n in names)
        # the conv in front of record i names the dilation: layer3 d2, layer4 d4, the bottleneck d1
        fused = []
        for i, r in enumerate(R):
            if r[0].startswith("wino_in "):
                dil = int(re.search(r"s1d(\d+)@", R[i - 1][0]).group(1))
                fused.append(wino_in_nsplit(2, r[0], r[2], dil))
        assert max(fused) > 1 and min(fused) == 1, fused


def test_rows_worked_by_hand(lib):
    """1-shot 473 R50 x6: 473 -> 237 (stem) -> 119 (max pool) -> 60 (layer2's stride); layer3 / layer4 dilated."""
    recs, ws, forms = export(lib, 50, 1, 473)
    by_name = {}
    for level, name, fl, by in recs:
        by_name.setdefault(name.split(" ", 1)[-1] if name.startswith("conv_") else name, []).append((level, name, fl, by))
    # the whole-pass record comes first, at level 1
    assert recs[0][:2] == (1, "extract_features N=1 S=473")
    # layer4 conv2: 512 -> 512, 3x3 d4, in the Winograd form F(2x2) (Ci >= 256), stage tag 4; 3 blocks
    l4 = by_name["512x512k3s1d4@60"]
    assert len(l4) == 3 and all(re.fullmatch(r"conv_igemm_x6w<\d+,\d+,4> 512x512k3s1d4@60", n) and lv == 2
                                for lv, n, _, _ in l4)
    # its FLOPs stay the direct conv's: 2 M Co K with M = 60 * 60, K = 9 * 512
    assert l4[0][2] == 2.0 * 3600 * 512 * 4608
    # layer2 conv2 at Ci 128: direct (the first block's at stride 2 from 119, three more at stride 1)
    l2 = by_name["128x128k3s2d1@60"] + by_name["128x128k3s1d1@60"]
    assert len(l2) == 4 and all(re.match(r"conv_igemm_x6<\d+,\d+,2>", n) and lv == 2 for lv, n, _, _ in l2)
    # the bottleneck: stage 6, level 1, over the 2048 layer4 channels
    (bott,) = by_name["2048x512k3s1d1@60"]
    assert bott[0] == 1 and re.match(r"conv_igemm_x6w<\d+,\d+,6> ", bott[1])
    assert [n for lv, n, _, _ in recs if lv == 1] == [recs[0][1], bott[1]]
    # the Winograd sub-records at level 3, three behind each Winograd conv: layer3 6, layer4 3, the bottleneck
    wino = [(lv, n) for lv, n, _, _ in recs if n.startswith("wino_")]
    assert len(wino) == 3 * (6 + 3 + 1) and all(lv == 3 for lv, _ in wino)
    assert all(lv == 2 for lv, n, _, _ in recs if not n.startswith(("wino_", "extract_features")) and n != bott[1])
    # workspace: A / B hold the larger of the stem's 237^2 x 128 and layer4's 60^2 x 2048 maps (the latter); the
    # PPM field F 60^2 x 512; no training-mode BN, no partials of it
    assert ws["bb.A"] == ws["bb.B"] == 60 * 60 * 2048 > 237 * 237 * 128
    assert ws["bb.F"] == 60 * 60 * 512 and ws["bn.part"] == 0
    assert forms == {"ppm_gemm": "few_rows"}


def diff(a, b):
    """The records a has more of than b, and those b has more of than a (multiset differences)"""
    def minus(p, q):
        q, out = [tuple(r) for r in q], []
        for r in p:
            if tuple(r) in q:
                q.remove(tuple(r))
            else:
                out.append(r)
        return out
    return minus(a, b), minus(b, a)


def test_each_knob_changes_what_it_says_and_nothing_else(lib, monkeypatch):
    base = records(lib, 50, 2, 33)
    whole = base[0][0]
    dual = re.compile(r"conv_igemm_x6<\d+,\d+,\d>(\+splitk\d+)? \d+\+\d+x\d+k1s1d1@\d+")
    assert sum(bool(dual.fullmatch(r[0])) for r in base) == 4   # one block with a downsample conv per layer

    monkeypatch.setenv("CWT_FUSE_DOWN", "0")   # the four two-source convs become conv3 + downsample conv
    gone, new = diff(base, records(lib, 50, 2, 33))
    assert sorted(r[0] for r in gone if r[0] != whole) == sorted(r[0] for r in base if dual.fullmatch(r[0]))
    new = [r[0] for r in new if r[0] != whole]
    assert len(new) == 8 and all(re.fullmatch(r"conv_igemm_x6<\d+,\d+,\d>(\+splitk\d+)? \d+x\d+k1s[12]d1@\d+", n)
                                 for n in new)
    monkeypatch.delenv("CWT_FUSE_DOWN")

    monkeypatch.setenv("CWT_FUSE_SPLITK_WINO", "0")   # the input transforms read reduced maps: fewer bytes, same launches
    off = records(lib, 50, 2, 33)
    assert [r[0] for r in off] == [r[0] for r in base]
    changed = [(a, b) for a, b in zip(base, off) if a != b]
    assert changed and all(a[0].startswith("wino_in ") and b[2] < a[2] and b[1] == a[1] for a, b in changed)
    monkeypatch.delenv("CWT_FUSE_SPLITK_WINO")

    monkeypatch.setenv("CWT_WINO", "0")   # every 3x3 conv direct: no Winograd name, no sub-record
    gone, new = diff(base, records(lib, 50, 2, 33))
    assert gone and all(r[0].startswith(("conv_igemm_x6w<", "wino_")) for r in gone)
    assert len(new) == 10 and all(re.fullmatch(r"conv_igemm_x6<\d+,\d+,\d>(\+splitk\d+)? \d+x\d+k3s1d\d@\d+", r[0])
                                  for r in new)
    monkeypatch.setenv("CWT_WINO", "2")   # F(2x2) wherever its weights exist: the default's choice at these widths
    assert records(lib, 50, 2, 33) == base
    monkeypatch.delenv("CWT_WINO")

    monkeypatch.setenv("CWT_PPM_SPLITK", "1")   # the PPM GEMMs' form alone; no record names it
    recs, _, forms = export(lib, 50, 2, 33)
    assert [list(r[1:]) for r in recs] == base and forms == {"ppm_gemm": "splitk"}
    monkeypatch.delenv("CWT_PPM_SPLITK")
    assert export(lib, 50, 2, 33)[2] == {"ppm_gemm": "few_rows"}
    assert export(lib, 50, 5, 33)[2] == {"ppm_gemm": "splitk"}   # 250 cells > the few-row form's 200

    monkeypatch.setenv("CWT_CONV_F32D", "0")   # the exact-fp32 family alone moves to the register-staged kernel
    assert records(lib, 50, 2, 33) == base
    assert records(lib, 50, 2, 33, "x3s") != base
    f32 = records(lib, 50, 2, 33, "f32")
    assert all(r[0].startswith("conv_igemm_f32<") for r in f32 if r[0].startswith("conv_"))
    monkeypatch.delenv("CWT_CONV_F32D")
    f32d = records(lib, 50, 2, 33, "f32d")
    assert all(r[0].startswith("conv_igemm_f32d<") for r in f32d if r[0].startswith("conv_"))
    # the same convs in the same order, whatever tile each family takes
    assert [r[0].split(" ", 1)[-1] for r in f32] == [r[0].split(" ", 1)[-1] for r in f32d]


def test_mode_selection(lib):
    """A training-mode BN pass runs exact fp32 on the register-staged kernel in either precision and arithmetic; a
    bf16 backbone runs bf16 under any arithmetic."""
    def family(prec, arith, tb):
        buf = C.create_string_buffer(1 << 18)
        assert lib.cwt_debug_extract_plan(50, 2, 33, prec, arith, tb, 0, buf, len(buf)) == 0
        return {ln.split("\t")[1].split("<")[0] for ln in buf.value.decode().splitlines() if "\tconv_igemm" in ln}

    for arith in (X3S, F32, X6):
        assert family(FP32, arith, 1) == family(BF16, arith, 1) == {"conv_igemm_f32"}
        assert family(BF16, arith, 0) == {"conv_igemm_b16"}
    assert family(FP32, X3S, 0) == {"conv_igemm_x3s"}
    assert family(FP32, F32, 0) == {"conv_igemm_f32d"}
    assert family(FP32, X6, 0) == {"conv_igemm_x6", "conv_igemm_x6w"}


# mode -> activation layout (0 fp32 NHWC, 1 S-layout, 2 bf16 NHWC), prec, on the LDS-DMA body, every conv writes
# fp32, accounted bytes per element: the booleans of the run_extract this plan replaced, evaluated by hand
#   layout = b16 ? 2 : conv_split ? 1 : 0;  prec = b16 ? 1 : conv_split ? 3 : x6 ? 6 : 0;
#   dma = b16 || conv_split || f32d || x6;  fp32 outputs = !(b16 || conv_split);  eb = b16 ? 2 : 4
TRAITS = {
    0: (0, 0, 0, 1, 4),   # f32
    1: (0, 0, 1, 1, 4),   # f32d
    2: (0, 6, 1, 1, 4),   # x6
    3: (1, 3, 1, 0, 4),   # x3s
    4: (2, 1, 1, 0, 2),   # b16
}


def test_mode_traits(lib):
    out = (C.c_int * 5)()
    for mode, want in TRAITS.items():
        assert lib.cwt_debug_extract_mode(mode, out) == 0
        assert tuple(out) == want, mode
    assert lib.cwt_debug_extract_mode(-1, out) == EARG and lib.cwt_debug_extract_mode(5, out) == EARG


@pytest.mark.parametrize("layers", [50, 101])
def test_architecture_lists_the_reference_keys(lib, layers):
    buf = C.create_string_buffer(1 << 16)
    assert lib.cwt_debug_backbone_arch(layers, buf, len(buf)) == 0
    got = []
    for line in buf.value.decode().splitlines():
        w, bn, Ci, Co, k, stride, pad, dil = line.split("\t")
        Ci, Co, k = int(Ci), int(Co), int(k)
        got.append([w, [Co, Ci, k, k]])
        got += [[f"{bn}.{p}", [Co]] for p in ("weight", "bias", "running_mean", "running_var")]
        got.append([f"{bn}.num_batches_tracked", []])
    ref = json.load(open(os.path.join(HERE, "golden", f"keys_r{layers}.json")))
    assert got == [e for e in ref if e[0] not in ("gamma", "classifier.weight")]
    assert lib.cwt_debug_backbone_arch(34, buf, len(buf)) == EARG


def test_export_refuses_bad_arguments(lib):
    buf = C.create_string_buffer(1 << 18)
    assert lib.cwt_debug_extract_plan(34, 2, 33, FP32, X6, 0, 0, buf, len(buf)) == EARG
    assert lib.cwt_debug_extract_plan(50, 2, 34, FP32, X6, 0, 0, buf, len(buf)) == EARG
    assert lib.cwt_debug_extract_plan(50, 2, 33, FP32, X6, 0, 0, buf, 16) == EARG
    assert b"buffer too small" in lib.cwt_last_error()
