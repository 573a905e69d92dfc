"""The form table and plan lookup of the LDS-DMA conv family (csrc/conv_forms.h), through the two
side-effect-free exports cwt_debug_conv_form / cwt_debug_conv_plan (no GPU needed): every measured
plan row comes back as written and names a form that exists, shapes in no table get the heuristic's
plan, and the admitted (prec, tile, var) set and each form's wave layout are pinned here."""
import ctypes as C
import os
import re

import pytest

from few_shot_seg_cwt_amd import _lib, build

CSRC = os.path.join(os.path.dirname(os.path.abspath(build.__file__)), "csrc")
EARG = 1001
TABLES = {3: ("conv_plans_x3s.inc", 32), 1: ("conv_plans_b16.inc", 64), 0: ("conv_plans_f32d.inc", 32),
          6: ("conv_plans_x6.inc", 32)}  # prec: measured table, K-tile depth
TILES = [(256, 256), (256, 128), (128, 256), (128, 128), (128, 64), (64, 128), (64, 64)]


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load_library()


def cdiv(a, b):
    return (a + b - 1) // b


def plan(lib, prec, M, Co, K, batch=0):
    out = (C.c_int * 5)()
    rc = lib.cwt_debug_conv_plan(prec, M, Co, K, batch, out)
    return rc, tuple(out)


def form(lib, prec, bm, bn, var):
    out = (C.c_int * 4)()
    rc = lib.cwt_debug_conv_form(prec, bm, bn, var, out)
    assert rc in (0, EARG), rc
    return tuple(out) if rc == 0 else None


def table_rows(name):
    """The data rows {M, Co, K, bm, bn, nsplit[, var[, batch]]} of a conv_plans_*.inc"""
    rows = []
    for line in open(os.path.join(CSRC, name)):
        m = re.match(r"\s*\{([^}]*)\}", line)
        if m:
            v = [int(t) for t in m.group(1).split(",")]
            rows.append(tuple(v + [0] * (8 - len(v))))
    return rows


@pytest.mark.parametrize("prec", sorted(TABLES))
def test_measured_rows_come_back_and_name_a_form(lib, prec):
    name, kdepth = TABLES[prec]
    rows = table_rows(name)
    assert rows, name
    for M, Co, K, bm, bn, nsplit, var, batch in rows:
        assert Co % bn == 0, (name, M, Co, K)
        kt = K // kdepth
        rc, got = plan(lib, prec, M, Co, K, batch)
        assert rc == 0, (name, M, Co, K, batch, rc)  # CWT_EARG: the row's form has no table row
        assert got[:3] == (bm, bn, var), (name, M, Co, K, batch, got)
        assert got[3] == cdiv(kt, cdiv(kt, nsplit)), (name, M, Co, K, batch, got)
        assert got[4] == cdiv(kt, nsplit), (name, M, Co, K, batch, got)
        assert form(lib, prec, bm, bn, var) is not None, (name, bm, bn, var)


def heuristic(M, Co, ktiles, batch=0):
    """plan_heuristic_s (batch = 0) and the batched fallback of the Winograd forms' GEMMs, written
    out: the largest tile giving >= 200 workgroups, splitting K by powers of two (>= 8 K-tiles per
    split) where the output grid is too small; batched: over the whole batch, no split-K."""
    best = None
    for bm, bn in TILES:
        if Co % bn:
            continue
        tiles = cdiv(M, bm) * (Co // bn)
        ks = 1
        while not batch and tiles * ks < 200 and ktiles // (ks * 2) >= 8:
            ks *= 2
        kt = cdiv(ktiles, ks)
        best = (bm, bn, 0, cdiv(ktiles, kt), kt)
        if tiles * best[3] * max(batch, 1) >= 200:
            return best
    return best


# prec, M, Co, K, batch -> bm, bn, var, nsplit, kt_per_split, worked by hand:
HEURISTIC_CASES = [
    # split-K: 144 K-tiles, Co = 64 admits 128x64 (1 tile) and 64x64 (2 tiles); K halves while a split
    # keeps >= 8 K-tiles: 16 splits of 9; neither reaches 200 workgroups, the last candidate stays
    ((3, 100, 64, 4608, 0), (64, 64, 0, 16, 9)),
    # the same conv in plain bf16: 64-deep K-tiles, 72 of them: 8 splits of 9
    ((1, 100, 64, 4608, 0), (64, 64, 0, 8, 9)),
    # the largest tile: 391 x 2 tiles of 256x256 already exceed 200 workgroups
    ((6, 100000, 512, 512, 0), (256, 256, 0, 1, 16)),
    # batched, 16 GEMMs: 256x256 64, 256x128 and 128x256 128 workgroups, 128x128 8 x 2 x 16 = 256
    ((6, 1000, 256, 256, 16), (128, 128, 0, 1, 8)),
]


@pytest.mark.parametrize("args,want", HEURISTIC_CASES, ids=lambda v: "-".join(map(str, v)))
def test_shape_in_no_table_gets_the_heuristic(lib, args, want):
    prec, M, Co, K, batch = args
    assert not [r for r in table_rows(TABLES[prec][0]) if r[:3] == (M, Co, K) and r[7] == batch]
    assert heuristic(M, Co, K // TABLES[prec][1], batch) == want
    assert plan(lib, prec, M, Co, K, batch) == (0, want)


# (bm, bn, var) -> (WAVES_M, WAVES_N, NSTG, PF), transcribed from the launch ladders this table replaced
FORMS_ALL = {
    (256, 256, 0): (2, 4, 2, 0), (256, 256, 1): (2, 4, 2, 0), (256, 256, 2): (2, 4, 2, 0),
    (256, 128, 0): (4, 2, 3, 0), (256, 128, 1): (4, 2, 3, 1), (256, 128, 2): (4, 2, 3, 1),
    (128, 256, 0): (2, 4, 3, 0), (128, 256, 1): (2, 4, 3, 1), (128, 256, 2): (2, 4, 3, 1),
    (128, 128, 0): (2, 2, 3, 0), (128, 128, 1): (2, 2, 3, 1), (128, 128, 2): (2, 4, 3, 1),
    (128, 128, 4): (2, 2, 2, 0),
    (128, 64, 0): (2, 2, 3, 0), (128, 64, 1): (2, 2, 3, 1), (128, 64, 2): (4, 2, 3, 1),
    (64, 128, 0): (2, 2, 3, 0), (64, 128, 1): (2, 2, 3, 1), (64, 128, 2): (2, 4, 3, 1),
    (64, 64, 0): (2, 2, 4, 0), (64, 64, 1): (2, 2, 4, 1), (64, 64, 2): (2, 4, 4, 1),
    # timing study, fixed tiles
    (64, 64, 8): (2, 2, 4, 2), (64, 64, 9): (2, 2, 4, 4), (128, 128, 10): (2, 4, 3, 3), (128, 128, 11): (2, 4, 3, 5),
}
FORMS_X6_ONLY = {
    (256, 256, 3): (4, 2, 2, 0), (256, 128, 3): (8, 1, 2, 0), (128, 256, 3): (4, 2, 2, 0),
    (128, 128, 3): (4, 1, 3, 0), (128, 128, 5): (4, 1, 2, 0),
    (128, 64, 3): (4, 1, 3, 0), (128, 64, 5): (4, 1, 2, 0),
    (64, 128, 3): (4, 1, 3, 0), (64, 128, 5): (4, 1, 2, 0),
    (64, 64, 3): (4, 1, 4, 0),
    # timing study
    (128, 128, 12): (4, 1, 2, 16), (128, 128, 14): (4, 1, 2, 4), (128, 128, 15): (4, 1, 2, 2),
    (128, 128, 16): (4, 1, 2, 6), (128, 128, 17): (4, 1, 2, 38), (128, 128, 18): (4, 1, 2, 64),
    (256, 256, 13): (4, 2, 2, 16),
}


@pytest.mark.parametrize("prec", [0, 1, 3, 6])
def test_admitted_forms_are_exactly_the_list(lib, prec):
    want = {**FORMS_ALL, **(FORMS_X6_ONLY if prec == 6 else {})}
    got = {}
    for bm in (64, 128, 256):
        for bn in (64, 128, 256):
            for var in range(21):
                f = form(lib, prec, bm, bn, var)
                if f is not None:
                    got[(bm, bn, var)] = f
    assert sorted(got) == sorted(want)
    assert got == want


def test_no_form_outside_the_families(lib):
    assert form(lib, 2, 128, 128, 0) is None and form(lib, 3, 128, 128, 6) is None
    assert form(lib, 6, 96, 128, 0) is None and form(lib, 6, 128, 128, -1) is None
    assert b"no such conv form" in lib.cwt_last_error()
