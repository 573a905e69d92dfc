"""The K-loop of conv_igemm_x6's 128x128 var 5 form, GEMM-shaped body against general body, counted in
the ISA the build's compiler and flags give (tools/x6_loop_isa.py; CPU only, one small translation
unit).  Inequalities between the two bodies compiled side by side, no fixed counts: a compiler
update moves both."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import x6_loop_isa  # noqa: E402


@pytest.fixture(scope="module")
def loops():
    res = x6_loop_isa.loop_isa([(128, 128, 5)])
    return res[(128, 128, 5, 0)], res[(128, 128, 5, x6_loop_isa.GEMM_PF)]


def test_same_matrix_and_memory_work(loops):
    general, gemm = loops
    assert general["loop"]["v_mfma"] > 0
    for c in ("v_mfma", "ds_", "buffer_", "s_barrier"):
        assert gemm["loop"][c] == general["loop"][c], c


def test_fewer_valu_and_salu(loops):
    general, gemm = loops
    valu = lambda r: r["loop"]["v_"] + r["loop"]["v_pk_"]  # noqa: E731
    assert valu(gemm) < valu(general), (valu(gemm), valu(general))
    assert gemm["loop"]["s_"] < general["loop"]["s_"], (gemm["loop"]["s_"], general["loop"]["s_"])


def test_no_more_registers_or_lds(loops):
    general, gemm = loops
    for k in ("vgpr", "agpr", "sgpr", "lds"):
        assert gemm[k] <= general[k], k
    assert gemm["spill"] == 0 and gemm["occupancy"] >= general["occupancy"]
