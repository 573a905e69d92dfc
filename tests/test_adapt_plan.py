"""The inner loop's launch plan (csrc/adapt_plan.h) through the side-effect-free exports
cwt_debug_adapt_plan / cwt_debug_adapt_form (no GPU needed): geometries worked by hand, every
knob's effect, the table recorded from the planner this one replaced
(tests/golden/adapt_plan_parent.json; its header says how), and each form's traits."""
import ctypes as C
import json
import os

import pytest

from few_shot_seg_cwt_amd import _lib, build

EARG = 1001
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adapt_plan_parent.json")
KNOBS = ["CWT_ADAPT_PERSIST", "CWT_ADAPT_UC", "CWT_ADAPT_UPW", "CWT_ADAPT_STREAM", "CWT_ADAPT_LOCK3",
         "CWT_ADAPT_BREG", "CWT_ADAPT_RES1", "CWT_ADAPT_PR", "CWT_ADAPT_DBG"]
STEPS = (0, -1, 0, 0, 0, 0)  # the per-step launches: persist, form, G, units, ncb, uc


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load_library()


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def plan(lib, E, n, S, upw=0, cu=256, iters=200):
    """-> (persist, form, G, units, ncb, uc), (k, span)"""
    h = (S - 1) // 8 + 1
    out = (C.c_int * 8)()
    assert lib.cwt_debug_adapt_plan(E, n, h, h, iters, upw, cu, out) == 0
    return tuple(out[:6]), tuple(out[6:])


# E, n, S, upw -> persist, form, G, units, ncb, uc, k at 256 CUs.  A unit is one of the h - 1 row pairs x
# ceil((w - 1) / 31) column blocks of a shot:
HAND_CASES = [
    # 1-shot 473 (h 60): 59 x 2 = 118 units <= 128 = half the CUs: one each, form 1
    ((1, 1, 473, 0), (1, 1, 118, 118, 2, 31, 1)),
    # the pipeline's context asks for two per workgroup: 59 workgroups, both units in registers
    ((1, 1, 473, 2), (1, 5, 59, 118, 2, 31, 2)),
    # 5-shot 473: 590 units > 128 -> 2 each wanted, 256 workgroups hold up to 3: lockstep, ceil(590 / 3) = 197
    ((1, 5, 473, 0), (1, 4, 197, 590, 2, 31, 3)),
    # 1-shot 641 (h 81): 80 x 3 = 240 units > 128 -> 2 each: 120 workgroups
    ((1, 1, 641, 0), (1, 5, 120, 240, 3, 31, 2)),
    # 5-shot 641: 1200 units on 256 workgroups, up to 5 each: streamed through LDS
    ((1, 5, 641, 0), (1, 3, 256, 1200, 3, 31, 5)),
]


@pytest.mark.parametrize("args,want", HAND_CASES, ids=lambda v: "-".join(map(str, v)))
def test_geometries_worked_by_hand(lib, args, want):
    E, n, S, upw = args
    got, (k, span) = plan(lib, E, n, S, upw)
    # span bounds the episodes a run of k units can touch wherever it starts: ceil((k - 1) / units per
    # episode) + 1, so 2 from k = 2 on even with one episode
    assert got + (k, span) == want + (1 if want[6] == 1 else 2,)


def test_knobs(lib, monkeypatch):
    monkeypatch.setenv("CWT_ADAPT_RES1", "1")
    assert plan(lib, 1, 5, 641)[0] == (1, 6, 256, 1200, 3, 31)
    assert plan(lib, 1, 5, 473)[0] == (1, 4, 197, 590, 2, 31)  # only the streamed form has a resident variant
    monkeypatch.delenv("CWT_ADAPT_RES1")
    monkeypatch.setenv("CWT_ADAPT_LOCK3", "0")
    assert plan(lib, 1, 5, 473)[0] == STEPS
    monkeypatch.setenv("CWT_ADAPT_STREAM", "1")  # the stream from k = 3: 256 workgroups, not the lockstep's 197
    assert plan(lib, 1, 5, 473)[0] == (1, 3, 256, 590, 2, 31)
    monkeypatch.delenv("CWT_ADAPT_LOCK3")
    monkeypatch.delenv("CWT_ADAPT_STREAM")
    monkeypatch.setenv("CWT_ADAPT_BREG", "0")
    assert plan(lib, 1, 1, 473, 2)[0] == (1, 2, 59, 118, 2, 31)
    assert plan(lib, 1, 1, 641)[0] == (1, 2, 120, 240, 3, 31)
    assert plan(lib, 1, 1, 473)[0] == (1, 1, 118, 118, 2, 31)  # no pair, no change
    monkeypatch.delenv("CWT_ADAPT_BREG")
    monkeypatch.setenv("CWT_ADAPT_UC", "15")  # 59 columns: 4 blocks of 15, not 2 of 31 -> 236 units, 2 each
    assert plan(lib, 1, 1, 473)[0] == (1, 5, 118, 236, 4, 15)
    monkeypatch.setenv("CWT_ADAPT_UC", "16")  # neither 15 nor 31: ignored
    assert plan(lib, 1, 1, 473)[0] == (1, 1, 118, 118, 2, 31)
    monkeypatch.delenv("CWT_ADAPT_UC")
    monkeypatch.setenv("CWT_ADAPT_UPW", "2")  # the context's choice goes first
    assert plan(lib, 1, 1, 473)[0][1:3] == (5, 59) and plan(lib, 1, 1, 473, 1)[0][1:3] == (1, 118)


@pytest.mark.parametrize("args", [a for a, _ in HAND_CASES], ids=lambda v: "-".join(map(str, v)))
def test_step_launches(lib, monkeypatch, args):
    E, n, S, upw = args
    assert plan(lib, E, n, S, upw, iters=0) == (STEPS, (0, 0))
    assert plan(lib, E, n, S, upw, cu=0) == (STEPS, (0, 0))
    assert plan(lib, E, n, S, upw, cu=-1)[0] == STEPS
    monkeypatch.setenv("CWT_ADAPT_PERSIST", "0")
    assert plan(lib, E, n, S, upw)[0] == STEPS


def test_register_stream_is_opt_in(lib, monkeypatch):
    monkeypatch.setenv("CWT_ADAPT_STREAM", "0")  # 5-shot 641, no LDS stream: only form 0 is left
    assert plan(lib, 1, 5, 641)[0] == STEPS
    monkeypatch.setenv("CWT_ADAPT_PERSIST", "2")
    assert plan(lib, 1, 5, 641)[0] == (1, 0, 256, 1200, 3, 31)


def test_recorded_table_of_the_replaced_planner(lib, monkeypatch):
    d = json.load(open(GOLDEN))
    assert d["columns"] == ["E", "n", "S", "upw", "cu_count", "iters", "env", "persist", "form", "G", "units", "ncb",
                            "uc"]
    rows = d["rows"]
    assert len(rows) >= 7 * 4 * 5 * 3 * 2 and {r[8] for r in rows} == {-1, 0, 1, 2, 3, 4, 5, 6}
    bad = []
    for i, env in enumerate(d["envs"]):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for E, n, S, upw, cu, iters, e, *want in rows:
            if e == i:
                got, (k, span) = plan(lib, E, n, S, upw, cu, iters)
                if got != tuple(want):
                    bad.append(((E, n, S, upw, cu, iters, env), got, want))
                # a persistent plan's units fit its workgroups, which fit the device
                assert not got[0] or (1 <= got[2] <= cu and (k - 1) * got[2] < got[3] <= k * got[2]), (E, n, S, got)
    assert not bad, (len(bad), bad[:5])


# form -> units in lockstep, episodes a workgroup may span, lock, breg, stream, res1: the kernel body's
# constexpr block before it read pa_form_traits, evaluated by hand for NRES 0..6
#   EWK = NRES >= 2 ? 2 : NRES == 1 ? 1 : 4;  LOCK = NRES == 2 || NRES == 4;  BREG = NRES == 5;
#   STREAM = NRES == 3 || NRES == 6;  RES1 = NRES == 6;  NU = (NRES == 2 || NRES == 5) ? 2 : NRES == 4 ? 3 : 1
TRAITS = {
    0: (1, 4, 0, 0, 0, 0),
    1: (1, 1, 0, 0, 0, 0),
    2: (2, 2, 1, 0, 0, 0),
    3: (1, 2, 0, 0, 1, 0),
    4: (3, 2, 1, 0, 0, 0),
    5: (2, 2, 0, 1, 0, 0),
    6: (1, 2, 0, 0, 1, 1),
}


def test_form_traits(lib):
    out = (C.c_int * 6)()
    for form, want in TRAITS.items():
        assert lib.cwt_debug_adapt_form(form, out) == 0
        assert tuple(out) == want, form
    assert lib.cwt_debug_adapt_form(-1, out) == EARG and lib.cwt_debug_adapt_form(7, out) == EARG
    assert b"no such inner-loop form" in lib.cwt_last_error()


def test_span_stays_within_the_forms_episode_copies(lib):
    """Several small episodes: a workgroup's units may touch more than one, never more than the form's
    body keeps W copies for."""
    out = (C.c_int * 6)()
    seen = set()
    for E in (2, 4, 8, 16, 64):
        for S in (17, 33, 65):
            for cu in (4, 64, 256):
                got, (k, span) = plan(lib, E, 1, S, 0, cu)
                if got[0]:
                    assert lib.cwt_debug_adapt_form(got[1], out) == 0
                    assert 1 <= span <= out[1], (E, S, cu, got, span)
                    seen.add(span)
    assert 2 in seen
