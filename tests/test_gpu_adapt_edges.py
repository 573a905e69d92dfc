"""Every form of the support-set inner loop (adapt.hip: the per-step launches adapt_step_kernel<1|2>
and the persistent forms adapt_persist_kernel<0..6>) against the float64 reference of
tests/adapt_ref.py, at the label and unit edges: labels whose last row, last column and corner
are alive; h = 2; units of 31 and 31 + 1 owned columns; the 129th hi-res column; uc = 15; E = 64;
three and four units per workgroup across two episodes whose features differ 64-fold in scale;
1-9 steps (the accumulator slots rotate mod 3 and mod 4); flat, steep and saturated logits.

The metric is err = max|W - W_ref| / max|W_ref - W0| per episode -- on the update, not on W -- and
the bar of a case max(4 x the fp32 oracle's err, 1e-5) (adapt_ref.E32; test_adapt_ref_cpu.py proves
the table and that each wrong loop of adapt_ref.WRONG misses the bar by 10x or more).  The planner
must choose the form each row names (cwt_debug_adapt_plan): a mismatch fails, it does not skip."""
import ctypes as C
import os

import pytest
import torch

import adapt_ref as R

pytestmark = pytest.mark.gpu

FORMS = [(name, lab) for name, spec in R.CASES.items() for lab, _, _ in spec["forms"]]
RUNS = [(name, lab, reg) for name, spec in R.CASES.items() for lab, _, _ in spec["forms"] for reg in spec["regimes"]]
PERSISTENT = [(name, lab) for name, spec in R.CASES.items() for lab, form, _ in spec["forms"] if form >= 0]
NAN_FORMS = [(name, lab) for name in ("pair", "k3") for lab, _, _ in R.CASES[name]["forms"]]


def _form(name, lab):
    return next((form, knobs) for l, form, knobs in R.CASES[name]["forms"] if l == lab)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cu(dev):
    from few_shot_seg_cwt_amd import _lib
    return _lib.cu_count(dev.index)


class knobs_set:
    """The planner's knobs set as a form's row says, every other one unset; restored on exit."""

    def __init__(self, knobs, extra=None):
        self.env = {v: knobs.get(k) for k, v in R.ENV.items()}
        self.env.update(extra or {})

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        for k, v in self.env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def direct_ctx(dev):
    """A context whose step launches are enqueued directly: the default context replays one captured
    graph per geometry, whichever CWT_ADAPT_G it was captured under."""
    from few_shot_seg_cwt_amd import _lib
    with knobs_set({}, {"CWT_ADAPT_GRAPH": "0"}):
        c = _lib.new_ctx(dev.index)
    yield c
    torch.cuda.synchronize()
    _lib.destroy_ctx(c, dev.index)


_dev_cache = {}


def _on_dev(c, dev):
    key = (c["name"], c["regime"])
    if key not in _dev_cache:
        _dev_cache.clear()   # one case's inputs at a time
        _dev_cache[key] = (c["f"].to(dev).contiguous(memory_format=torch.channels_last), c["lbl"].to(dev))
    return _dev_cache[key]


def _run(c, dev, knobs, iters=None, W0=None, lbl=None, single=False, ctx=None):
    """inner_adapt_batch (single: inner_adapt, E = 1) on the case's inputs under the form's knobs."""
    from few_shot_seg_cwt_amd import _lib
    from few_shot_seg_cwt_amd.episode import inner_adapt, inner_adapt_batch
    f, l = _on_dev(c, dev)
    l = l if lbl is None else lbl.to(dev)
    W = (c["W0"] if W0 is None else W0).clone().to(dev)
    iters = c["iters"] if iters is None else iters
    with knobs_set(knobs):
        if ctx is not None:
            with _lib.using_ctx(ctx, dev.index):
                inner_adapt_batch(f, l, W, R.LR, iters)
        elif single:
            inner_adapt(f, l[0], W[0], R.LR, iters)
        else:
            inner_adapt_batch(f, l, W, R.LR, iters)
        torch.cuda.synchronize()
    return W.cpu()


def _case(name, regime, cu):
    return R.make_case(name, regime, cu)


@pytest.mark.parametrize("name,lab", FORMS, ids=[f"{n}-{l}" for n, l in FORMS])
def test_plan_takes_the_named_form(dev, cu, name, lab):
    from few_shot_seg_cwt_amd import _lib
    form, knobs = _form(name, lab)
    spec = R.CASES[name]
    n = spec["n"](cu) if callable(spec["n"]) else spec["n"]
    h = (spec["S"] - 1) // 8 + 1
    out = (C.c_int * 8)()
    with knobs_set(knobs):
        _lib.check(_lib.lib().cwt_debug_adapt_plan(spec["E"], n, h, h, R.iters_of(spec["S"]), 0, cu, out), "plan")
    assert (out[0], out[1]) == (int(form >= 0), form), f"{name}/{lab}: plan {tuple(out)}"


@pytest.mark.parametrize("name,lab,regime", RUNS, ids=[f"{n}-{l}-{r}" for n, l, r in RUNS])
def test_form_vs_float64(dev, cu, direct_ctx, name, lab, regime):
    from few_shot_seg_cwt_amd import _lib
    form, knobs = _form(name, lab)
    c = _case(name, regime, cu)
    _lib.check_status()
    W = _run(c, dev, knobs, ctx=direct_ctx if "G" in knobs else None)
    _lib.check_status()
    e = R.err(W, c["W_ref"], c["W0"])
    print(f"{name}/{lab}/{regime}: err max {float(e.max()):.3e} (episode {int(e.argmax())})  bar {c['bar']:.1e}")
    assert torch.isfinite(W).all()
    assert float(e.max()) <= c["bar"], e.tolist()


@pytest.mark.parametrize("name,lab", PERSISTENT, ids=[f"{n}-{l}" for n, l in PERSISTENT])
def test_persistent_form_repeats_bitwise(dev, cu, name, lab):
    """The persistent forms sum 64-bit fixed-point integers: the same call twice, the same bits.
    (The step launches add floats atomically and are exempt.)"""
    _, knobs = _form(name, lab)
    c = _case(name, "steep", cu)
    assert torch.equal(_run(c, dev, knobs), _run(c, dev, knobs))


@pytest.mark.parametrize("regime", R.ALL3)
@pytest.mark.parametrize("iters", R.ITERS)
@pytest.mark.parametrize("lab", R.ITERS_FORMS)
def test_step_counts(dev, cu, lab, iters, regime):
    """0 steps return W0 bitwise; 1-9 walk the accumulator slots (mod 3 / mod 4) from every start."""
    _, knobs = _form(R.ITERS_CASE, lab)
    c = _case(R.ITERS_CASE, regime, cu)
    W = _run(c, dev, knobs, iters=iters)
    if iters == 0:
        assert torch.equal(W, c["W0"])
        return
    ref = R.adapt_loop(c["f"], c["lbl"], c["W0"], R.LR, iters)
    e = float(R.err(W, ref, c["W0"]).max())
    print(f"pair/{lab}/{regime} iters {iters}: err {e:.3e}")
    assert torch.isfinite(W).all() and e <= R.FLOOR


@pytest.mark.parametrize("name,lab", [(n, l) for n, l in PERSISTENT if n in ("pair", "c129")],
                         ids=lambda v: str(v))
def test_single_entry_point_is_the_batch_of_one(dev, cu, name, lab):
    _, knobs = _form(name, lab)
    c = _case(name, "steep", cu)
    assert torch.equal(_run(c, dev, knobs, single=True), _run(c, dev, knobs))


# ---- the NaN edges ----

def _other_episode_ok(c, W):
    if c["E"] > 1:   # k3: episode 1 is untouched by episode 0's input
        e = float(R.err(W[1], c["W_ref"][1], c["W0"][1]))
        assert torch.isfinite(W[1]).all() and e <= c["bar"], e


@pytest.mark.parametrize("name,lab", NAN_FORMS, ids=[f"{n}-{l}" for n, l in NAN_FORMS])
def test_all_foreground_is_nan(dev, cu, name, lab):
    """Episode 0 all class 1: class weight nb / nf = 0 and sum w = 0, so the reference's mean is
    0 / 0 and its W NaN after one step (test_adapt_ref_cpu.test_all_foreground_is_nan)."""
    _, knobs = _form(name, lab)
    c = _case(name, "flat", cu)
    lbl = c["lbl"].clone()
    lbl[0] = 1
    W = _run(c, dev, knobs, lbl=lbl)
    assert torch.isnan(W[0]).all()
    _other_episode_ok(c, W)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("name,lab", NAN_FORMS, ids=[f"{n}-{l}" for n, l in NAN_FORMS])
def test_nonfinite_w0_is_nan(dev, cu, name, lab, bad):
    """One Inf or NaN in episode 0's W0: every gradient is NaN in the reference, so W is NaN after
    one step (test_adapt_ref_cpu.test_nonfinite_w0_is_nan); 0 steps return W0."""
    from few_shot_seg_cwt_amd import _lib
    _, knobs = _form(name, lab)
    c = _case(name, "flat", cu)
    W0 = c["W0"].clone()
    W0[0, 1, 77] = bad
    for iters in (1, c["iters"]):
        W = _run(c, dev, knobs, W0=W0, iters=iters)
        assert torch.isnan(W[0]).all(), f"iters {iters}: {int(torch.isfinite(W[0]).sum())} finite entries"
    _other_episode_ok(c, W)
    _lib.check_status()
    Wz = _run(c, dev, knobs, W0=W0, iters=0)
    assert torch.equal(Wz.nan_to_num(nan=7.0), W0.nan_to_num(nan=7.0))
