"""The inner loop's float64 reference, cases and bars (tests/adapt_ref.py) on the CPU alone: the
reference is the oracle's loop and the reference project's recorded W; the bars test_gpu_adapt_edges.py
holds the kernels to come from the fp32 oracle's own error; every wrong loop a case is meant to see
misses that case's bar by 10x or more; and the metric of the earlier inner-loop tests, on their own
inputs, sees neither a dropped last row or column nor a linearised sigmoid."""
import os

import numpy as np
import pytest
import torch

import adapt_ref as R
from few_shot_seg_cwt_amd import synthetic as syn
from oracle import cwt_oracle as O

torch.set_num_threads(min(8, os.cpu_count() or 1))
SEED = 2021
CASES = R.all_cases()
IDS = [f"{n}-{r}" for n, r in CASES]


# ---- the reference is the oracle's loop, and the reference project's ----

def test_reference_is_the_oracle_in_float32():
    """inner_adapt_ref(dtype=float32) -- what adapt_ref.oracle32 measures E32 with -- is
    oracle.inner_adapt bitwise, class weight included."""
    c = R.make_case("pair", "steep")
    o = O.inner_adapt(c["f"], c["lbl"][0], c["W0"][0].reshape(2, R.C, 1, 1), R.LR, c["iters"],
                      O.class_weight(c["lbl"][0].numpy()))
    assert torch.equal(R.oracle32(c)[0], o.reshape(2, R.C))


def test_reference_vs_golden_small(golden_dir):
    """modules_small.npz: W after 200 steps as the reference project computed it (fp32), at the bar
    test_oracle_golden.test_inner_loop_small holds the oracle to."""
    g = dict(np.load(os.path.join(golden_dir, "modules_small.npz")))
    ep = syn.make_episode(SEED, 7, 33, 2)
    lbl = torch.from_numpy(ep["s_label"][0])
    f, W0 = torch.from_numpy(g["feat_r50_S33"]), torch.from_numpy(g["inner_W0"]).reshape(2, R.C)
    W = R.inner_adapt_ref(f, lbl, W0, 0.1, 200)
    assert R.rel_old(W, g["inner_W200"].reshape(2, R.C)) < 1e-4
    Wm = R.adapt_loop(f, lbl[None], W0[None], 0.1, 200)[0]
    assert R.rel_old(Wm, W) < 1e-12


def test_reference_vs_golden_episode(golden_dir):
    """episode_pascal_r50_1shot.npz: the adapted W of a 473^2 episode (200 steps), at the bar of
    test_oracle_golden._episode_check.  (train_pascal_r50_1shot.npz holds an adapted W as well, but of
    train-mode features with the run's Dropout2d masks, which no reference of the loop alone has.)"""
    g = dict(np.load(os.path.join(golden_dir, "episode_pascal_r50_1shot.npz")))
    cfg = syn.cfg_defaults()
    ep = syn.make_episode(SEED, 0, cfg["image_size"], cfg["shot"])
    f = O.extract_features(torch.from_numpy(ep["spprt_imgs"])[0], O.to_torch_state(syn.make_pspnet_state(50, SEED)), 50)
    lbl = torch.from_numpy(ep["s_label"])[0]
    W = R.adapt_loop(f, lbl[None], torch.from_numpy(g["e0_W0"])[None], cfg["cls_lr"], cfg["adapt_iter"])[0]
    assert R.rel_old(W, g["e0_W"]) < 1e-4


@pytest.mark.parametrize("name,regime", CASES, ids=IDS)
def test_matrix_form_is_the_interpolate_form(name, regime):
    """adapt_loop (explicit U_y z U_x^T and gradient, batched) against inner_adapt_ref (torch's
    interpolate, cross_entropy and autograd), both float64: 1e-12 of max|W|, first and last episode."""
    c = R.make_case(name, regime)
    n = c["n"]
    for e in sorted({0, c["E"] - 1}):
        W = R.inner_adapt_ref(c["f"][e * n:(e + 1) * n], c["lbl"][e], c["W0"][e], R.LR, c["iters"])
        assert R.rel_old(c["W_ref"][e], W) < 1e-12


def test_interpolation_weights_are_exact_eighths():
    for h in (2, 3, 17, 33):
        U = R.interp_matrix(h, 8 * (h - 1) + 1)
        assert torch.equal(U * 8, (U * 8).round()) and torch.equal(U.sum(1), torch.ones(U.shape[0], dtype=U.dtype))
        assert U[-1, -1] == 1.0 and U[-1, :-1].abs().max() == 0.0   # row S-1 reads lo-res row h-1 alone


# ---- the cases ----

def test_case_table():
    """Shapes, label edges and regimes (make_case asserts the label properties and the logit gap);
    over the table the corner (S-1, S-1) is foreground somewhere and background somewhere, and the
    foreground runs from one pixel to most of the image."""
    corners, shares = set(), []
    for name, regime in CASES:
        c = R.make_case(name, regime)
        assert c["S"] - 1 == 8 * (c["h"] - 1) and tuple(c["f"].shape) == (c["E"] * c["n"], R.C, c["h"], c["h"])
        corners |= set(c["lbl"][:, :, -1, -1].flatten().tolist())
        shares += ((c["lbl"] == 1).flatten(1).sum(1) / (c["lbl"] != 255).flatten(1).sum(1).double()).tolist()
        if c["E"] > 1:   # adjacent episodes differ in the exponent of max|f|
            amax = c["f"].reshape(c["E"], -1).abs().amax(1).log2()
            assert ((amax[1:] - amax[:-1]).abs() > 4).all()
    assert corners == {0, 1}
    one = R.make_case("e64", "flat")["lbl"][0]
    assert int((one == 1).sum()) == 1 and one[0, -1, -1] == 1
    assert min(shares) < 0.003 and max(shares) > 0.85
    k3, k4 = R.make_case("k3", "flat"), R.make_case("k4", "flat")
    assert (k3["n"], k4["n"]) == (130, 200)   # 520 and 800 units at 256 CUs


@pytest.mark.parametrize("name,regime", CASES, ids=IDS)
def test_e32_table_holds(name, regime):
    """The recorded error of the fp32 oracle, from which the device bar is made, within 2x."""
    c = R.make_case(name, regime)
    e32 = float(R.err(R.oracle32(c), c["W_ref"], c["W0"]).max())
    print(f"{name}/{regime}: e32 {e32:.3e} recorded {R.E32[(name, regime)]:.3e} bar {c['bar']:.3e}")
    assert R.E32[(name, regime)] / 2 <= e32 <= R.E32[(name, regime)] * 2
    assert c["bar"] == max(4 * R.E32[(name, regime)], R.FLOOR)
    upd = (c["W_ref"] - c["W0"].double()).abs().amax((1, 2)) / c["W_ref"].abs().amax((1, 2))
    assert upd.min() > 0.015   # the metric's denominator is no rounding residue


@pytest.mark.parametrize("regime", R.ALL3)
def test_iters_cases_take_the_floor(regime):
    """`pair` at 0..9 steps: the fp32 oracle is within FLOOR / 4 of the reference, so FLOOR is these
    runs' bar; 0 steps return W0; and applying the first update twice (j) misses the bar by 10x."""
    c = R.make_case(R.ITERS_CASE, regime)
    for it in R.ITERS:
        ref = R.adapt_loop(c["f"], c["lbl"], c["W0"], R.LR, it)
        if it == 0:
            assert torch.equal(ref, c["W0"].double())
            continue
        e32 = float(R.err(R.oracle32(c, it), ref, c["W0"]).max())
        ej = float(R.err(R.wrong_loop("j", c, it), ref, c["W0"]).max())
        print(f"pair/{regime} iters {it}: e32 {e32:.2e} (j) {ej:.2e}")
        assert 4 * e32 <= R.FLOOR
        assert ej >= 10 * R.FLOOR


# ---- the condition that keeps the bars honest ----

@pytest.mark.parametrize("name,regime", CASES, ids=IDS)
def test_wrong_loops_miss_the_bar_tenfold(name, regime):
    """Each wrong loop the case is meant to see, in float64: its worst episode's err -- what a
    kernel with that mistake would show -- is at least 10x the case's bar."""
    c = R.make_case(name, regime)
    for letter in R.wrong_loops_of(name, regime):
        e = float(R.err(R.wrong_loop(letter, c), c["W_ref"], c["W0"]).nan_to_num(nan=float("inf")).max())
        print(f"{name}/{regime} ({letter}) {R.WRONG[letter][0]}: err {e:.2e}  bar {c['bar']:.1e}")
        assert e >= 10 * c["bar"], (letter, R.WRONG[letter][0])


# ---- the condition on the old metric: why this file exists ----

@pytest.mark.parametrize("shots,S", [(2, 65), (3, 49), (4, 81)])
def test_old_metric_on_old_inputs_is_blind(shots, S):
    """The inputs of test_gpu_shapes.test_inner_loop_shots_vs_oracle: the last row and column of
    every label are 255, so loops (a) and (b) ARE the reference there, and the linearised sigmoid
    (i) stays under 2e-4 of max|W| (the test's bar is 1e-4; two of the three pass it)."""
    ep = syn.make_episode(SEED, 40 + shots, S, shots)
    lbl = torch.from_numpy(ep["s_label"][0])[None]
    assert (lbl[..., -1, :] == 255).all() and (lbl[..., :, -1] == 255).all()
    h = (S - 1) // 8 + 1
    f = torch.from_numpy(syn.normal(SEED, f"fs{shots}", (shots, 512, h, h), 0.1))
    W0 = torch.from_numpy(syn.normal(SEED, f"w0{shots}", (2, 512), 0.05))[None]
    c = dict(f=f, lbl=lbl, W0=W0, S=S, iters=20)
    ref = R.adapt_loop(f, lbl, W0, 0.1, 20)
    assert R.rel_old(R.wrong_loop("a", c), ref) == 0.0
    assert R.rel_old(R.wrong_loop("b", c), ref) == 0.0
    wi = R.wrong_loop("i", c)
    print(f"shots {shots} S {S}: (i) old metric {R.rel_old(wi, ref):.2e}, err {float(R.err(wi, ref, W0)):.2e}")
    assert R.rel_old(wi, ref) < 2e-4
    assert float(R.err(wi, ref, W0)) > 10 * R.FLOOR   # and the new metric sees it


# ---- the NaN edges, on the reference alone ----

def test_all_foreground_is_nan():
    """Class weight nb / nf = 0 and sum w = 0: the mean is 0 / 0 and W is NaN after one step, in
    both statements of the loop."""
    c = R.make_case("pair", "flat")
    lbl = torch.ones_like(c["lbl"])
    assert torch.isnan(R.adapt_loop(c["f"], lbl, c["W0"], R.LR, 1)).all()
    assert torch.isnan(R.inner_adapt_ref(c["f"], lbl[0], c["W0"][0], R.LR, 1)).all()
    assert torch.equal(R.adapt_loop(c["f"], lbl, c["W0"], R.LR, 0), c["W0"].double())


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_nonfinite_w0_is_nan(bad):
    c = R.make_case("pair", "flat")
    W0 = c["W0"].clone()
    W0[0, 1, 77] = bad
    for it in (1, 3):
        assert torch.isnan(R.inner_adapt_ref(c["f"], c["lbl"][0], W0[0], R.LR, it)).all()
        assert torch.isnan(R.adapt_loop(c["f"], c["lbl"], W0, R.LR, it)).all()
    assert torch.equal(R.inner_adapt_ref(c["f"], c["lbl"][0], W0[0], R.LR, 0).float(), W0[0]) or bad != bad
