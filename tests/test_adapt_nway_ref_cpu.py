"""The N-way inner loop's float64 reference, cases and bars (tests/adapt_nway_ref.py) on the CPU
alone: the two float64 forms agree to 1e-12, every recorded E32 is reproduced within 2x, every
wrong loop misses its case's bar by 10x or more, and the edges are pinned from autograd."""
import os

import pytest
import torch
import torch.nn.functional as F

import adapt_nway_ref as R
import nway_pixel_ref as P

torch.set_num_threads(min(8, os.cpu_count() or 1))
CASES = R.all_cases()
IDS = [f"{n}-{r}" for n, r in CASES]


@pytest.mark.parametrize("name,regime", CASES, ids=IDS)
def test_forms_agree_and_e32(name, regime):
    c = R.make_case(name, regime)
    a = R.inner_adapt_nway_ref(c["f"], c["lbl"], c["W0"], R.LR, c["iters"], c["fg"], c["tp"])
    assert torch.isfinite(a).all()
    if c["kind"] == "allign":
        assert torch.equal(a, c["W0"].double()) and torch.equal(c["W_ref"], c["W0"].double())
        return
    assert R.err(a, c["W_ref"], c["W0"]) < 1e-12
    e32 = R.err(R.oracle32(c), c["W_ref"], c["W0"])
    rec = R.E32[(name, regime)]
    assert rec / 2 <= e32 <= rec * 2, (e32, rec)


@pytest.mark.parametrize("letter,name,regime", [(L, n, r) for L, (_, _, cs) in R.WRONG.items() for n, r in cs])
def test_wrong_loops_miss_the_bar(letter, name, regime):
    c = R.make_case(name, regime)
    e = R.err(R.wrong_loop(letter, c), c["W_ref"], c["W0"])
    assert e >= 10 * c["bar"], (R.WRONG[letter][0], e, c["bar"])


def test_every_case_value_is_covered():
    specs = R.CASES.values()
    assert {s["N"] for s in specs} >= {2, 3, 16, 17, 33, 62, 64}
    assert {s["n"] for s in specs} == {1, 5}
    assert {s["S"] for s in specs} >= {9, 17, 129, 137}
    assert {s["tp"] for s in specs} == {1.0, 1.1}
    assert {-1, 0, 1} <= {s["fg"] for s in specs} and any(s["fg"] == s["N"] - 1 for s in specs)
    assert {s["kind"] for s in specs} == {"all", "sparse", "nofg", "allign", "big"}
    for name, regime in CASES:
        c = R.make_case(name, regime, with_ref=False)
        lbl, N, S = c["lbl"], c["N"], c["S"]
        if c["kind"] == "allign":
            assert (lbl == 255).all()
            continue
        kept = (lbl >= 0) & (lbl < N)
        assert kept[:, S - 1, :].any() and kept[:, :, S - 1].any() and kept[:, S - 1, S - 1].all()
        if c["kind"] == "all":
            assert len(torch.unique(lbl[kept])) == N
        if c["kind"] == "nofg":
            assert not (lbl == c["fg"]).any()
        if c["kind"] == "big":
            assert ((lbl >= N) & (lbl != 255)).any()


def test_absent_fg_is_finite_in_autograd():
    """weight[fg] = inf with no such target: F.cross_entropy's loss and gradient are finite."""
    c = R.make_case("pair-nofg", "steep")
    wt = R.class_weight(R.clean_labels(c["lbl"], c["N"]), c["N"], c["fg"], c["tp"])
    assert torch.isinf(wt[c["fg"]])
    assert torch.isfinite(c["W_ref"]).all() and R.err(c["W0"], c["W_ref"], c["W0"]) == 1.0


def test_all_ignored_leaves_w_unchanged_in_autograd():
    c = R.make_case("pair-allign", "flat")
    W = c["W0"].double().reshape(c["N"], R.C, 1, 1).requires_grad_(True)
    out = F.interpolate(F.conv2d(c["f"].double(), W), size=(c["S"], c["S"]), mode="bilinear", align_corners=True)
    loss = F.cross_entropy(out, c["lbl"], weight=torch.ones(c["N"], dtype=torch.float64), ignore_index=255)
    g, = torch.autograd.grad(loss, W)
    assert torch.isnan(loss) and (g == 0).all()


def test_relabel_quirk():
    """out = s == 0 ? (am == 1 ? idx : am) : (s == 1 ? idx : s) IS the reference's two assignments:
    a background pixel predicted as base class 1 ends as idx_cls."""
    z = P.draw_logits(3, 2, 17, 3, 17)
    hi = P.upsample(z, 17)
    s = torch.randint(0, 3, (2, 17, 17), generator=torch.Generator().manual_seed(0))
    s[s == 2] = 255
    idx = 16
    lit = P.reset_spt_label_literal(s, hi, idx)
    m = hi.clone()
    m[:, idx] = -1000.0
    am = m.argmax(1)
    idx_t = torch.full_like(s, idx)
    formula = torch.where(s == 0, torch.where(am == 1, idx_t, am), torch.where(s == 1, idx_t, s))
    assert torch.equal(lit, formula)
    assert ((s == 0) & (am == 1)).any()
