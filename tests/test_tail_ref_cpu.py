"""tests/tail_ref.py on the CPU: the float64 tail reference against the oracle's own fp32 path and
the reference's fixture, and the properties of the shared cases that tests/test_gpu_tail_edges.py
relies on when it demands equal counts with no slack -- all asserted on the reference alone."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tail_ref as R
from few_shot_seg_cwt_amd import synthetic as syn
from oracle import cwt_oracle as O

torch.set_num_threads(min(8, os.cpu_count() or 1))
SEED = 2021


@pytest.fixture(scope="module")
def tsd():
    return syn.make_transformer_state(4, 512, SEED)


def test_helper_fp32_is_the_oracle_path(golden_dir, tsd):
    """The helper at float32 is the oracle's episode path (run_inference_episode's tail) on the
    small fixture's features; its W' meets the reference module's recorded output, and the
    float64 run agrees with the fp32 one to fp32 rounding."""
    g = dict(np.load(os.path.join(golden_dir, "modules_small.npz")))
    f = torch.from_numpy(g["feat_r50_S33"])                                   # [2,512,5,5]
    W = torch.stack([torch.from_numpy(g["mha_h4_q"][0]), torch.from_numpy(g["inner_W200"]).reshape(2, 512)])
    lab = torch.from_numpy(syn.make_episode(SEED, 7, 33, 2)["s_label"][0])    # [2,33,33]
    W2, pq, pq0, iut, ces, cec, iut0 = R.tail_reference(W, f, lab, tsd, dtype=torch.float32)
    ts = O.to_torch_state(tsd)
    with torch.no_grad():
        fqn = O.normalize(f)
        W2o = O.cwt_forward(W, fqn, fqn, ts, 4)
        pqo = O.classify(W2o, fqn)
        for b in range(2):
            pq0o = F.conv2d(f[b:b + 1], W[b].reshape(2, 512, 1, 1))
            assert R.relerr(pq0[b:b + 1], pq0o) < 1e-6
            up, up0 = O.upsample(pqo[b:b + 1], 33), O.upsample(pq0o, 33)
            i, u, t = O.intersection_union(up.argmax(1)[0], lab[b])
            i0, u0, t0 = O.intersection_union(up0.argmax(1)[0], lab[b])
            assert torch.equal(iut[b], torch.stack([i, u, t]).double())
            assert torch.equal(iut0[b], torch.stack([i0, u0, t0]).double())
            ce = F.cross_entropy(up, lab[b:b + 1], ignore_index=255, reduction="sum")
            assert abs(float(ces[b]) - float(ce)) <= 1e-6 * abs(float(ce))
            assert float(cec[b]) == float((lab[b] != 255).sum())
    assert torch.equal(W2, W2o) and R.relerr(pq, pqo) < 1e-6   # (the helper classifies row by row)
    assert R.relerr(W2[:1], g["mha_h4_out"]) < 1e-5
    r64 = R.tail_reference(W, f, lab, tsd)
    assert r64[0].dtype == torch.float64
    assert max(R.relerr(W2, r64[0]), R.relerr(pq, r64[1]), R.relerr(pq0, r64[2])) < 1e-5
    assert torch.equal(r64[5], cec) and torch.equal(r64[3][:, 2], iut[:, 2])


@pytest.mark.parametrize("h,S", [(2, 9), (5, 33), (33, 257), (37, 289)])
def test_integer_upsample_is_exact_and_ties(h, S):
    """S - 1 = 8 (h - 1) and integer logits in [-8, 8]: the fp32 and float64 F.interpolate results
    are bitwise equal, and at least 1 % of the pixels tie exactly -- so a kernel's counts on such
    logits must equal the reference's, ties (class 0) included."""
    lg = R.integer_logits(np.random.default_rng([SEED, h, S]), 2, h, h)
    up32, up64 = O.upsample(lg, S), O.upsample(lg.double(), S)
    assert up32.dtype == torch.float32 and torch.equal(up32.double(), up64)
    ties = float((up64[:, 1] == up64[:, 0]).double().mean())
    print(f"h={h} S={S}: {ties:.3f} of the pixels tie")
    assert ties >= 0.01
    assert torch.equal(up32.argmax(1), up64.argmax(1))
    assert bool((up64.argmax(1)[up64[:, 1] == up64[:, 0]] == 0).all())   # argmax: class 0 on a tie


@pytest.mark.parametrize("name,B,h", R.CASES)
def test_case_properties(tsd, name, B, h):
    """Every case (and seed) of the GPU file: the masked low-margin pixels are at most 0.5 % of the
    valid ones; the bar is the project's 1e-5 or 4 x the fp32 oracle's own error; and each data
    case has the property it is there for."""
    c = R.case_reference(name, B, h, tsd)
    W2, pq, pq0, iut, ces, cec, iut0 = c["ref"]
    print(f"{name} B={B} h={h}: bar {c['bar']:.3g} fp32-oracle error {c['err32']} masked share {c['share']:.5f} "
          f"exact ties in pred_q0 {c['tie0']:.4f}")
    assert c["share"] <= R.MASK_CAP
    assert c["bar"] == R.TOL if name not in R.MEASURED_BAR else c["bar"] >= R.TOL
    if name in R.MEASURED_BAR:
        assert c["bar"] == max(4.0 * max(c["err32"].values()), R.TOL)
    for x in (W2, pq, pq0, ces):
        assert bool(torch.isfinite(x).all())
    hw = h * h
    if B >= 2:     # the all-255 item: no valid pixel, no CE, no counts
        assert float(cec[1]) == 0 and float(ces[1]) == 0 and float(iut[1].abs().sum() + iut0[1].abs().sum()) == 0
    if B >= 3:     # the all-class-1 item (before masking)
        assert bool((c["label"][B - 1] == 1).all()) and float(iut[B - 1, 2, 0]) == 0
    dead = R.dead_tokens(name, hw)
    if dead:
        fh = O.normalize(c["f"].double()).reshape(B, 512, hw)
        assert float(fh[:, :, dead].abs().max()) == 0.0
        assert float(pq.reshape(B, 2, hw)[:, :, dead].abs().max()) == 0.0
        assert float(pq0.reshape(B, 2, hw)[:, :, dead].abs().max()) == 0.0
    if name == "sparse":
        assert 0.69 < float((c["f"] == 0).double().mean()) < 0.71
    if name in R.SCALE:   # the normalisation cancels the scale; the baseline logits carry it
        base = R.case_reference("benign", B, h, tsd)["ref"]
        assert R.relerr(W2, base[0]) < 1e-6 and R.relerr(pq, base[1]) < 1e-6
        assert R.relerr(pq0, base[2] * R.SCALE[name]) < 1e-6
    if name == "dominant":
        sc = R.scores(c["W"], c["f"], tsd)
        spread = sc.max(-1).values - sc.min(-1).values
        print(f"score spread per row: {[round(float(s), 1) for s in spread.flatten()]}")
        assert abs(float(spread.mean()) - R.SPREAD) < 1.0 and 20.0 < float(spread.min()) and float(spread.max()) < 45.0
        assert bool((sc.argmax(-1) == hw - 1).all())          # the last token, in the ragged last chunk
        assert hw % R.CHUNK != 0
    if name == "wtie":
        assert torch.equal(pq0[:, 0], pq0[:, 1])
        assert c["tie0"] == 1.0 and float(iut0[:, 0, 1].sum() + iut0[:, 1, 1].sum() - iut0[:, 2, 1].sum()) == 0
    if name == "exact":
        assert c["tie0"] >= 0.01
        # integer W . f and eighths weights: the reference's fp32 path is bitwise the float64 one
        p32 = O.classify(c["W"], c["f"])
        assert torch.equal(p32.double(), pq0) and torch.equal(O.upsample(p32, c["S"]).double(), O.upsample(pq0, c["S"]))
