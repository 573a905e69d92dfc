"""The float64 reference of the episode tail (test.py:190-224 after the inner loop) and the input
cases the tail's tests share -- a helper, not a test.

The reference composes oracle/cwt_oracle.py (pinned against the reference's own fixtures by
test_oracle_golden.py) on float64 tensors: normalize, cwt_forward in its unfolded form, classify,
upsample, intersection_union, F.cross_entropy(ignore_index=255, reduction="sum") and the valid
count.  Nothing here imports few_shot_seg_cwt_amd, so the kernels are never their own reference;
the transformer state is passed in by the tests.

The cases (make_case) are the data and shapes of tests/test_gpu_tail_edges.py; test_tail_ref_cpu.py
asserts the properties the GPU file relies on (tie shares, low-margin caps, the dominating token's
score spread) on the reference alone.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import cwt_oracle as O

HEADS = 4
C = 512
TOL = 1e-5            # test_gpu_tail.TOL: the project's bar for this function (fp32 re-association)
MASK_CAP = 0.005      # masked (low-margin) pixels over valid pixels, at most
CHUNK = 32            # tokens per chunk of the kernels' token pass (TL_TPB / TOK_TPB)

# (B, h) with S = 8 (h - 1) + 1: one wave's tokens, one chunk, a ragged last chunk, > 32 chunks
SHAPES = [(1, 2), (3, 5), (2, 6), (4, 9), (1, 17), (1, 33), (1, 37)]
DATA_SHAPES = [(2, 6), (1, 17)]
DATA_CASES = ["sparse", "dead_first", "dead_last", "dead_chunk", "scale_lo", "scale_hi", "dominant", "wtie", "exact"]
CASES = [("benign", B, h) for B, h in SHAPES] + [(n, B, h) for n in DATA_CASES for B, h in DATA_SHAPES]
MEASURED_BAR = ("scale_lo", "scale_hi", "dominant")   # bar = max(4 x the fp32 oracle's error, TOL)
EXACT0 = ("wtie", "exact")                            # pred_q0 is exact in fp32: iut0 with no masking
SCALE = {"scale_lo": 1e-3, "scale_hi": 1e3}
SPREAD = 30.0         # the dominating-token case: mean score spread per (query, head) row
SEEDS = {}            # (name, B, h) -> seed, where the default seed missed the low-margin cap


def to64(tsd, dtype=torch.float64):
    return {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in tsd.items()}


def side(h: int) -> int:
    return 8 * (h - 1) + 1


def metrics_reference(logits, target, dtype=torch.float64):
    """(iut [B,3,2], ce_sum [B], ce_count [B]) of [B,2,h,w] logits against a [B,S,S] target:
    bilinear(align_corners) upsample, argmax, intersection_union, CE(ignore 255) sum and the
    valid count (util.py:237-308; test.py:214-224), in dtype."""
    lg = torch.as_tensor(logits).detach().cpu().to(dtype)
    lab = torch.as_tensor(target).detach().cpu().long()
    B, S = lg.shape[0], lab.shape[-1]
    with torch.no_grad():
        up = O.upsample(lg, S)
        iut = torch.stack([torch.stack(O.intersection_union(up[b].argmax(0), lab[b])) for b in range(B)])
        ce_sum = torch.stack([F.cross_entropy(up[b:b + 1], lab[b:b + 1], ignore_index=255, reduction="sum")
                              for b in range(B)]).double()
        ce_count = (lab != 255).flatten(1).sum(1).double()
    return iut.double(), ce_sum, ce_count


def classify_rows(W, f):
    """O.classify one class row at a time: the two rows then go through the same routine in the
    same order, so coinciding rows of W give bitwise coinciding logit planes -- an exact tie, as
    in exact arithmetic -- whichever way a BLAS blocks a two-row product."""
    return torch.cat([O.classify(W[:, i:i + 1].contiguous(), f) for i in range(W.shape[1])], 1)


def tail_reference(W, f_q, q_label, tsd, heads: int = HEADS, dtype=torch.float64):
    """(W', pred_q, pred_q0, iut [B,3,2], ce_sum [B], ce_count [B], iut0 [B,3,2]) of
    W [B,2,C], f_q [B,C,h,w], q_label [B,S,S] (0 / 1 / 255) and the transformer state, in dtype."""
    W = torch.as_tensor(W).detach().cpu().to(dtype)
    f = torch.as_tensor(f_q).detach().cpu().to(dtype).contiguous()
    lab = torch.as_tensor(q_label).detach().cpu().long()
    tsd = to64(tsd, dtype)
    with torch.no_grad():
        fh = O.normalize(f)
        W2 = O.cwt_forward(W, fh, fh, tsd, heads)
        pq = classify_rows(W2, fh)
        pq0 = classify_rows(W, f)
    iut, ce_sum, ce_count = metrics_reference(pq, lab, dtype)
    iut0, _, _ = metrics_reference(pq0, lab, dtype)
    return W2, pq, pq0, iut, ce_sum, ce_count, iut0


def margins(pred, S: int):
    """|l1 - l0| of the upsampled logits, [B,S,S], in pred's dtype."""
    up = O.upsample(pred, S)
    return (up[:, 1] - up[:, 0]).abs()


def scores(W, f_q, tsd, heads: int = HEADS):
    """The attention scores (q W_h^T)(f_hat W_h^T)^T / sqrt(C) in float64: [heads*B, 2, hw]
    (transformer.py:23-30 before the softmax)."""
    W = torch.as_tensor(W).double()
    fh = O.normalize(torch.as_tensor(f_q).double())
    B = fh.shape[0]
    k = fh.reshape(B, C, -1).permute(0, 2, 1)
    Wq = to64(tsd)["w_qkvs.weight"]
    qp = (W @ Wq.t()).view(B, 2, heads, C).permute(2, 0, 1, 3).reshape(-1, 2, C)
    kp = (k @ Wq.t()).view(B, k.shape[1], heads, C).permute(2, 0, 1, 3).reshape(-1, k.shape[1], C)
    return torch.bmm(qp, kp.transpose(1, 2)) / math.sqrt(C)


def integer_logits(rng, B: int, h: int, w: int):
    """[B,2,h,w] float32 integers in [-8, 8], plane 1 copied from plane 0 on the left half: with
    S - 1 = 8 (h - 1) the align_corners weights are multiples of 1/8, so the upsampled values are
    multiples of 1/64 below 2^4 -- exact in fp32 -- and the left half ties exactly."""
    lg = rng.integers(-8, 9, size=(B, 2, h, w)).astype(np.float32)
    lg[:, 1, :, : (w + 1) // 2] = lg[:, 0, :, : (w + 1) // 2]
    return torch.from_numpy(lg)


def make_labels(rng, B: int, S: int):
    """0 / 1 / 255 in test_gpu_tail._labels' proportions (30 % class 1, 5 % ignored); with B >= 2
    item 1 is all 255, with B >= 3 the last item is all class 1."""
    lab = (rng.random((B, S, S)) < 0.3).astype(np.int64)
    lab[rng.random((B, S, S)) < 0.05] = 255
    if B >= 2:
        lab[1] = 255
    if B >= 3:
        lab[B - 1] = 1
    return torch.from_numpy(lab)


def dead_tokens(name: str, hw: int):
    """Token indices (row-major over h x h) that are all zero in the case."""
    if name == "dead_first":
        return [0]
    if name == "dead_last":
        return [hw - 1]
    if name == "dead_chunk":
        c = min(3, hw // CHUNK - 1)
        return list(range(c * CHUNK, (c + 1) * CHUNK))
    if name == "exact":   # its block of zero tokens: the first two rows
        return list(range(2 * math.isqrt(hw)))
    return []


def make_case(name: str, B: int, h: int, tsd) -> dict:
    """float32 inputs of one case: f [B,C,h,h], W [B,2,C], label [B,S,S]; every case of a shape
    starts from the same benign draw (|N(0,1)| features, W at 0.05)."""
    seed = SEEDS.get((name, B, h), 0)
    rng = np.random.default_rng([2021, B, h, seed])
    f = np.abs(rng.standard_normal((B, C, h, h))).astype(np.float32)
    W = (0.05 * rng.standard_normal((B, 2, C))).astype(np.float32)
    lab = make_labels(rng, B, side(h))
    hw = h * h
    ft = f.reshape(B, C, hw)   # a view: token p is ft[:, :, p]
    if name == "sparse":
        f[rng.random(f.shape) < 0.7] = 0.0
    elif name.startswith("dead"):
        ft[:, :, dead_tokens(name, hw)] = 0.0
    elif name in SCALE:
        f = (f * np.float32(SCALE[name])).astype(np.float32)
    elif name == "wtie":
        W[:, 1] = W[:, 0]
    elif name == "exact":
        f = rng.integers(0, 4, size=f.shape).astype(np.float32)
        f[:, :, :2, :] = 0.0   # a block of zero tokens: its upsampled interior ties at 0 == 0
        W = rng.integers(-1, 2, size=W.shape).astype(np.float32)
    elif name == "dominant":
        # the last token (alone or nearly so in the ragged last chunk) points along the mean score
        # direction of the eight (query, head) rows; W is then scaled to the wanted spread
        Wq = np.asarray(tsd["w_qkvs.weight"], np.float64).reshape(HEADS, C, C)
        for b in range(B):
            r = np.stack([Wq[hd].T @ (Wq[hd] @ W[b, i].astype(np.float64)) for i in range(2) for hd in range(HEADS)])
            d = (r / np.linalg.norm(r, axis=1, keepdims=True)).sum(0)
            ft[b, :, hw - 1] = np.maximum(d, 0.0).astype(np.float32) * 10.0
        sc = scores(torch.from_numpy(W), torch.from_numpy(f), tsd)
        spread = float((sc.max(-1).values - sc.min(-1).values).mean())
        W = (W * np.float32(SPREAD / spread)).astype(np.float32)
    return dict(name=name, B=B, h=h, S=side(h), f=torch.from_numpy(np.ascontiguousarray(f)),
                W=torch.from_numpy(np.ascontiguousarray(W)), label=lab)


def relerr(a, b) -> float:
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


_cache = {}


def case_reference(name: str, B: int, h: int, tsd) -> dict:
    """One case with its float64 reference, its logits bar, the low-margin mask and the reference
    of the masked target -- computed once and shared (never modified) by the tests.

    bar: TOL, or for MEASURED_BAR cases max(4 x err32, TOL) with err32 the error of the oracle's
    fp32 CPU path against the float64 reference on the same inputs.
    mask: pixels with |l1 - l0| <= 2 bar max|logits| in the reference's upsampled pred_q, and in
    its pred_q0 unless that is exact (EXACT0); they are set to 255 in `target`, which both the
    kernels and `ref` (the reference on the masked target) get.  `share` = masked / valid pixels."""
    key = (name, B, h)
    if key in _cache:
        return _cache[key]
    c = make_case(name, B, h, tsd)
    W2, pq, pq0, *_ = tail_reference(c["W"], c["f"], c["label"], tsd)
    bar, err32 = TOL, None
    if name in MEASURED_BAR:
        o32 = tail_reference(c["W"], c["f"], c["label"], tsd, dtype=torch.float32)
        err32 = dict(W2=relerr(o32[0], W2), pred_q=relerr(o32[1], pq), pred_q0=relerr(o32[2], pq0))
        bar = max(4.0 * max(err32.values()), TOL)
    S = c["S"]
    m, m0 = margins(pq, S), margins(pq0, S)
    low = m <= 2.0 * bar * float(pq.abs().max())
    if name not in EXACT0:
        low |= m0 <= 2.0 * bar * float(pq0.abs().max())
    if name == "wtie":
        # W's rows coincide, so W' rows and pred_q's planes coincide up to rounding on every
        # pixel: pred_q's counts are not defined by the reference here and are not compared
        low = torch.zeros_like(low)
    dead = dead_tokens(name, h * h)
    if dead:
        # a pixel all of whose taps (of non-zero weight) are dead tokens has both logits exactly 0
        # on either side: an exact tie, kept in the comparison
        alive = torch.ones(1, 1, h * h, dtype=torch.float64)
        alive[0, 0, dead] = 0.0
        low &= O.upsample(alive.view(1, 1, h, h), S)[0] != 0
    valid = c["label"] != 255
    target = c["label"].clone()
    target[low] = 255
    share = float((low & valid).sum()) / max(float(valid.sum()), 1.0)
    tie0 = float(((m0 == 0) & valid).sum()) / max(float(valid.sum()), 1.0)
    ref = tail_reference(c["W"], c["f"], target, tsd)
    c.update(bar=bar, err32=err32, target=target, share=share, tie0=tie0, ref=ref, margin=m, margin0=m0)
    _cache[key] = c
    return c
