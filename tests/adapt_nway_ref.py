"""The float64 reference of the N-way support-set inner loop (pspnet.py:207-221 increment_inner_loop
with model_util.py:76-97 weighted_adpt_ce_loss), the input cases its tests share and the
deliberately wrong loops that keep their bars honest -- a helper, not a test, modelled on
tests/adapt_ref.py.

Plain torch on float64 and nothing from few_shot_seg_cwt_amd.  Two statements of the same loop:

  inner_adapt_nway_ref  F.conv2d -> F.interpolate(bilinear, align_corners=True) -> F.cross_entropy(
                        weight, ignore_index=255) -> autograd -> W -= lr dW, weight = 1 but for
                        weight[fg_idx] = float32(float32(bg / fg) ** tp);
  adapt_nway_loop       the same with explicit interpolation matrices and the CE gradient written
                        out.  Its keyword arguments turn it into the wrong loops (WRONG).

A label outside [0, N) is ignored like 255 (the device's rule; torch's cross_entropy rejects such
labels, so both forms map them to 255 first).  err() is relative to the UPDATE W_ref - W0.

The device bar of a case is max(4 x E32, 1e-5): E32 is the error of the same loop in float32 torch
on the CPU against the float64 one (measured when this file was made, asserted within 2x by
test_adapt_nway_ref_cpu.py); the 4x is room for another valid fp32 summation order.

The kernel tiles as the 2-way step kernel does (lo-res row pairs x 16-column blocks), so the
block-boundary cases are the same: w = 17 (S = 129) and w = 18 (S = 137).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from adapt_ref import FLOOR, REGIMES, interp_matrix

C = 512
LR = 0.1
ITERS = 20
ITERS_CASE = "pair-N17"
ITERS_SET = (0, 1, 2, 3, 4, 5)

# name -> S, N, n, fg_idx, tp, label contents, regimes
#   all: every class present; sparse: three classes present; nofg: fg_idx absent;
#   allign: every pixel 255; big: 3 % of the pixels carry labels >= N other than 255
CASES = {
    "h2-N2": dict(S=9, N=2, n=1, fg=1, tp=1.0, kind="all", regimes=("flat", "steep", "saturated")),
    "h2-N17": dict(S=9, N=17, n=5, fg=16, tp=1.1, kind="sparse", regimes=("flat", "steep")),
    "pair-N3": dict(S=17, N=3, n=1, fg=0, tp=1.0, kind="all", regimes=("flat", "steep", "saturated")),
    "pair-N16": dict(S=17, N=16, n=1, fg=1, tp=1.1, kind="all", regimes=("steep",)),
    "pair-N17": dict(S=17, N=17, n=5, fg=16, tp=1.0, kind="big", regimes=("flat", "steep", "saturated")),
    "pair-N33": dict(S=17, N=33, n=1, fg=-1, tp=1.0, kind="sparse", regimes=("steep",)),
    "pair-N64": dict(S=17, N=64, n=1, fg=63, tp=1.0, kind="all", regimes=("flat",)),
    "pair-nofg": dict(S=17, N=17, n=1, fg=5, tp=1.1, kind="nofg", regimes=("steep",)),
    "pair-allign": dict(S=17, N=3, n=1, fg=1, tp=1.0, kind="allign", regimes=("flat",)),
    "c129-N16": dict(S=129, N=16, n=1, fg=15, tp=1.0, kind="all", regimes=("steep",)),
    "c129-N62": dict(S=129, N=62, n=1, fg=61, tp=1.1, kind="all", regimes=("flat", "saturated")),
    "c137-N17": dict(S=137, N=17, n=1, fg=1, tp=1.0, kind="big", regimes=("steep",)),
    "c137-N2": dict(S=137, N=2, n=5, fg=1, tp=1.0, kind="all", regimes=("flat",)),
}

# err() of the float32 loop (inner_adapt_nway_ref, dtype float32, on the CPU) against the float64
# reference; test_adapt_nway_ref_cpu.py asserts each within 2x
E32 = {
    ("h2-N2", "flat"): 1.61e-06,
    ("h2-N2", "steep"): 2.98e-06,
    ("h2-N2", "saturated"): 4.71e-06,
    ("h2-N17", "flat"): 6.31e-07,
    ("h2-N17", "steep"): 1.41e-06,
    ("pair-N3", "flat"): 7.22e-07,
    ("pair-N3", "steep"): 2.50e-06,
    ("pair-N3", "saturated"): 4.91e-06,
    ("pair-N16", "steep"): 2.46e-06,
    ("pair-N17", "flat"): 1.01e-06,
    ("pair-N17", "steep"): 2.22e-06,
    ("pair-N17", "saturated"): 6.91e-07,
    ("pair-N33", "steep"): 1.23e-06,
    ("pair-N64", "flat"): 3.85e-07,
    ("pair-nofg", "steep"): 1.99e-06,
    ("pair-allign", "flat"): 0.00e+00,
    ("c129-N16", "steep"): 1.69e-06,
    ("c129-N62", "flat"): 5.43e-06,
    ("c129-N62", "saturated"): 1.64e-06,
    ("c137-N17", "steep"): 1.22e-06,
    ("c137-N2", "flat"): 6.50e-05,
}


def bar(name: str, regime: str) -> float:
    return max(4.0 * E32[(name, regime)], FLOOR)


def all_cases():
    return [(name, regime) for name, spec in CASES.items() for regime in spec["regimes"]]


# ---------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------

def clean_labels(lbl: torch.Tensor, N: int) -> torch.Tensor:
    """Labels outside [0, N) -> 255."""
    return torch.where((lbl >= 0) & (lbl < N), lbl, torch.full_like(lbl, 255))


def class_weight(lbl: torch.Tensor, N: int, fg_idx: int, tp: float) -> torch.Tensor:
    """float32 [N], as weighted_adpt_ce_loss builds it from the cleaned labels' bincount."""
    wt = torch.ones(N, dtype=torch.float32)
    if fg_idx >= 0:
        fg = (lbl == fg_idx).sum()
        bg = (lbl != 255).sum() - fg
        wt[fg_idx] = (bg / fg) ** tp   # int64 / int64 -> float32, ** in float32
    return wt


def adapt_nway_loop(f, lbl, W0, lr, iters, fg_idx, tp, *, wrong_class=False, no_tp=False, norm_count=False,
                    first16=False, padded=False, row0_shortcut=False, drop_last_row=False, big_as_bg=False):
    """f [n, C, h, w], lbl [n, S, S] int64, W0 [N, C] -> W [N, C] float64.  The keyword arguments
    are the wrong loops (WRONG), one line each."""
    W = torch.as_tensor(W0).detach().cpu().double().clone()
    N = W.shape[0]
    f = torch.as_tensor(f).detach().cpu().double()
    lbl = torch.as_tensor(lbl).detach().cpu().long()
    if big_as_bg:
        lbl = torch.where((lbl >= N) & (lbl != 255), torch.zeros_like(lbl), lbl)          # (h)
    lbl = clean_labels(lbl, N)
    n, S = lbl.shape[0], lbl.shape[-1]
    h, w = f.shape[-2:]
    Uy, Ux = interp_matrix(h, S), interp_matrix(w, S)
    wt = class_weight(lbl, N, fg_idx, 1.0 if no_tp else tp).double()                      # (b)
    if wrong_class and fg_idx >= 0:
        wt = torch.roll(wt, 1)                                                            # (a)
    valid = lbl != 255
    safe = torch.where(valid, lbl, torch.zeros_like(lbl))
    wy = torch.where(valid, wt[safe], torch.zeros((), dtype=torch.float64))   # an unused infinite weight never enters
    sumw = valid.double().sum() if norm_count else wy.sum()                               # (c)
    onehot = F.one_hot(safe, N).permute(0, 3, 1, 2).double()
    if drop_last_row:
        wy = wy.clone()
        wy[:, S - 1, :] = 0.0                                                             # (g)
    for _ in range(iters):
        z = torch.einsum("kc,nchw->nkhw", W, f)
        zh = Uy @ z @ Ux.t()
        if first16:
            p = torch.zeros_like(zh)
            p[:, :16] = torch.softmax(zh[:, :16], 1)                                      # (d)
        elif padded:
            npad = -(-N // 16) * 16
            zp = torch.cat([zh, zh.new_zeros(n, npad - N, S, S)], 1)
            p = torch.softmax(zp, 1)[:, :N]                                               # (e)
        else:
            p = torch.softmax(zh, 1)
        g = wy.unsqueeze(1) * (p - onehot)
        glo = Uy.t() @ g @ Ux
        dW = torch.einsum("nkhw,nchw->kc", glo, f)
        if sumw != 0:
            dW = dW / sumw
        if row0_shortcut:
            dW[0] = -dW[1]                                                                # (f)
        W -= lr * dW
    return W


def inner_adapt_nway_ref(f, lbl, W0, lr, iters, fg_idx, tp, dtype=torch.float64) -> torch.Tensor:
    """The loop through torch's own interpolate, cross_entropy and autograd in `dtype`."""
    f = torch.as_tensor(f).detach().cpu().to(dtype)
    N = W0.shape[0]
    lbl = clean_labels(torch.as_tensor(lbl).detach().cpu().long(), N)
    weight = class_weight(lbl, N, fg_idx, tp).to(dtype)
    W = torch.as_tensor(W0).detach().cpu().to(dtype).reshape(N, C, 1, 1).clone().requires_grad_(True)
    for _ in range(iters):
        out = F.interpolate(F.conv2d(f, W), size=lbl.shape[-2:], mode="bilinear", align_corners=True)
        loss = F.cross_entropy(out, lbl, weight=weight, ignore_index=255)
        g, = torch.autograd.grad(loss, W)
        with torch.no_grad():
            W -= lr * g
    return W.detach().reshape(N, C)


def err(W, W_ref, W0) -> float:
    """max|W - W_ref| / max|W_ref - W0|; NaN where W is not finite."""
    W, W_ref, W0 = (torch.as_tensor(t).detach().cpu().double().reshape(-1) for t in (W, W_ref, W0))
    return float((W - W_ref).abs().max() / (W_ref - W0).abs().max().clamp_min(1e-300))


# ---------------------------------------------------------------------------------------------
# the wrong loops
# ---------------------------------------------------------------------------------------------

# letter -> (what a kernel would have done, keyword arguments, the (case, regime)s meant to see it)
WRONG = {
    "a": ("weight on the wrong class", dict(wrong_class=True), [("pair-N3", "steep"), ("c129-N16", "steep")]),
    "b": ("tp ignored", dict(no_tp=True), [("pair-N16", "steep"), ("h2-N17", "steep")]),
    "c": ("normalised by the pixel count, not sum w", dict(norm_count=True), [("pair-N17", "steep"), ("c129-N16", "steep")]),
    "d": ("softmax over the first 16 rows only", dict(first16=True), [("pair-N17", "steep"), ("pair-N33", "steep")]),
    "e": ("padded rows inside the softmax", dict(padded=True), [("pair-N17", "flat"), ("pair-N3", "flat")]),
    "f": ("dW[0] = -dW[1], the 2-way shortcut", dict(row0_shortcut=True), [("pair-N3", "steep"), ("pair-N17", "steep")]),
    "g": ("hi-res row S-1 dropped", dict(drop_last_row=True), [("h2-N2", "steep"), ("pair-N17", "steep"), ("c137-N17", "steep")]),
    "h": ("labels >= N counted as background", dict(big_as_bg=True), [("pair-N17", "steep"), ("c137-N17", "steep")]),
}


def wrong_loop(letter: str, c: dict) -> torch.Tensor:
    return adapt_nway_loop(c["f"], c["lbl"], c["W0"], LR, c["iters"], c["fg"], c["tp"], **WRONG[letter][1])


# ---------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------

def make_labels(rng, n: int, S: int, N: int, fg: int, kind: str) -> torch.Tensor:
    """[n, S, S] int64: a coarse random class map (blocks of about S/4), 5 % of the pixels 255, the
    last row, the last column and the corner alive (a kept class each, fg among them where it is
    present at all)."""
    if kind == "allign":
        return torch.full((n, S, S), 255, dtype=torch.int64)
    if kind == "all":
        present = np.arange(N)
    elif kind == "nofg":
        present = np.array([c for c in range(N) if c != fg])
    else:   # sparse, big: three classes, fg (where there is one) among them
        present = np.array(sorted({0, max(fg, 1), N // 2}))
    g = max(2, -(-S // 4)) if kind != "all" else S   # every class present needs per-pixel draws at small S
    coarse = present[rng.integers(0, len(present), (n, g, g))]
    idx = (np.arange(S) * g) // S
    lab = coarse[:, idx][:, :, idx].astype(np.int64)
    if kind == "all":   # every class somewhere: seeded positions off the last row and column
        pos = rng.permutation((S - 1) * (S - 1))[:N]
        lab[0, pos // (S - 1), pos % (S - 1)] = np.arange(N)
    alive = lab.copy()
    lab[rng.random((n, S, S)) < 0.05] = 255
    if kind == "big":
        lab[rng.random((n, S, S)) < 0.03] = N + 3
        lab[0, 1, 1] = 254
    lab[:, S - 1, S - 1] = alive[:, S - 1, S - 1]
    p = rng.permutation(S - 1)[:2]
    lab[:, S - 1, p[0]] = alive[:, S - 1, p[0]]
    lab[:, p[1], S - 1] = alive[:, p[1], S - 1]
    if kind not in ("nofg",) and fg >= 0:
        lab[0, S - 1, p[1]] = fg
    if kind == "all":
        lab[0, pos // (S - 1), pos % (S - 1)] = np.arange(N)
    return torch.from_numpy(lab)


_cache = {}


def make_case(name: str, regime: str, with_ref: bool = True) -> dict:
    """One (case, regime): float32 f [n, C, h, h], W0 [N, C], lbl [n, S, S], the float64 reference
    after ITERS steps and the bar -- computed once and shared (never modified) by the tests."""
    key = (name, regime)
    if key in _cache and (not with_ref or "W_ref" in _cache[key]):
        return _cache[key]
    spec = CASES[name]
    S, N, n = spec["S"], spec["N"], spec["n"]
    h = (S - 1) // 8 + 1
    fstd, wstd, _ = REGIMES[regime]
    rng = np.random.default_rng([2024, list(CASES).index(name), list(REGIMES).index(regime)])
    f = torch.from_numpy((fstd * rng.standard_normal((n, C, h, h))).astype(np.float32))
    W0 = torch.from_numpy((wstd * rng.standard_normal((N, C))).astype(np.float32))
    lbl = make_labels(rng, n, S, N, spec["fg"], spec["kind"])
    c = dict(name=name, regime=regime, S=S, N=N, n=n, h=h, fg=spec["fg"], tp=spec["tp"], kind=spec["kind"], f=f,
             W0=W0, lbl=lbl, iters=ITERS)
    if with_ref:
        c["W_ref"] = adapt_nway_loop(f, lbl, W0, LR, ITERS, spec["fg"], spec["tp"])
        c["bar"] = bar(name, regime) if key in E32 else None
    _cache[key] = c
    return c


def oracle32(c: dict, iters=None) -> torch.Tensor:
    return inner_adapt_nway_ref(c["f"], c["lbl"], c["W0"], LR, c["iters"] if iters is None else iters, c["fg"],
                                c["tp"], dtype=torch.float32)
