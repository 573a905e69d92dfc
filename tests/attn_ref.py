"""The float64 reference of the CWT attention's TRAINING path (forward and the five parameter
gradients) and the input cases its tests share -- a helper, not a test.

The training path (cwt_attention_fwd_train / cwt_attention_bwd_train: rowdot, coldot,
attn_partial_kernel, attn_combine_kernel, layernorm_kernel, ln_bwd_kernel, outer_acc_kernel,
attn_bwd_kernel) is a three-level online softmax (wave -> workgroup -> 32-token chunk -> combine).
With the synthetic state as drawn (w_qkvs at std 1/sqrt(512), q at 0.3, unit tokens) every score
lies within +-0.07, the softmax is uniform to a few percent and exp(m_chunk - M) is 1 at every
level: a forward that never rescales between chunks, or averages the tokens, passes a 1e-4 bar.
The cases here scale w_qkvs so that the mean (max - min) score per row is 8 or 30, order the tokens
so that every chunk has another running max, and use the smallest shapes that reach each path of
the kernels (one token, fewer than 8, nv = 8, exactly one chunk, a ragged chunk of one token, 33
and 70 chunks).

reference      oracle/cwt_oracle.cwt_forward's formula on [B, hw, C] tokens, with the two dropout
               masks of tests/test_gpu_dropout.ref_forward, gradients by autograd.
reassociated   the form the kernels compute (the header comment of csrc/cwt_attn.hip) in plain
               torch; its only use is an honest fp32 rounding figure for that association.
err32          per case, the worst row-wise error of both in float32 on the CPU against float64;
               the bar of the GPU tests is max(4 x err32, 1e-5) -- from the CPU alone.
mutants        three wrong forwards; test_attn_ref_cpu.py asserts that the cases see them.

Nothing here imports few_shot_seg_cwt_amd except its synthetic generator, so the kernels are never
their own reference.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from few_shot_seg_cwt_amd import synthetic as syn

SEED = 2021
C = 512
CHUNK = 32            # tokens per workgroup of attn_partial_kernel / attn_bwd_kernel (ATT_TPB)
TOL = 1e-5            # tail_ref.TOL: the project's bar for this function's fp32 re-association
PARAMS = ["w_qkvs.weight", "layer_norm.weight", "layer_norm.bias", "fc.weight", "fc.bias"]
TENSORS = ["out"] + PARAMS

# name -> (B, hw, heads, target spread or None, token order or None)
CASES = {
    "one_token":   (1, 1, 4, None, None),      # single token: P = 1, ds = 0
    "one_wave":    (2, 7, 1, None, None),      # < 8 tokens: three idle waves (m = -inf guards)
    "cap_nv8":     (4, 9, 2, 8.0, None),       # nv = 8, coldot's cap
    "chunk_edge":  (3, 32, 4, 30.0, None),     # exactly one full chunk, near one-hot P
    "chunk_edge1": (2, 33, 1, 8.0, "up"),      # the second chunk holds one token
    "two_chunks":  (1, 63, 4, 8.0, None),      # test_gpu_parity's backward shape, a real softmax
    "c33_up":      (1, 1025, 4, 8.0, "up"),    # 33 chunks: the combine's second round has one live
    "c33_down":    (1, 1025, 4, 8.0, "down"),  # chunk; the last chunk holds one token
    "c33_b2":      (2, 1025, 2, 30.0, "last"),  # the same, B = 2, dominant token alone in the last chunk
    "c70":         (1, 2209, 4, 30.0, None),   # 70 chunks: three rounds, the last chunk one token
}
NAMES = list(CASES)
DROPOUT_CASES = ["two_chunks", "chunk_edge1", "c33_b2"]
DROPOUT_P = [(0.1, 0.5), (0.5, 0.0)]   # (p_attn, p_out)
SEEDS = {}            # name -> seed, where the default draw missed a sensitivity floor


def to_dtype(tsd, dtype=torch.float64):
    return {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in tsd.items()}


def _split(x, B, heads):
    """[B, n, heads*C] -> [heads*B, n, C] (transformer.py:62-68)."""
    n = x.shape[1]
    return x.view(B, n, heads, C).permute(2, 0, 1, 3).reshape(-1, n, C)


def scores(q, f, w_qkvs, heads):
    """The attention scores (q W_h^T)(f W_h^T)^T / sqrt(C) in float64: [heads*B, 2, hw], row h*B + b."""
    q, f, Wq = (torch.as_tensor(np.asarray(x)).double() for x in (q, f, w_qkvs))
    B = f.shape[0]
    return torch.bmm(_split(q @ Wq.t(), B, heads), _split(f @ Wq.t(), B, heads).transpose(1, 2)) / math.sqrt(C)


def _tail(o, q, p, m_out):
    y = o @ p["fc.weight"].t() + p["fc.bias"]
    if m_out is not None:
        y = y * m_out
    return F.layer_norm(y + q, (C,), p["layer_norm.weight"], p["layer_norm.bias"], 1e-5)


def _softmax(s):
    return torch.softmax(s, dim=2)


def forward(q, f, p, heads, m_attn=None, m_out=None, attn_fn=_softmax):
    """MultiHeadAttentionOne.forward (transformer.py:54-83) as oracle.cwt_oracle.cwt_forward states
    it, on tokens f [B, hw, C] (k = v); m_attn [heads*B, 2, hw] multiplies the softmax output,
    m_out [B, 2, C] multiplies fc(.) before the residual."""
    B = f.shape[0]
    Wq = p["w_qkvs.weight"]
    qp, kp = _split(q @ Wq.t(), B, heads), _split(f @ Wq.t(), B, heads)
    attn = attn_fn(torch.bmm(qp, kp.transpose(1, 2)) / math.sqrt(C))
    if m_attn is not None:
        attn = attn * m_attn
    o = torch.bmm(attn, kp).view(heads, B, 2, C).permute(1, 2, 0, 3).reshape(B, 2, -1)
    return _tail(o, q, p, m_out)


def forward_reassociated(q, f, p, heads, m_attn=None, m_out=None):
    """The kernels' association (csrc/cwt_attn.hip): a = W_h q, r = W_h^T a / sqrt(C), s = r . f,
    g = P f, o = W_h g, then fc + residual + LayerNorm."""
    B = f.shape[0]
    W = p["w_qkvs.weight"].view(heads, C, C)
    a = torch.einsum("hdc,bic->hbid", W, q)
    r = torch.einsum("hdc,hbid->hbic", W, a) / math.sqrt(C)
    s = torch.einsum("hbic,bpc->hbip", r, f)
    P = torch.softmax(s, dim=3)
    if m_attn is not None:
        P = P * m_attn.view(heads, B, 2, -1)
    g = torch.einsum("hbip,bpc->hbic", P, f)
    o = torch.einsum("hdc,hbic->bihd", W, g).reshape(B, 2, heads * C)
    return _tail(o, q, p, m_out)


def _with_grads(fn, q, f, tsd, heads, gout, m_attn, m_out, dtype, **kw):
    cast = lambda x: None if x is None else torch.as_tensor(np.asarray(x)).detach().to(dtype)  # noqa: E731
    p = {k: v.requires_grad_(True) for k, v in to_dtype(tsd, dtype).items()}
    out = fn(cast(q), cast(f), p, heads, cast(m_attn), cast(m_out), **kw)
    grads = torch.autograd.grad(out, [p[n] for n in PARAMS], cast(gout))
    return out.detach(), dict(zip(PARAMS, grads))


def reference(q, f_tokens, tsd, heads, gout, m_attn=None, m_out=None, dtype=torch.float64):
    """(out [B,2,C], {parameter name: gradient of <out, gout>}) in dtype."""
    return _with_grads(forward, q, f_tokens, tsd, heads, gout, m_attn, m_out, dtype)


def reassociated(q, f_tokens, tsd, heads, gout, m_attn=None, m_out=None, dtype=torch.float64):
    return _with_grads(forward_reassociated, q, f_tokens, tsd, heads, gout, m_attn, m_out, dtype)


# ---- three wrong forwards (float64), for test_attn_ref_cpu.py's sensitivity conditions ----
def _uniform(s):
    """The softmax replaced by a plain mean over the tokens."""
    return torch.full_like(s, 1.0 / s.shape[2])


def _chunk_norm(s):
    """No rescale between 32-token chunks: every chunk's exponentials are taken against its own max
    and the partial sums are added as they are."""
    hw = s.shape[2]
    pad = (-hw) % CHUNK
    sp = F.pad(s, (0, pad), value=-math.inf).view(s.shape[0], s.shape[1], -1, CHUNK)
    e = torch.exp(sp - sp.max(dim=3, keepdim=True).values).reshape(s.shape[0], s.shape[1], -1)[:, :, :hw]
    return e / e.sum(dim=2, keepdim=True)


def _detach(s):
    """The right forward with no gradient through the softmax (attn_bwd_kernel's whole path)."""
    return torch.softmax(s, dim=2).detach()


_MUTANTS = {"uniform": _uniform, "chunk_norm": _chunk_norm, "detach": _detach}
mutants = list(_MUTANTS)


def mutant(kind, q, f_tokens, tsd, heads, gout):
    return _with_grads(forward, q, f_tokens, tsd, heads, gout, None, None, torch.float64, attn_fn=_MUTANTS[kind])


# ---- the metric ----
def rows(x, name, heads):
    """x as [rows, elements]: each (b, i) row of `out`, each head's C x C block of the w_qkvs
    gradient, each head's column block of the fc.weight gradient, the whole of a 512-vector."""
    x = torch.as_tensor(x).detach().double().cpu()
    if name == "out":
        return x.reshape(-1, C)
    if name == "w_qkvs.weight":
        return x.reshape(heads, C * C)
    if name == "fc.weight":
        return x.reshape(C, heads, C).permute(1, 0, 2).reshape(heads, C * C)
    return x.reshape(1, -1)


def rowwise_err(a, b, name, heads) -> float:
    """max |a - b| / max |b| per row, the worst row: a small head or batch item cannot hide behind
    a large one."""
    a, b = rows(a, name, heads), rows(b, name, heads)
    return float(((a - b).abs().max(dim=1).values / b.abs().max(dim=1).values.clamp_min(1e-30)).max())


def errors(got, ref, heads) -> dict:
    """{tensor: rowwise_err} of (out, grads) pairs."""
    e = {"out": rowwise_err(got[0], ref[0], "out", heads)}
    e.update({n: rowwise_err(got[1][n], ref[1][n], n, heads) for n in PARAMS})
    return e


def rel(a, b) -> float:
    """max |a - b| / max |b| over the whole tensor (the existing CWT tests' metric)."""
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# ---- the cases ----
def spread_of(sc) -> float:
    return float((sc.max(-1).values - sc.min(-1).values).mean())


def make_case(name: str, B: int, hw: int, heads: int, spread=None, order=None) -> dict:
    """float32 inputs of one case: f [B, hw, C] unit tokens (normalised in float64, then rounded),
    q [B, 2, C] at std 0.3, gout [B, 2, C] at std 1 and the transformer state with w_qkvs scaled
    by sqrt(spread / measured spread) (scores are quadratic in it) and rounded to float32.
    order: 'up' / 'down' sort each batch item's tokens by row (head 0, query 0)'s score, so every
    chunk has another running max; 'last' moves that row's arg-max token to index hw - 1."""
    seed = SEEDS.get(name, SEED)
    f = syn.normal(seed, f"attn/{name}/f", (B, hw, C)).astype(np.float64)
    f = (f / np.linalg.norm(f, axis=2, keepdims=True)).astype(np.float32)
    q = syn.normal(seed, f"attn/{name}/q", (B, 2, C), 0.3)
    gout = syn.normal(seed, f"attn/{name}/gout", (B, 2, C), 1.0)
    tsd = dict(syn.make_transformer_state(heads, C, SEED))
    if spread is not None:
        s0 = spread_of(scores(q, f, tsd["w_qkvs.weight"], heads))
        tsd["w_qkvs.weight"] = (tsd["w_qkvs.weight"].astype(np.float64) * math.sqrt(spread / s0)).astype(np.float32)
    if order is not None:
        row = scores(q, f, tsd["w_qkvs.weight"], heads)[:B, 0].numpy()   # head 0: rows 0..B-1; query 0
        for b in range(B):
            if order == "last":
                perm = np.arange(hw)
                a = int(row[b].argmax())
                perm[[a, hw - 1]] = perm[[hw - 1, a]]
            else:
                perm = np.argsort(row[b], kind="stable")
                perm = perm[::-1] if order == "down" else perm
            f[b] = f[b][perm]
    f = np.ascontiguousarray(f)
    sc = scores(q, f, tsd["w_qkvs.weight"], heads)
    return dict(name=name, B=B, hw=hw, heads=heads, target=spread, order=order, f=torch.from_numpy(f),
                q=torch.from_numpy(q), gout=torch.from_numpy(gout), tsd=tsd, scores=sc, spread=spread_of(sc))


def masks(B, heads, hw, pa, po, seed):
    """The kernels' two dropout masks, regenerated from the seed (tests/dropout_ref.py) exactly as
    test_gpu_dropout.masks: m_attn [heads*B, 2, hw] (row h*B + b), m_out [B, 2, C]."""
    from dropout_ref import dropout_scale
    NR = 2 * heads
    ma = np.zeros((heads * B, 2, hw), np.float32)
    for b in range(B):
        for h in range(heads):
            for i in range(2):
                ma[h * B + b, i] = dropout_scale(pa, seed, 1, (b * NR + h * 2 + i) * hw + np.arange(hw))
    mo = dropout_scale(po, seed, 2, np.arange(B * 2 * C)).reshape(B, 2, C)
    return torch.from_numpy(ma), torch.from_numpy(mo)


def dropout_seed(name, pa, po) -> int:
    return 123456789 + 1000 * NAMES.index(name) + int(round(100 * pa)) + int(round(10 * po))


_cache = {}


def case_reference(name: str, drop=None) -> dict:
    """One case with its float64 reference (out, grads), err32 and bar -- computed once and shared
    (never modified) by the tests.  drop = (p_attn, p_out, seed): the same with the kernels'
    dropout masks of that seed on both.

    err32: {tensor: the worse of reference's and reassociated's float32 CPU error against the
    float64 reference, row-wise}; bar = max(4 x max err32, TOL), tail_ref.case_reference's rule."""
    key = (name, drop)
    if key in _cache:
        return _cache[key]
    B, hw, heads, spread, order = CASES[name]
    c = dict(make_case(name, B, hw, heads, spread, order))
    ma = mo = None
    if drop is not None:
        ma, mo = masks(B, heads, hw, *drop)
    args = (c["q"], c["f"], c["tsd"], heads, c["gout"], ma, mo)
    ref = reference(*args)
    e_ref = errors(reference(*args, dtype=torch.float32), ref, heads)
    e_re = errors(reassociated(*args, dtype=torch.float32), ref, heads)
    err32 = {n: max(e_ref[n], e_re[n]) for n in TENSORS}
    c.update(ref=ref, m_attn=ma, m_out=mo, err32=err32, err32_reference=e_ref, err32_reassociated=e_re,
             bar=max(4.0 * max(err32.values()), TOL))
    _cache[key] = c
    return c
