"""tests/attn_ref.py on the CPU: what tests/test_gpu_attn_edges.py relies on, asserted on the
reference alone -- the float64 reference is the oracle's formula, the kernels' association is the
same function, every case has the score spread it is there for, the cases SEE a wrong softmax
(sensitivity floors: conditions, not measurements) and the fp32 error that sets the GPU bar."""
import os

import pytest
import torch

import attn_ref as A
from oracle import cwt_oracle as O

torch.set_num_threads(min(8, os.cpu_count() or 1))

UNIFORM_FLOOR = 0.05      # `uniform` moves out by at least this, row-wise
CHUNK_NORM_FLOOR = 0.05   # `chunk_norm` moves out by at least this (cases of more than one chunk)
DETACH_FLOOR = 0.5        # `detach` moves the w_qkvs gradient by at least this
ERR32_CAP = 1e-5


def test_table_reaches_every_path():
    """The shapes are the ones the kernels branch on: ATT_TPW = 8 tokens per wave, 32 per chunk,
    32 chunks per round of the combine, nv = 2 B <= 8."""
    hw = {n: v[1] for n, v in A.CASES.items()}
    assert hw["one_token"] == 1 and hw["one_wave"] < 8 and A.CASES["cap_nv8"][0] * 2 == 8
    assert hw["chunk_edge"] == A.CHUNK and hw["chunk_edge1"] == A.CHUNK + 1 and A.CHUNK < hw["two_chunks"] < 2 * A.CHUNK
    for n in ("c33_up", "c33_down", "c33_b2"):
        assert A.CASES[n][1] == 32 * A.CHUNK + 1          # 33 chunks, the last of one token
    assert A.CASES["c70"][1] == 69 * A.CHUNK + 1 and 64 < 70 <= 96   # three rounds of 32
    assert {A.CASES[n][2] for n in A.NAMES} == {1, 2, 4} and {A.CASES[n][0] for n in A.NAMES} == {1, 2, 3, 4}
    assert set(A.DROPOUT_CASES) <= set(A.NAMES)


@pytest.mark.parametrize("name", ["one_wave", "cap_nv8", "two_chunks"])
def test_reference_is_the_oracle_formula(name):
    c = A.case_reference(name)
    B, hw, heads = c["B"], c["hw"], c["heads"]
    k = c["f"].double().permute(0, 2, 1).reshape(B, A.C, hw, 1)
    with torch.no_grad():
        o = O.cwt_forward(c["q"].double(), k, k, A.to_dtype(c["tsd"]), heads)
    assert c["ref"][0].dtype == torch.float64
    assert A.rel(c["ref"][0], o) < 1e-12


@pytest.mark.parametrize("name", ["two_chunks", "chunk_edge1"])
def test_masks_apply_as_in_the_dropout_test(name):
    """With masks, `reference` is test_gpu_dropout.ref_forward (attention mask after the softmax,
    output mask on fc(.) before the residual)."""
    import math
    import torch.nn.functional as F
    B, hw, heads, _, _ = A.CASES[name]
    pa, po = A.DROPOUT_P[0]
    c = A.case_reference(name, (pa, po, A.dropout_seed(name, pa, po)))
    t = A.to_dtype(c["tsd"])
    q, kt, Wq = c["q"].double(), c["f"].double(), t["w_qkvs.weight"]
    qp = (q @ Wq.t()).view(B, 2, heads, A.C).permute(2, 0, 1, 3).reshape(-1, 2, A.C)
    kp = (kt @ Wq.t()).view(B, hw, heads, A.C).permute(2, 0, 1, 3).reshape(-1, hw, A.C)
    attn = torch.softmax(torch.bmm(qp, kp.transpose(1, 2)) / math.sqrt(A.C), dim=2) * c["m_attn"].double()
    out = torch.bmm(attn, kp).view(heads, B, 2, A.C).permute(1, 2, 0, 3).reshape(B, 2, -1)
    out = (out @ t["fc.weight"].t() + t["fc.bias"]) * c["m_out"].double()
    out = F.layer_norm(out + q, (A.C,), t["layer_norm.weight"], t["layer_norm.bias"], 1e-5)
    assert A.rel(c["ref"][0], out) < 1e-12
    assert 0.0 < float((c["m_attn"] == 0).float().mean()) < 0.3 and float((c["m_out"] == 0).float().mean()) > 0.3


@pytest.mark.parametrize("name", A.NAMES)
def test_case(name):
    """Per case: the algebra (reassociated == reference in float64, out and all gradients, 1e-12),
    the spread, the order, the sensitivity floors and err32."""
    c = A.case_reference(name)
    B, hw, heads, target, order = A.CASES[name]
    args = (c["q"], c["f"], c["tsd"], heads, c["gout"])
    ref = c["ref"]
    e = A.errors(A.reassociated(*args), ref, heads)
    assert max(e.values()) < 1e-12, e
    for x in [ref[0]] + list(ref[1].values()):
        assert bool(torch.isfinite(x).all()) and float(x.abs().max()) > 0
    assert c["f"].dtype == c["q"].dtype == torch.float32 and c["f"].shape == (B, hw, A.C)
    assert float((c["f"].double().norm(dim=2) - 1).abs().max()) < 1e-6
    print(f"{name}: B={B} hw={hw} H={heads} spread {c['spread']:.4g} (target {target}) order {order}")
    sc = c["scores"]
    if target is not None:
        assert abs(c["spread"] - target) <= 0.01 * target
    row = sc[:B, 0]                                         # (head 0, query 0) of every batch item
    if order == "up":
        assert bool((row[:, 1:] >= row[:, :-1]).all())
    elif order == "down":
        assert bool((row[:, 1:] <= row[:, :-1]).all())
    elif order == "last":
        assert bool((row.argmax(-1) == hw - 1).all()) and hw % A.CHUNK == 1
    if target is not None and target >= 8 and hw > 1:
        m_u = A.rowwise_err(A.mutant("uniform", *args)[0], ref[0], "out", heads)
        m_d = A.rowwise_err(A.mutant("detach", *args)[1]["w_qkvs.weight"], ref[1]["w_qkvs.weight"], "w_qkvs.weight",
                            heads)
        print(f"  uniform moves out by {m_u:.3g}, detach moves the w_qkvs gradient by {m_d:.3g}")
        assert m_u >= UNIFORM_FLOOR and m_d >= DETACH_FLOOR
        d = A.mutant("detach", *args)
        assert A.rel(d[0], ref[0]) < 1e-12                   # the forward of `detach` is the right one
        if hw > A.CHUNK:
            m_c = A.rowwise_err(A.mutant("chunk_norm", *args)[0], ref[0], "out", heads)
            print(f"  chunk_norm moves out by {m_c:.3g}")
            assert m_c >= CHUNK_NORM_FLOOR
        else:   # one chunk: nothing to rescale, the mutant is the reference
            assert A.rel(A.mutant("chunk_norm", *args)[0], ref[0]) < 1e-12
    worst = max(c["err32"].values())
    print(f"  err32 {worst:.3g} (reference {max(c['err32_reference'].values()):.3g}, reassociated "
          f"{max(c['err32_reassociated'].values()):.3g}) bar {c['bar']:.3g}  per tensor {c['err32']}")
    assert worst < ERR32_CAP
    assert c["bar"] == max(4.0 * worst, A.TOL)


@pytest.mark.parametrize("pa,po", A.DROPOUT_P)
@pytest.mark.parametrize("name", A.DROPOUT_CASES)
def test_dropout_case(name, pa, po):
    """The masked function: same algebra, and its own err32 under the cap."""
    drop = (pa, po, A.dropout_seed(name, pa, po))
    c = A.case_reference(name, drop)
    heads = c["heads"]
    e = A.errors(A.reassociated(c["q"], c["f"], c["tsd"], heads, c["gout"], c["m_attn"], c["m_out"]), c["ref"], heads)
    assert max(e.values()) < 1e-12, e
    plain = A.case_reference(name)
    assert A.rel(c["ref"][0], plain["ref"][0]) > 1e-2          # the masks do something
    worst = max(c["err32"].values())
    print(f"{name} p=({pa}, {po}): err32 {worst:.3g} bar {c['bar']:.3g}")
    assert worst < ERR32_CAP


def test_rowwise_metric_sees_a_small_row():
    """An error in a row 1000 x smaller than the largest is invisible to max|err| / max|ref| over
    the tensor and plain to the row-wise metric, for each row layout."""
    H = 2
    for name, shape, idx in [("out", (2, 2, A.C), (1, 0)), ("w_qkvs.weight", (H * A.C, A.C), (slice(A.C, None),)),
                             ("fc.weight", (A.C, H * A.C), (slice(None), slice(A.C, None)))]:
        b = torch.ones(shape, dtype=torch.float64)
        b[idx] = 1e-3
        a = b.clone()
        a[idx] = 1.1e-3
        assert A.rel(a, b) < 2e-4 and abs(A.rowwise_err(a, b, name, H) - 0.1) < 1e-9
    v = torch.ones(A.C, dtype=torch.float64)
    assert A.rowwise_err(v * 1.5, v, "fc.bias", H) == 0.5
