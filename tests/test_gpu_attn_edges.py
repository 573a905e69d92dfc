"""The CWT attention's TRAINING path (cwt_attention_fwd_train / cwt_attention_bwd_train: rowdot,
coldot, attn_partial_kernel, attn_combine_kernel, layernorm_kernel, ln_bwd_kernel, outer_acc_kernel,
attn_bwd_kernel) against the float64 reference of tests/attn_ref.py, where the softmax matters:
w_qkvs scaled to a score spread of 8 or 30 per row, tokens ordered so that every chunk has another
running max, and the smallest shapes that reach each path (one token, fewer than 8, nv = 8 with
B = 4, exactly one chunk, a last chunk of one token, 33 and 70 chunks, B >= 2 with H = 2 and 4).

Metric: max |err| / max |ref| per row (each (b, i) row of out, each head's block of the w_qkvs and
fc.weight gradients), the worst row.  Bar per case: max(4 x err32, 1e-5), err32 the float32 CPU
error of the reference and of the kernels' association in plain torch against float64
(attn_ref.case_reference; test_attn_ref_cpu.py holds it under 1e-5 and asserts that the cases see a
missed rescale, a uniform softmax and a dropped softmax gradient).  Every measured error is
printed."""
import pytest
import torch

import attn_ref as A

pytestmark = pytest.mark.gpu

from few_shot_seg_cwt_amd import synthetic as syn  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda", 0)


def _module(c):
    from few_shot_seg_cwt_amd import MultiHeadAttentionOne
    t = MultiHeadAttentionOne(c["heads"], A.C, A.C, A.C, dropout=0.5)
    t.load_state_dict(c["tsd"])
    t.eval()
    return t


def _inputs(c, dev):
    return c["q"].to(dev), c["f"].to(dev).contiguous(), c["gout"].to(dev).contiguous()


def _grads(t, g):
    return {n: t.view(n, g) for n in A.PARAMS}


def _run(t, q, f, gout, drop=None, grad=None):
    """(out, flat gradient) of the explicit training calls; grad: the buffer to accumulate into."""
    from few_shot_seg_cwt_amd import _lib
    out, saved = t._fwd(q, f, need_saved=True, drop=drop)
    g = torch.zeros_like(t.flat) if grad is None else grad
    t._bwd(q, f, saved, gout, g, drop=drop)
    torch.cuda.synchronize()
    _lib.check_status()
    return out, g


def _compare(c, t, out, g, what):
    errs = A.errors((out, _grads(t, g)), c["ref"], c["heads"])
    for x in (out, g):
        assert bool(torch.isfinite(x).all()), f"{what}: non-finite output"
    print(f"{what} B={c['B']} hw={c['hw']} H={c['heads']} spread {c['spread']:.3g}: errors "
          + " ".join(f"{n}={v:.3g}" for n, v in errs.items())
          + f" | err32 {max(c['err32'].values()):.3g} bar {c['bar']:.3g}")
    assert max(errs.values()) < c["bar"], errs


@pytest.mark.parametrize("name", A.NAMES)
def test_train_path_vs_float64(dev, name):
    c = A.case_reference(name)
    t = _module(c)
    out, g = _run(t, *_inputs(c, dev))
    _compare(c, t, out, g, name)


@pytest.mark.parametrize("pa,po", A.DROPOUT_P)
@pytest.mark.parametrize("name", A.DROPOUT_CASES)
def test_train_path_with_dropout_vs_float64(dev, name, pa, po):
    """The same with both dropouts on, masks regenerated from the seed (tests/dropout_ref.py): with
    a peaked softmax a dropped dominant token changes everything downstream."""
    drop = (pa, po, A.dropout_seed(name, pa, po))
    c = A.case_reference(name, drop)
    t = _module(c)
    out, g = _run(t, *_inputs(c, dev), drop=drop)
    _compare(c, t, out, g, f"{name} p=({pa}, {po})")


@pytest.mark.parametrize("name", ["cap_nv8", "two_chunks"])
def test_backward_accumulates(dev, name):
    """include/cwt.h: the five gradients are ACCUMULATED (+=).  _bwd into a pre-filled buffer is
    pre-fill + the zero-start result, and two backward_into calls give twice one."""
    c = A.case_reference(name)
    t = _module(c)
    q, f, gout = _inputs(c, dev)
    from few_shot_seg_cwt_amd import _lib
    out, saved = t._fwd(q, f, need_saved=True)     # one forward: both backwards read the same saved
    pre = torch.from_numpy(syn.normal(A.SEED, f"attn/{name}/prefill", tuple(t.flat.shape))).to(dev)
    g0, g1 = torch.zeros_like(t.flat), pre.clone()
    t._bwd(q, f, saved, gout, g0)
    t._bwd(q, f, saved, gout, g1)
    torch.cuda.synchronize()
    _lib.check_status()
    for n in A.PARAMS:
        want = t.view(n, pre).double() + t.view(n, g0).double()
        e = A.rel(t.view(n, g1), want)
        print(f"{name} pre-filled {n}: {e:.3g}")
        assert e < 1e-6, n
    out, state = t.forward_train(q, f)
    assert state[3] is None                      # eval mode: no dropout
    t.flat.grad = None
    t.backward_into(state, gout)
    once = t.flat.grad.clone()
    t.backward_into(state, gout)
    torch.cuda.synchronize()
    for n in A.PARAMS:
        e = A.rel(t.view(n, t.flat.grad), 2.0 * t.view(n, once).double())
        print(f"{name} backward_into twice {n}: {e:.3g}")
        assert e < 1e-6, n


def test_autograd_path_batch(dev):
    """t(q, k, k).backward(gout) with k as NCHW [2, 512, 3, 11] (as_tokens makes it token-major)
    fills flat.grad with what the explicit calls give on the same tokens."""
    from few_shot_seg_cwt_amd.transformer import as_tokens
    c = A.make_case("autograd", 2, 33, 4, spread=8.0)
    t = _module(c)
    q, f, gout = _inputs(c, dev)
    k = f.permute(0, 2, 1).reshape(2, A.C, 3, 11).contiguous()           # plain NCHW
    assert k.is_contiguous() and torch.equal(as_tokens(k).permute(0, 2, 3, 1).reshape(2, 33, A.C), f)
    out_e, g = _run(t, q, as_tokens(k), gout)
    t.flat.grad = None
    out = t(q, k, k)
    assert out.requires_grad
    out.backward(gout)
    torch.cuda.synchronize()
    assert A.rel(out, out_e) < 1e-6
    for n in A.PARAMS:
        e = A.rel(t.view(n, t.flat.grad), t.view(n, g))
        print(f"autograd {n}: {e:.3g}")
        assert e < 1e-6, n
    ref = A.reference(c["q"], c["f"], c["tsd"], 4, c["gout"])
    errs = A.errors((out, _grads(t, t.flat.grad)), ref, 4)
    print("autograd against float64:", errs)
    assert max(errs.values()) < A.TOL, errs


@pytest.mark.parametrize("name", A.NAMES)
def test_forward_without_saved_equals_with_saved(dev, name):
    """need_saved only adds the score store, and two forwards agree run to run: the W^T a projection
    (coldot) meets in float64 atomics, so r does not depend on the order its 32 partials arrive in.
    Bound: the 1e-6 of test_dropout_masks_rate_and_modes.  (With r summed by fp32 atomics the
    spread-30 cases differed by up to 1.2e-6 between two forwards of the same inputs.)"""
    c = A.case_reference(name)
    t = _module(c)
    q, f, _ = _inputs(c, dev)
    a, _ = t._fwd(q, f, need_saved=True)
    b, saved = t._fwd(q, f, need_saved=False)
    torch.cuda.synchronize()
    assert saved is None
    e = A.rel(b, a)
    print(f"{name}: without saved against with saved {e:.3g}")
    assert e < 1e-6


def test_argument_errors(dev):
    """B = 5 (nv = 10 > coldot's 8 vectors) and heads = 3 are refused by the argument checks, before
    any launch; the context's status word stays clean and the next call works."""
    from few_shot_seg_cwt_amd import MultiHeadAttentionOne, _lib
    with pytest.raises(NotImplementedError):
        MultiHeadAttentionOne(3, A.C, A.C, A.C)
    c = A.case_reference("one_wave")
    t = _module(c)
    q, f, gout = _inputs(c, dev)
    out, g = _run(t, q, f, gout)
    q5, f5 = q[:1].repeat(5, 1, 1).contiguous(), f[:1].repeat(5, 1, 1).contiguous()
    with pytest.raises(_lib.CwtError, match="B <= 4"):
        t._fwd(q5, f5, need_saved=True)
    with pytest.raises(_lib.CwtError, match="B <= 4"):
        t._bwd(q5, f5, torch.zeros(16, device=dev), q5.clone(), torch.zeros_like(t.flat))
    t.n_head = 3                                    # past the constructor: the library's own check
    try:
        with pytest.raises(_lib.CwtError, match="heads must be 1, 2 or 4"):
            t._fwd(q, f, need_saved=False)
    finally:
        t.n_head = c["heads"]
    torch.cuda.synchronize()
    _lib.check_status()
    out2, g2 = _run(t, q, f, gout)
    assert A.rel(out2, out) < 1e-6 and A.rel(g2, g) < 1e-6
