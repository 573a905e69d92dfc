"""FuseNet1 and the fusion trainer's device ops: the build's counterparts of the reference's
``FuseNet1`` (src/model/transformer.py:286-330) and of the per-episode arithmetic of
src/train_fuse.py:173-186 (support mask, blend, disagreement-weighted loss).

``FuseNet1(im_size, mid_dim)`` keeps the reference's constructor, ``forward(corr_lst, s_mask,
pd_lst) -> wt [B, 2, h, w]`` and state_dict keys (``conv4d.{0,2}.conv{1,2}.{weight,bias}``,
``att.{0,2}.{weight,bias}``).  The forward runs

  cwt_fuse_stack          each correlation through the strided 4-D stack, written straight into its
                          column range of the token matrix X [h w][ldx] (no reshape / permute / cat)
  cwt_fuse_mask_bias      the broadcast support mask's m^2 channels folded into att.0's bias
  cwt_linear (x2)         att.0 + ReLU, att.2 over X (exact fp32 MFMA)
  cwt_fuse_softmax2       the softmax over the two logits

and the backward the same chain reversed (cwt_fuse_softmax2_backward, cwt_linear_backward,
cwt_fuse_mask_bias_backward, cwt_fuse_stack_backward once per correlation, the second accumulating).
Only FuseNet1's parameters receive a gradient: the correlations, the mask and the predictions come
out of ``no_grad`` in the trainer, and the kernels carry none to them.

X's columns: [0, m^2) y2(corr_lst[0]), [m^2, 2 m^2) y2(corr_lst[1]), then pd_lst[0]'s and pd_lst[1]'s
two channels, then zero columns up to a multiple of 4 (cwt_linear's K); att.0's weight is repacked
to those columns on every call and the zero columns' gradients are dropped.

Declared differences: one episode per call (B = 1: the mask's fold into the bias is per image, and
the reference trainer's batch is 1); exactly two correlations and two predictions, as the trainer
passes them.
"""
from __future__ import annotations

import torch

from . import _lib

_CONV_NAMES = ("conv4d.0.conv1.weight", "conv4d.0.conv1.bias", "conv4d.0.conv2.weight", "conv4d.0.conv2.bias",
               "conv4d.2.conv1.weight", "conv4d.2.conv1.bias", "conv4d.2.conv2.weight", "conv4d.2.conv2.bias")
_ATT_NAMES = ("att.0.weight", "att.0.bias", "att.2.weight", "att.2.bias")
PARAM_NAMES = _CONV_NAMES + _ATT_NAMES


def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    return _lib.require(t, name).contiguous()


def _tokens(f: torch.Tensor) -> torch.Tensor:
    """[B, C, h, w] (any memory format) -> the same tensor with NHWC storage ([B, hw, C] tokens)"""
    return f.contiguous(memory_format=torch.channels_last)


def stack_saved_floats(B, hA, wA, hB, wB) -> int:
    return int(_lib.lib().cwt_fuse_stack_saved_floats(B, hA, wA, hB, wB))


def fuse_stack(corr: torch.Tensor, params, X: torch.Tensor, col: int, save: bool = False):
    """corr [B, hA, wA, hB, wB] through the 4-D stack into X[..., col : col + mB nB] (X [B hA wA, ldx]);
    params: the eight tensors of ``_CONV_NAMES``.  save: also return layer 1's output
    [B, hA wA, mB nB, 16] (after its ReLU) for fuse_stack_backward."""
    corr = _f32(corr, "corr")
    B, hA, wA, hB, wB = corr.shape
    ps = [_f32(p.detach(), n) for p, n in zip(params, _CONV_NAMES)]
    _lib.require(X, "X")
    if X.dim() != 2 or not X.is_contiguous() or X.shape[0] != B * hA * wA:
        raise ValueError("X must be a contiguous [B hA wA, ldx] matrix")
    y1 = None
    if save:
        y1 = torch.empty((B, hA * wA, ((hB + 1) // 2) * ((wB + 1) // 2), 16), device=corr.device, dtype=torch.float32)
    _lib.check(_lib.lib().cwt_fuse_stack(_lib.ctx(corr.device.index), _lib.ptr(corr), B, hA, wA, hB, wB,
                                         *[_lib.ptr(p) for p in ps], _lib.ptr(y1), _lib.ptr(X), X.shape[1], int(col),
                                         _lib.stream_ptr(corr.device)), "cwt_fuse_stack")
    return y1


def fuse_stack_backward(corr, params, y1, X, dX, col: int, grads, accumulate: bool):
    """The eight parameter gradients of <dX, y2> into ``grads`` (tensors shaped like ``params``)."""
    corr = _f32(corr, "corr")
    B, hA, wA, hB, wB = corr.shape
    w2a, w2b = _f32(params[4].detach(), "w2a"), _f32(params[6].detach(), "w2b")
    dX = _f32(dX, "dX")
    if dX.shape != X.shape:
        raise ValueError("dX must have X's shape")
    _lib.check(_lib.lib().cwt_fuse_stack_backward(
        _lib.ctx(corr.device.index), _lib.ptr(corr), B, hA, wA, hB, wB, _lib.ptr(w2a), _lib.ptr(w2b), _lib.ptr(y1),
        _lib.ptr(X), _lib.ptr(dX), X.shape[1], int(col), int(accumulate), *[_lib.ptr(g) for g in grads],
        _lib.stream_ptr(corr.device)), "cwt_fuse_stack_backward")
    return grads


def support_mask(s_label: torch.Tensor, m: int, align_corners: bool, pool: bool = False) -> torch.Tensor:
    """s_label [H, W] (or [1, H, W]) int64 -> [1, 1, m, m]: 255 -> 0, the bilinear resize
    (train_fuse.py:173-175 trains with align_corners=True, :319-321 validates with False); pool: the
    resize goes to [2m, 2m] and AvgPool2d(2, 2) follows."""
    lbl = _lib.require(s_label, "s_label", torch.int64).contiguous()
    if lbl.dim() == 3:
        if lbl.shape[0] != 1:
            raise ValueError("the fusion trainer is one-shot: s_label must hold one support label")
        lbl = lbl[0]
    H, W = lbl.shape
    out = torch.empty((1, 1, m, m), device=lbl.device, dtype=torch.float32)
    _lib.check(_lib.lib().cwt_fuse_support_mask(_lib.ctx(lbl.device.index), _lib.ptr(lbl), H, W, int(m),
                                                int(bool(align_corners)), int(bool(pool)), _lib.ptr(out),
                                                _lib.stream_ptr(lbl.device)), "cwt_fuse_support_mask")
    return out


def _linear(x, w, b, relu):
    from .detr import linear
    return linear(x, w, b, relu)


def _linear_backward(x, w, out, d, want_dx: bool):
    N, K = w.shape
    P = x.shape[0]
    f = dict(device=x.device, dtype=torch.float32)
    dx = torch.empty_like(x) if want_dx else None
    dw, db = torch.empty((N, K), **f), torch.empty(N, **f)
    _lib.check(_lib.lib().cwt_linear_backward(_lib.ctx(x.device.index), _lib.ptr(x), P, K, _lib.ptr(w), N,
                                              _lib.ptr(out), _lib.ptr(d), _lib.ptr(dx), _lib.ptr(dw), K, _lib.ptr(db),
                                              _lib.stream_ptr(x.device)), "cwt_linear_backward")
    return dx, dw, db


def pack_att0(W, n, ldx):
    """att.0.weight [mid, 3n + 4(, 1, 1)] -> [mid, ldx] in X's column order: the two stacks' 2n columns, the
    predictions' four, zeros up to ldx (the mask's n columns go into the bias, cwt_fuse_mask_bias)"""
    Wf = W.detach().reshape(W.shape[0], -1)
    Wx = torch.zeros((W.shape[0], ldx), device=W.device, dtype=torch.float32)
    Wx[:, :2 * n] = Wf[:, :2 * n]
    Wx[:, 2 * n:2 * n + 4] = Wf[:, 3 * n:]
    return Wx


def att_forward(X, n, att_params, sm, pd0, pd1, Wx=None):
    """FuseNet1.att and the softmax over X [P, ldx] whose first 2n columns hold the two stacks' outputs:
    writes the predictions' four columns and the zero padding, folds the mask sm [n] into att.0's bias.
    Wx: pack_att0's matrix when the caller keeps one (FuseNet1 does, per parameter version).
    -> (wt [1, 2, P] planes, what att_backward needs)"""
    W, b, W2, b2 = att_params
    dev = X.device
    L, st, cx = _lib.lib(), _lib.stream_ptr(dev), _lib.ctx(dev.index)
    P, ldx = X.shape
    mid, K = W.shape[0], 2 * n + 4
    X[:, 2 * n:2 * n + 2] = pd0.reshape(2, P).t()
    X[:, 2 * n + 2:K] = pd1.reshape(2, P).t()
    if ldx > K:
        X[:, K:] = 0
    Wf = W.reshape(mid, -1).contiguous()                  # [mid, 3 m^2 + 4]
    if Wx is None:
        Wx = pack_att0(W, n, ldx)
    sm = _f32(sm, "s_mask")
    b_eff = torch.empty(mid, device=dev, dtype=torch.float32)
    _lib.check(L.cwt_fuse_mask_bias(cx, _lib.ptr(Wf), Wf.shape[1], 2 * n, _lib.ptr(sm), n, _lib.ptr(b.contiguous()),
                                    mid, _lib.ptr(b_eff), st), "cwt_fuse_mask_bias")
    hid = _linear(X, Wx, b_eff, True)
    W2f = W2.reshape(2, mid).contiguous()
    z = _linear(hid, W2f, b2, False)
    wt = torch.empty((1, 2, P), device=dev, dtype=torch.float32)
    _lib.check(L.cwt_fuse_softmax2(cx, _lib.ptr(z), 1, P, _lib.ptr(wt), st), "cwt_fuse_softmax2")
    return wt, (X, sm, Wx, hid, W2f, wt, z)


def att_backward(saved, d_wt):
    """-> (dX [P, ldx], d att.0.weight [mid, 3n + 4], d att.0.bias, d att.2.weight [2, mid], d att.2.bias)"""
    X, sm, Wx, hid, W2f, wt, _ = saved
    dev = X.device
    L, st, cx = _lib.lib(), _lib.stream_ptr(dev), _lib.ctx(dev.index)
    P, mid, n = X.shape[0], Wx.shape[0], sm.numel()
    K = 2 * n + 4
    d_wt = d_wt.contiguous()
    d_z = torch.empty((P, 2), device=dev, dtype=torch.float32)
    _lib.check(L.cwt_fuse_softmax2_backward(cx, _lib.ptr(wt), _lib.ptr(d_wt), 1, P, _lib.ptr(d_z), st),
               "cwt_fuse_softmax2_backward")
    d_hid, dW2, db2 = _linear_backward(hid, W2f, None, d_z, True)
    dX, dWx, db = _linear_backward(X, Wx, hid, d_hid, True)
    dW = torch.empty((mid, 3 * n + 4), device=dev, dtype=torch.float32)
    dW[:, :2 * n] = dWx[:, :2 * n]
    dW[:, 3 * n:] = dWx[:, 2 * n:K]   # the zero columns past K carry no parameter
    _lib.check(L.cwt_fuse_mask_bias_backward(cx, _lib.ptr(db), _lib.ptr(sm), mid, n, _lib.ptr(dW), dW.shape[1],
                                             2 * n, st), "cwt_fuse_mask_bias_backward")
    return dX, dW, db, dW2, db2


class _FuseNet1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, corr_l, corr_h, s_mask, pd0, pd1, opts, *params):
        conv, att = params[:8], [p.detach() for p in params[8:]]
        B, hA, wA, hB, wB = corr_l.shape
        n = s_mask.numel()
        ldx = (2 * n + 4 + 3) // 4 * 4
        train = any(ctx.needs_input_grad[6:])   # forward runs with grad mode off: ask the context
        X = torch.empty((hA * wA, ldx), device=corr_l.device, dtype=torch.float32)
        record, save = opts.get("record"), train or bool(opts.get("two_pass"))
        y1l = fuse_stack(corr_l, conv, X, 0, save=save)
        y1h = fuse_stack(corr_h, conv, X, n, save=save)
        wt, saved = att_forward(X, n, att, s_mask.reshape(-1), pd0, pd1, opts.get("Wx"))
        if record is not None:   # the ReLU gates of this forward, for the gradient tests: y1 > 0, X > 0, hid > 0
            record.update(X=X, y1=(y1l, y1h), hid=saved[3], z=saved[6])
        if train:
            ctx.save_for_backward(corr_l, corr_h, y1l, y1h, *saved, *conv)
            ctx.shapes = [p.shape for p in params]
        return wt.reshape(1, 2, hA, wA)

    @staticmethod
    def backward(ctx, d_wt):
        corr_l, corr_h, y1l, y1h, *rest = ctx.saved_tensors
        saved, conv = rest[:7], rest[7:]
        shapes = ctx.shapes
        X, n = saved[0], saved[1].numel()
        dX, dW, db, dW2, db2 = att_backward(saved, d_wt)
        grads = [torch.empty(s, device=X.device, dtype=torch.float32) for s in shapes[:8]]
        fuse_stack_backward(corr_l, conv, y1l, X, dX, 0, grads, False)
        fuse_stack_backward(corr_h, conv, y1h, X, dX, n, grads, True)
        return (None,) * 6 + tuple(grads) + (dW.reshape(shapes[8]), db, dW2.reshape(shapes[10]), db2)


class _CenterPivot(torch.nn.Module):
    """The parameters of a CenterPivotConv4d (conv4d.py:16-19): conv1 over the query plane, conv2 over
    the support plane.  Holder only: the arithmetic is cwt_fuse_stack's."""

    def __init__(self, cin: int, cout: int):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(cin, cout, 3, padding=1)
        self.conv2 = torch.nn.Conv2d(cin, cout, 3, padding=1)


class FuseNet1(torch.nn.Module):
    """transformer.py:286-330.  Parameters are drawn by nn.Conv2d's default init from the host RNG in the
    reference's order, then moved to ``device`` ("cpu" builds a holder for checkpoint work; the forward
    needs a GPU and raises without one)."""

    def __init__(self, im_size: int = 30, mid_dim: int = 256, device=None):
        super().__init__()
        if mid_dim % 4:
            raise ValueError("mid_dim must be a multiple of 4 (cwt_linear's K)")
        self.im_size, self.mid_dim = int(im_size), int(mid_dim)
        self.record = None   # a dict here receives each forward's X, y1, hid, z (the ReLU gates; test hook)
        # How a forward that trains nothing runs the 4-D stack: "fused" recomputes layer 1 on each output's halo
        # and stores nothing (no 16-channel buffer, 207 MB per correlation at 473^2); "two_pass" stores it for
        # the call, as training does -- the same bits, about 4x faster at 473^2 (the fusion trainer)
        self.eval_form = "fused"
        self._att0 = None    # (version of att.0.weight, its storage, ldx, the repacked matrix)
        self.conv4d = torch.nn.Sequential(_CenterPivot(1, 16), torch.nn.ReLU(inplace=True), _CenterPivot(16, 1),
                                          torch.nn.ReLU(inplace=True))
        self.pool = torch.nn.AvgPool2d(kernel_size=2, stride=2)
        in_dim = self.im_size * self.im_size * 3 + 4
        self.att = torch.nn.Sequential(torch.nn.Conv2d(in_dim, mid_dim, kernel_size=1, padding=0), torch.nn.ReLU(),
                                       torch.nn.Conv2d(mid_dim, 2, kernel_size=1, padding=0))
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu"
        self.to(device)

    def _packed_att0(self, n: int, ldx: int):
        """pack_att0(att.0.weight), kept until the parameter changes (an optimiser step, load_state_dict and
        .to() all move its version or its storage)"""
        W = self.att[0].weight
        key = (W._version, W.data_ptr(), ldx)
        if self._att0 is None or self._att0[0] != key:
            self._att0 = (key, pack_att0(W, n, ldx))
        return self._att0[1]

    def _params(self):
        sd = dict(self.named_parameters())
        return [sd[n] for n in PARAM_NAMES]

    def forward(self, corr_lst, s_mask, pd_lst):
        if len(corr_lst) != 2 or len(pd_lst) != 2:
            raise ValueError("FuseNet1 takes two correlations and two predictions (train_fuse.py:177)")
        corr_l, corr_h = corr_lst
        B, hA, wA, hB, wB = corr_l.shape
        if B != 1:
            raise ValueError("FuseNet1 runs one episode per call (B = 1)")
        m = self.im_size
        if ((hB + 1) // 2, (wB + 1) // 2) != (m, m) or corr_h.shape != corr_l.shape:
            raise ValueError(f"correlations must be [1, h, w, hs, ws] with ceil(hs/2) = ceil(ws/2) = im_size = {m}")
        if s_mask.shape[-1] == 2 * m:
            s_mask = self.pool(s_mask)
        if s_mask.numel() != m * m:
            raise ValueError(f"s_mask must be [1, 1, {m}, {m}] or [1, 1, {2 * m}, {2 * m}]")
        pd0, pd1 = (_f32(p.detach(), "pd") for p in pd_lst)
        if pd0.shape != (1, 2, hA, wA) or pd1.shape != pd0.shape:
            raise ValueError("pd_lst must hold two [1, 2, h, w] predictions")
        if self.eval_form not in ("fused", "two_pass"):
            raise ValueError(f"eval_form {self.eval_form!r}: 'fused' or 'two_pass'")
        n = m * m
        opts = dict(record=self.record, two_pass=self.eval_form == "two_pass",
                    Wx=self._packed_att0(n, (2 * n + 4 + 3) // 4 * 4))
        return _FuseNet1Fn.apply(corr_l.detach(), corr_h.detach(), s_mask.detach(), pd0, pd1, opts,
                                 *self._params())


class _FuseBlendFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, wv, fq, wt):
        B, C, h, w = wv.shape
        out = torch.empty_like(wv)   # channels_last, as wv
        _lib.check(_lib.lib().cwt_fuse_blend(_lib.ctx(wv.device.index), _lib.ptr(wv), _lib.ptr(fq), _lib.ptr(wt), B,
                                             h * w, C, _lib.ptr(out), _lib.stream_ptr(wv.device)), "cwt_fuse_blend")
        ctx.save_for_backward(wv, fq)
        return out

    @staticmethod
    def backward(ctx, d_out):
        wv, fq = ctx.saved_tensors
        B, C, h, w = wv.shape
        d_out = _tokens(d_out)
        d_wt = torch.empty((B, 2, h, w), device=wv.device, dtype=torch.float32)
        _lib.check(_lib.lib().cwt_fuse_blend_backward(_lib.ctx(wv.device.index), _lib.ptr(wv), _lib.ptr(fq),
                                                      _lib.ptr(d_out), B, h * w, C, _lib.ptr(d_wt),
                                                      _lib.stream_ptr(wv.device)), "cwt_fuse_blend_backward")
        return None, None, d_wt


def fuse_blend(weighted_v: torch.Tensor, f_q: torch.Tensor, wt: torch.Tensor) -> torch.Tensor:
    """out = weighted_v * wt[:, 0:1] + f_q * wt[:, 1:2] (train_fuse.py:178) on NHWC tokens; [B, C, h, w]
    channels_last.  Differentiable in wt only: weighted_v and f_q come out of no_grad."""
    wv, fq = _tokens(_lib.require(weighted_v.detach(), "weighted_v")), _tokens(_lib.require(f_q.detach(), "f_q"))
    if wv.shape != fq.shape or wt.shape != (wv.shape[0], 2) + wv.shape[2:]:
        raise ValueError("fuse_blend: weighted_v, f_q [B, C, h, w] and wt [B, 2, h, w]")
    return _FuseBlendFn.apply(wv, fq, _lib.require(wt, "wt").contiguous())


class _FuseLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pd_q, pd_q0, pd_q1, label):
        _, _, h, w = pd_q.shape
        S = label.shape[-1]
        dev = pd_q.device
        f = dict(device=dev, dtype=torch.float32)
        loss, iut, dis = torch.empty(1, **f), torch.empty((3, 3, 2), **f), torch.empty(1, **f)
        d = torch.empty_like(pd_q) if pd_q.requires_grad or ctx.needs_input_grad[0] else None
        _lib.check(_lib.lib().cwt_fuse_loss_head(_lib.ctx(dev.index), _lib.ptr(pd_q), _lib.ptr(pd_q0), _lib.ptr(pd_q1),
                                                 h, w, _lib.ptr(label), S, _lib.ptr(loss), _lib.ptr(d), _lib.ptr(iut),
                                                 _lib.ptr(dis), _lib.stream_ptr(dev)), "cwt_fuse_loss_head")
        ctx.d = d
        ctx.mark_non_differentiable(iut, dis)
        return loss.reshape(()), iut, dis

    @staticmethod
    def backward(ctx, g, _gi, _gd):
        return ctx.d * g, None, None, None


def fuse_loss_head(pd_q: torch.Tensor, pd_q0: torch.Tensor, pd_q1: torch.Tensor, q_label: torch.Tensor):
    """train_fuse.py:180-186, :195-205 on the low-resolution logits [1, 2, h, w] and q_label [1, S, S]
    (or [S, S]) int64: -> (loss, iut [3, 3, 2] = {intersection, union, target} x class of pred_q,
    pred_q0, pred_q1, the number of disagreeing pixels [1]).  The loss is differentiable in pd_q."""
    lbl = _lib.require(q_label, "q_label", torch.int64).contiguous()
    if lbl.dim() == 3 and lbl.shape[0] != 1 or lbl.shape[-1] != lbl.shape[-2]:
        raise ValueError("q_label must be one square label")
    ps = [_lib.require(p, n) for p, n in ((pd_q, "pd_q"), (pd_q0, "pd_q0"), (pd_q1, "pd_q1"))]
    if any(p.shape != ps[0].shape for p in ps) or ps[0].dim() != 4 or ps[0].shape[:2] != (1, 2):
        raise ValueError("pd_q, pd_q0, pd_q1 must be [1, 2, h, w]")
    return _FuseLossFn.apply(ps[0].contiguous(), ps[1].detach().contiguous(), ps[2].detach().contiguous(), lbl)
