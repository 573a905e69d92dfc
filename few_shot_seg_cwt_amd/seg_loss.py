"""The MMN / DeTr trainers' loss head on the device (cwt_seg_head_loss, csrc/seg_loss.hip):
``criterion(F.interpolate(model.classifier(f), size=label, mode='bilinear', align_corners=True),
label)`` of src/train_kshot.py:168-183 with ``criterion = SegLoss(loss_type)``
(src/model/model_util.py:9-73) and the classifier of src/model/pspnet.py:183-187, as one call
that also forms d loss / d f.  The S x S logits are never stored.

``seg_head_loss_nway`` (cwt_seg_head_loss_nway, csrc/seg_loss_nway.hip) is the class-incremental
trainer's head (src/train_cca.py:177-198): an N-way classifier, ``compress_pred(., idx_cls, 'lg')``
and ``SegLoss(loss_type)(., label, 'pb')``.  Both go through one autograd Function and one
validator; the 2-way head is the case with no idx_cls and no iut."""
from __future__ import annotations

import torch

from . import _lib
from .transformer import as_tokens

WT_CE, WT_DC, CE = 0, 1, 2


def loss_type_id(loss_type) -> int:
    """SegLoss.forward's dispatch (model_util.py:16-24): 'wt_dc' / 'dc' -> dice, 'ce' -> the
    unweighted CE, anything else -> the class-weighted CE."""
    if isinstance(loss_type, int):
        if loss_type not in (WT_CE, WT_DC, CE):
            raise ValueError(f"loss_type id must be 0, 1 or 2, got {loss_type}")
        return loss_type
    if loss_type in ("wt_dc", "dc"):
        return WT_DC
    if loss_type == "ce":
        return CE
    return WT_CE


def _call(W, ft, target, idx_cls, lt, want_logits, want_grad, want_iut):
    """idx_cls None: cwt_seg_head_loss on W [2, C]; else cwt_seg_head_loss_nway on W [N, C]."""
    B, C, h, w = ft.shape
    N = W.shape[0]
    S = target.shape[-1]
    dev = ft.device
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    logits = torch.empty((B, N, h, w), device=dev, dtype=torch.float32) if want_logits else None
    d_f = torch.empty_like(ft) if want_grad else None   # channels_last, as ft
    iut = torch.empty((B, 3, 2), device=dev, dtype=torch.float32) if want_iut else None
    if idx_cls is None:
        _lib.check(_lib.lib().cwt_seg_head_loss(
            _lib.ctx(dev.index), _lib.ptr(W), _lib.ptr(ft), B, h, w, C, _lib.ptr(target), S, lt, _lib.ptr(loss),
            _lib.ptr(logits), _lib.ptr(d_f), _lib.stream_ptr(dev)), "cwt_seg_head_loss")
    else:
        _lib.check(_lib.lib().cwt_seg_head_loss_nway(
            _lib.ctx(dev.index), _lib.ptr(W), _lib.ptr(ft), B, h, w, C, N, _lib.ptr(target), S, int(idx_cls), lt,
            _lib.ptr(loss), _lib.ptr(logits), _lib.ptr(d_f), _lib.ptr(iut), _lib.stream_ptr(dev)),
            "cwt_seg_head_loss_nway")
    return loss, logits, d_f, iut


class _SegHeadLossFn(torch.autograd.Function):
    """The loss and d loss / d f come out of the same call; backward scales the kept gradient."""

    @staticmethod
    def forward(ctx, ft, W, target, idx_cls, lt, want_logits, want_iut):
        loss, logits, d_f, iut = _call(W, ft, target, idx_cls, lt, want_logits, True, want_iut)
        ctx.save_for_backward(d_f)
        if logits is None:
            logits = torch.empty(0, device=ft.device)
        if iut is None:
            iut = torch.empty(0, device=ft.device)
        ctx.mark_non_differentiable(logits, iut)
        return loss.reshape(()), logits, iut

    @staticmethod
    def backward(ctx, g, _g_logits, _g_iut):
        (d_f,) = ctx.saved_tensors
        return d_f * g, None, None, None, None, None, None


def _head(W, f, target, idx_cls, loss_type, return_logits, return_iut):
    """The arguments checked, then the loss (and logits, iut) with autograd to f where f asks for it."""
    _lib.require(f, "f")
    _lib.require(W, "W")
    _lib.require(target, "target", torch.int64)
    if f.dim() != 4 or target.dim() != 3 or target.shape[0] != f.shape[0] or target.shape[1] != target.shape[2]:
        raise ValueError(f"f must be [B,C,h,w] and target [B,S,S], got {tuple(f.shape)} and {tuple(target.shape)}")
    C = f.shape[1]
    if idx_cls is None:
        if W.numel() != 2 * C:
            raise ValueError(f"W must hold 2 x {C} weights, got {tuple(W.shape)}")
        N = 2
    else:
        if W.dim() < 2 or W.numel() != W.shape[0] * C:
            raise ValueError(f"W must be [N, {C}], got {tuple(W.shape)}")
        N, idx_cls = W.shape[0], int(idx_cls)
    W = W.detach().reshape(N, C).contiguous()
    target = target.contiguous()
    lt = loss_type_id(loss_type)
    ft = as_tokens(f)
    if torch.is_grad_enabled() and f.requires_grad:
        loss, logits, iut = _SegHeadLossFn.apply(ft, W, target, idx_cls, lt, bool(return_logits), bool(return_iut))
    else:
        loss, logits, _, iut = _call(W, ft.detach(), target, idx_cls, lt, return_logits, False, return_iut)
        loss = loss.reshape(())
    out = (loss,) + ((logits,) if return_logits else ()) + ((iut,) if return_iut else ())
    return out if len(out) > 1 else loss


def seg_head_loss(W: torch.Tensor, f: torch.Tensor, target: torch.Tensor, loss_type="wt_dc",
                  return_logits: bool = False):
    """W [2, C] (or [1, 2, C] / [2, C, 1, 1]: the binary classifier's weight, a constant), f
    [B, C, h, w] features, target int64 [B, S, S] (255 = ignore) -> the scalar loss, with autograd
    to f; with return_logits also the low-resolution logits [B, 2, h, w] (for the IoU logging)."""
    return _head(W, f, target, None, loss_type, return_logits, False)


def seg_head_loss_nway(W: torch.Tensor, f: torch.Tensor, target: torch.Tensor, idx_cls: int, loss_type="wt_dc",
                       return_logits: bool = False, return_iut: bool = False):
    """train_cca.py:177-198 (cwt_seg_head_loss_nway, csrc/seg_loss_nway.hip): W [N, C] (or
    [N, C, 1, 1]: the N-way classifier's weight, a constant), f [B, C, h, w], target int64 [B, S, S]
    in {0, 1, 255} -> SegLoss(loss_type)(compress_pred(upsample(W . f), idx_cls, 'lg'), target, 'pb'),
    a scalar with autograd to f.  With return_logits also the low-resolution logits [B, N, h, w]
    (classify_nway's, bit for bit); with return_iut also the [B, 3, 2] intersection / union /
    target counts of the mask p > 0.5 (the training meters' pred.argmax(1), train_cca.py:211-213).
    The CE forms take the probabilities as logits, as the reference's SegLoss does."""
    return _head(W, f, target, int(idx_cls), loss_type, return_logits, return_iut)


compress_pred_loss = seg_head_loss_nway   # by the reference's name for the compression


class SegLoss(torch.nn.Module):
    """model_util.py:9-24 by name ('wt_dc', 'dc', 'ce', anything else -> 'wt_ce'), applied to
    features through the classifier weight: ``SegLoss(t)(W, f, target)``."""

    def __init__(self, loss_type: str = "wt_ce", num_cls: int = 2, fg_idx: int = 1):
        super().__init__()
        if num_cls != 2 or fg_idx != 1:
            raise NotImplementedError("SegLoss: 2-way episodes with foreground index 1 only")
        self.loss_type = loss_type

    def forward(self, W, f, target, return_logits: bool = False):
        return seg_head_loss(W, f, target, self.loss_type, return_logits)
