"""Float64 restatements for the loss-head and WeightAverage-dropout tests, written from the
reference's formulas and differentiated by torch autograd (no project code):

* head_loss: the classifier (src/model/pspnet.py:183-187, a bias-free 1x1 conv), the bilinear
  align_corners=True upsample to the label size (src/train_kshot.py:168-183) and SegLoss
  (src/model/model_util.py:9-73: weighted_dice_loss, weighted_ce_loss, CrossEntropyLoss(ignore 255)).
* weight_average_drop: WeightAverage (src/model/msm/msm_func.py:50-104) with its two dropouts
  given as explicit masks (att_drop on the softmax weights, :90; proj_drop on conv_back's output
  before the residual, :100), the masks drawn by tests/dropout_ref.py.
"""
import numpy as np
import torch
import torch.nn.functional as F

from dropout_ref import dropout_scale

WA_ATT_STREAM, WA_PROJ_STREAM = 6, 7   # csrc/common.h


def head_logits(W, f):
    """W [2, C], f [B, C, h, w] -> [B, 2, h, w]."""
    return torch.einsum("kc,bchw->bkhw", W, f)


def seg_loss(z, target, loss_type):
    """SegLoss.forward on the upsampled logits z [B, 2, S, S] and the int64 target [B, S, S]."""
    if loss_type in ("wt_dc", "dc"):   # weighted_dice_loss, reduction 'sum', eps 1e-8
        B = z.shape[0]
        t = torch.stack([target == 0, target == 1], dim=1).to(z.dtype)
        p = torch.sigmoid(z).reshape(2 * B, -1)
        t = t.reshape(2 * B, -1)
        part = (p ** 2).sum(-1) + (t ** 2).sum(-1)
        loss = 1 - 2 * (t * p).sum(-1) / torch.clamp(part, min=1e-8)
        return loss.sum() / B
    if loss_type == "ce":
        return F.cross_entropy(z, target, ignore_index=255)
    fg = (target == 1).sum()
    bg = ((target != 1) & (target != 255)).sum()
    weight = torch.ones(2, dtype=z.dtype)
    weight[1] = bg.to(z.dtype) / fg.to(z.dtype)
    return F.cross_entropy(z, target, weight=weight, ignore_index=255)


def head_loss(W, f, target, loss_type):
    """-> (loss, low-resolution logits)."""
    lg = head_logits(W, f)
    z = F.interpolate(lg, size=target.shape[-2:], mode="bilinear", align_corners=True)
    return seg_loss(z, target, loss_type), lg


def wa_masks(N, C, h, w, p_att, p_proj, seed):
    """(att mask [N, 9, h, w], proj mask [N, C, h, w]) float64, indexed as the kernels draw them:
    att ((n h + y) w + x) 9 + r, proj the NHWC linear index."""
    ia = np.arange(N * h * w * 9, dtype=np.uint64)
    ma = dropout_scale(p_att, seed, WA_ATT_STREAM, ia).reshape(N, h, w, 9) if p_att > 0 else np.ones((N, h, w, 9))
    ip = np.arange(N * h * w * C, dtype=np.uint64)
    mp = dropout_scale(p_proj, seed, WA_PROJ_STREAM, ip).reshape(N, h, w, C) if p_proj > 0 else np.ones((N, h, w, C))
    return (torch.from_numpy(np.ascontiguousarray(ma)).double().permute(0, 3, 1, 2),
            torch.from_numpy(np.ascontiguousarray(mp)).double().permute(0, 3, 1, 2))


def weight_average_drop(x, p, att_mask, proj_mask):
    """msm_func.py:66-104, R = 3; p = (w_theta, b_theta, w_phi, b_phi, w_g, b_g, w_back, b_back)."""
    wt, bt, wp, bp, wg, bg, wb, bb = p
    B, C, h, w = x.shape
    xp = F.pad(x, (1, 1, 1, 1), mode="replicate")
    theta = F.conv2d(x, wt, bt)
    cos, gs = [], []
    for dy in range(3):
        for dx in range(3):
            nb = xp[:, :, dy:dy + h, dx:dx + w]
            cos.append(F.cosine_similarity(F.conv2d(nb, wp, bp), theta, dim=1))
            gs.append(F.conv2d(nb, wg, bg))
    sm = torch.softmax(torch.stack(cos, 1), dim=1) * att_mask
    wavg = sum(sm[:, r:r + 1] * gs[r] for r in range(9))
    return x + F.conv2d(wavg, wb, bb) * proj_mask
