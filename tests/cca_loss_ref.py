"""Float64 restatement of the class-incremental trainer's loss head (src/train_cca.py:177-198) and of
pred_q2 (train_cca.py:347, 353), written from the reference's formulas and differentiated by torch
autograd -- a helper, nothing from few_shot_seg_cwt_amd:

* head_loss: the N-way classifier (a bias-free 1x1 conv), the bilinear align_corners=True upsample
  to the label size, compress_pred(., idx_cls, 'lg') (src/model/model_util.py:158-166; F.softmax
  without dim on a 4-D tensor is dim = 1) and SegLoss(loss_type)(., label, 'pb')
  (model_util.py:9-73).  The CE forms take the two-channel PROBABILITIES as logits: SegLoss.forward
  ignores input_type on those branches.
* iut_half: intersection / union / target of pred.argmax(1) of the compressed prediction
  (train_cca.py:211-213) -- the mask p > 0.5, a tie to class 0.
* mix_mask: pred2bmask of softmax(z0) (1 - att_wt) + softmax(z1) att_wt.
* the draws of the GPU tests, redrawn until no hi-res pixel sits within GAP of a decision edge.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

GAP = 1e-4
LOSS_TYPES = ["wt_ce", "wt_dc", "ce"]
# (B, N, idx_cls, C, h, S)
CASES = [(1, 17, 16, 512, 5, 33),
         (2, 16, 3, 64, 7, 49),     # B > 1, idx_cls in the middle
         (1, 2, 1, 512, 6, 50),     # S - 1 is not a multiple of h - 1
         (1, 64, 63, 512, 6, 50),   # the class limit
         (1, 33, 0, 512, 9, 65)]    # idx_cls = 0, one class past a 32-class tile
SCALES = [1.0, 8.0, 30.0]
# (B, N, h, S) of the pred_q2 tests
MIX_CASES = [(1, 17, 5, 33), (2, 3, 7, 49), (1, 64, 6, 50)]
MIX_WTS = [0.2, 0.5]


def upsample(lg, S):
    return F.interpolate(lg, size=(S, S), mode="bilinear", align_corners=True)


def head_logits(W, f):
    """W [N, C], f [B, C, h, w] -> [B, N, h, w]."""
    return torch.einsum("kc,bchw->bkhw", W, f)


def compress_pred(z, idx_cls):
    """model_util.py:158-166 with input_type 'lg'."""
    p = torch.softmax(z, dim=1)[:, idx_cls]
    return torch.stack([1.0 - p, p], dim=1)


def weighted_dice_loss(q, target, eps=1e-8):
    """model_util.py:40-73 with input_type 'pb' (no sigmoid), reduction 'sum'."""
    B = q.shape[0]
    t = torch.stack([target == 0, target == 1], dim=1).to(q.dtype).reshape(2 * B, -1)
    q = q.reshape(2 * B, -1)
    part = (q ** 2).sum(-1) + (t ** 2).sum(-1)
    loss = 1 - 2 * (t * q).sum(-1) / torch.clamp(part, min=eps)
    return loss.sum() / B


def ce_on_probabilities(q, target, weighted):
    """CrossEntropyLoss(weight, ignore_index=255) with q [B, 2, S, S] taken as logits, written out:
    sum_p w_y nll_p / sum_p w_y over the pixels labelled 0 or 1; weighted: w = [1, #bg / #fg]
    (model_util.py:27-37; with no foreground pixel the weight multiplies nothing)."""
    lsm = torch.log_softmax(q, dim=1)
    bg, fg = target == 0, target == 1
    w1 = bg.sum().to(q.dtype) / fg.sum().to(q.dtype) if weighted and int(fg.sum()) > 0 else 1.0
    num = -(lsm[:, 0][bg].sum() + w1 * lsm[:, 1][fg].sum())
    return num / (bg.sum() + w1 * fg.sum())


def seg_loss_pb(q, target, loss_type):
    """SegLoss(loss_type).forward(q, target, 'pb') (model_util.py:16-24)."""
    if loss_type in ("wt_dc", "dc"):
        return weighted_dice_loss(q, target)
    return ce_on_probabilities(q, target, weighted=loss_type != "ce")


def head_loss(W, f, target, idx_cls, loss_type):
    """-> (loss, low-resolution logits)."""
    lg = head_logits(W, f)
    q = compress_pred(upsample(lg, target.shape[-1]), idx_cls)
    return seg_loss_pb(q, target, loss_type), lg


def iut_of_mask(mask, target):
    """intersectionAndUnionGPU(mask, target, 2, 255) per image: [B, 3, 2] float64."""
    B = mask.shape[0]
    iut = torch.zeros(B, 3, 2, dtype=torch.float64)
    for b in range(B):
        live = target[b] != 255
        for k in range(2):
            o, t = (mask[b] == k) & live, target[b] == k
            iut[b, 0, k] = (o & t).sum()
            iut[b, 2, k] = t.sum()
            iut[b, 1, k] = o.sum() + t.sum() - (o & t).sum()
    return iut


def iut_half(z_hi, target, idx_cls):
    """The training meters' mask: compress_pred(z).argmax(1), i.e. p > 0.5 with a tie to class 0."""
    return iut_of_mask(compress_pred(z_hi, idx_cls).argmax(1), target)


def iut_argmax(z_hi, target, idx_cls):
    """pred2bmask's mask (argmax == idx_cls): NOT what the training meters use."""
    return iut_of_mask((z_hi.argmax(1) == idx_cls).long(), target)


def mix(z0_hi, z1_hi, att_wt):
    return torch.softmax(z0_hi, 1) * (1 - att_wt) + torch.softmax(z1_hi, 1) * att_wt


def mix_mask(z0_hi, z1_hi, att_wt, idx_cls):
    return (mix(z0_hi, z1_hi, att_wt).argmax(1) == idx_cls).long()


def half_share(z_hi, idx_cls):
    """Share of hi-res pixels with |p - 0.5| <= GAP."""
    p = torch.softmax(z_hi, 1)[:, idx_cls]
    return float(((p - 0.5).abs() <= GAP).double().mean())


def mix_gap_share(m):
    """(share of pixels whose top-two gap is in (0, GAP], share of exact ties)."""
    top = m.topk(2, 1).values
    g = top[:, 0] - top[:, 1]
    return float(((g > 0) & (g <= GAP)).double().mean()), float((g == 0).double().mean())


def draw_labels(rng, B, S):
    """{0, 1, 255} at p = [0.6, 0.3, 0.1] and a fully ignored band of rows: wt_ce differs from ce."""
    t = rng.choice([0, 1, 255], size=(B, S, S), p=[0.6, 0.3, 0.1]).astype(np.int64)
    t[:, 3:6, :] = 255
    t = torch.from_numpy(t)
    assert int((t == 0).sum()) != int((t == 1).sum())
    return t


_INPUTS = {}


def inputs(case, scale):
    """W [N, C] = scale U(-1, 1) / sqrt(C), f [B, C, h, h] = relu(randn), target [B, S, S]: float64
    tensors holding float32 values (the device sees the same numbers), redrawn until no hi-res
    pixel has |p - 0.5| <= GAP in float64."""
    key = (case, scale)
    if key not in _INPUTS:
        B, N, idx, C, h, S = case
        for k in range(200):
            rng = np.random.default_rng([1000 * N + 10 * S + B, int(scale), k])
            W = (scale * rng.uniform(-1, 1, (N, C)) / math.sqrt(C)).astype(np.float32)
            f = np.maximum(rng.standard_normal((B, C, h, h)), 0).astype(np.float32)
            W, f = torch.from_numpy(W).double(), torch.from_numpy(f).double()
            tgt = draw_labels(rng, B, S)
            if half_share(upsample(head_logits(W, f), S), idx) == 0.0:
                _INPUTS[key] = (W, f, tgt)
                break
        else:
            raise AssertionError("no draw clear of p = 0.5")
    return _INPUTS[key]


_REF = {}


def reference(case, scale, loss_type):
    """float64 (loss, logits, d_f, iut) of one case, computed once."""
    key = (case, scale, loss_type)
    if key not in _REF:
        W, f, tgt = inputs(case, scale)
        fo = f.clone().requires_grad_(True)
        loss, lg = head_loss(W, fo, tgt, case[2], loss_type)
        loss.backward()
        _REF[key] = (loss.detach(), lg.detach(), fo.grad, iut_half(upsample(lg.detach(), case[5]), tgt, case[2]))
    return _REF[key]


_MIX = {}


def draw_mix(case, scale=4.0):
    """Two float32 logit tensors [B, N, h, h] and a target whose mix has, at every att_wt of
    MIX_WTS and at 0, no top-two gap in (0, GAP] at any hi-res pixel in float64.  Where N > 3, class
    N-1's plane duplicates class 0's in both tensors: -10000 everywhere but +1000 at lo-res (0, 0),
    so the two tie exactly at hi-res pixel (0, 0) -- the pixel that pins the first-index rule."""
    if case not in _MIX:
        B, N, h, S = case
        tie = N > 3   # at least two live classes beside the tied pair
        for k in range(500):
            rng = np.random.default_rng([77, N, S, k])
            zs = []
            for _ in range(2):
                z = (scale * rng.standard_normal((B, N, h, h))).astype(np.float32)
                if tie:
                    z[:, 0] = -10000.0
                    z[:, 0, 0, 0] = 1000.0
                    z[:, N - 1] = z[:, 0]
                zs.append(torch.from_numpy(z))
            tgt = draw_labels(rng, B, S)
            tgt[:, 0, 0] = 1   # the tie pixel counts
            hi = [upsample(z.double(), S) for z in zs]
            ok = True
            for a in [0.0] + MIX_WTS:
                near, ties = mix_gap_share(mix(hi[0], hi[1], a))
                ok = ok and near == 0.0 and (ties > 0) == tie and ties <= 1e-2
            if ok:
                _MIX[case] = (zs[0], zs[1], tgt)
                break
        else:
            raise AssertionError("no draw with the gap")
    return _MIX[case]
