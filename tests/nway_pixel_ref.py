"""Float64 torch statements of the per-pixel N-way operations (model_util.py:119-127 reset_spt_label;
model_util.py:158-175 pred2bmask / compress_pred with intersectionAndUnionGPU(., 2, 255)) and the
logits their tests draw -- a helper, nothing from few_shot_seg_cwt_amd."""
import numpy as np
import torch
import torch.nn.functional as F

GAP = 1e-4


def upsample(logits, S):
    return F.interpolate(logits.double(), size=(S, S), mode="bilinear", align_corners=True)


def reset_spt_label_literal(s_label, pred_hi, idx_cls):
    """The reference's two assignments, word for word, on copies."""
    pred, s_label = pred_hi.clone(), s_label.clone()
    pred[:, idx_cls, :, :] = -1000.0
    pred_mask = pred.argmax(1)
    idx_bg = torch.where(s_label == 0)
    s_label[idx_bg] = pred_mask[idx_bg]
    s_label[torch.where(s_label == 1)] = idx_cls
    return s_label


def metrics_ref(pred_hi, q_label, idx_cls):
    """iut [B,3,2] and ce [B,2] (sum, count) in float64."""
    B = pred_hi.shape[0]
    mask = (pred_hi.argmax(1) == idx_cls).long()
    iut = torch.zeros(B, 3, 2, dtype=torch.float64)
    ce = torch.zeros(B, 2, dtype=torch.float64)
    lsm = torch.log_softmax(pred_hi, 1)
    lfg = lsm[:, idx_cls]
    others = torch.cat([pred_hi[:, :idx_cls], pred_hi[:, idx_cls + 1:]], 1)
    lbg = torch.logsumexp(others, 1) - torch.logsumexp(pred_hi, 1)   # log(1 - p_fg), never from 1 - p
    for b in range(B):
        live = q_label[b] != 255
        for k in range(2):
            o, t = (mask[b] == k) & live, (q_label[b] == k)
            iut[b, 0, k] = (o & t).sum()
            iut[b, 2, k] = t.sum()
            iut[b, 1, k] = o.sum() + t.sum() - (o & t).sum()
        ce[b, 0] = -(lfg[b][q_label[b] == 1].sum() + lbg[b][q_label[b] == 0].sum())
        ce[b, 1] = ((q_label[b] == 0) | (q_label[b] == 1)).sum()
    return iut, ce


def gap_of(pred_hi):
    """Smallest top-two gap over the hi-res pixels, exact ties excluded; and the share of exact ties."""
    top = pred_hi.topk(2, 1).values
    g = top[:, 0] - top[:, 1]
    tie = g == 0
    return float(g[~tie].min()), float(tie.double().mean())


def draw_logits(seed, B, N, h, S, scale=30.0):
    """float32 [B,N,h,h] whose upsampled top-two gap exceeds GAP at every hi-res pixel in float64,
    exact ties apart (redrawn until it holds).  Where one pixel is at most 0.1 % of the image and
    N > 2, class N-1's plane duplicates class 0's: -10000 everywhere but +1000 at lo-res (0, 0), so the
    two tie exactly at hi-res pixel (0, 0) alone -- the pixel that pins the first-index rule."""
    tie = N > 2 and S * S >= 1000
    for k in range(200):
        rng = np.random.default_rng([seed, k])
        z = (scale * rng.standard_normal((B, N, h, h))).astype(np.float32)
        if tie:
            z[:, 0] = -10000.0
            z[:, 0, 0, 0] = 1000.0
            z[:, N - 1] = z[:, 0]
        t = torch.from_numpy(z)
        g, share = gap_of(upsample(t, S))
        if g > GAP and share <= 1e-3 and (share > 0) == tie:
            return t
    raise AssertionError("no draw with the gap")
