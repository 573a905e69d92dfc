"""The fusion trainer's episode step and validation on the device: the build's counterparts of
src/train_fuse.py:121-229 (the step scripts/train_fuse.sh runs) and ``validate_epoch`` (:254-360).
A trained MatchNet stays frozen; only FuseNet1 trains.

Order of operations per training episode (train_fuse.py:131-192):
  extract_features(support ++ query)   one backbone pass, the rmid features beside the feature map
  inner_adapt(f_s, s_label, W0)        the support-set inner loop
  pd_q0 = W . f_q                      the plain prediction
  l_corr0 = get_corr(fq_mid, fs_mid); h_corr = get_corr(f_q, f_s)
  CorrNet.corr_forward(l_corr0, f_s, ret_attn=True) -> l_corr, weighted_v   (frozen, no_grad)
  pd_q1 = W . weighted_v
  s_mask = support_mask(s_label, m, align_corners=True)      (validation: False, as the reference)
  wt = FusionNet([l_corr, h_corr], s_mask, [pd_q0, pd_q1])
  out = weighted_v wt0 + f_q wt1; pd_q = W . out
  loss = sum ce_i m_i / sum m_i, m_i = 1 where pred_q0 and pred_q1 disagree, else 0.001
  backward, optimizer.step(), scheduler.step() (cosine)
Nothing is read back inside the step; the epoch loop reads the loss and the counts for its meters.

Declared differences: the reference calls ``CorrNet(corr=...)``, which its own
MatchNet.forward does not accept -- the mirror calls ``corr_forward``; one shot only (the reference's cat
of [1, 2, h, w] with [shot, ...] fails for more); the classifier is the plain 2-way W of mmn_train; the
hard-coded MatchNet checkpoint path is an argument (``load_corr_net``).
"""
from __future__ import annotations

import time
from collections import defaultdict

import numpy as np
import torch

from . import _lib
from .episode import _a, _class_weight_check, classify
from .fuse import fuse_blend, fuse_loss_head, support_mask
from .heads import get_corr
from .mmn_train import _adapt, _features, _next, get_scheduler  # noqa: F401  (get_scheduler: the trainer's own)
from .util import AverageMeter


def load_corr_net(path: str, temp: float = 20.0, device=None):
    """train_fuse.py:102-105 with the path as an argument: MatchNet(temp, cv_type='red', sym_mode=True)
    from a checkpoint's 'state_dict'."""
    from .match import MatchNet
    net = MatchNet(temp=temp, cv_type="red", sym_mode=True, device=device)
    net.load_state_dict(torch.load(path, map_location="cpu")["state_dict"], strict=True)
    return net


def mid_feature(args, lst: dict):
    """train_fuse.py:157-162: 'nr' takes the deepest layer's feature, 'mid2' .. 'mid4' that layer's."""
    rmid = str(_a(args, "rmid", "nr"))
    if rmid == "nr":
        return lst[max(k for k, v in lst.items() if v)][-1]
    if rmid in ("mid2", "mid3", "mid4"):
        return lst[int(rmid[-1])][-1]
    raise KeyError(f"rmid {rmid!r}: the fusion trainer takes 'nr', 'mid2', 'mid3' or 'mid4'")


def _one_shot(f_s):
    if f_s.shape[0] != 1:
        raise ValueError(f"the fusion trainer is one-shot ({f_s.shape[0]} supports given): the reference's "
                         "FuseNet1 concatenates [1, 2, h, w] predictions with per-shot correlations")


def fuse_forward(W, f_s, f_q, fs_mid, fq_mid, s_label, CorrNet, Net, align_corners: bool):
    """The episode from the features on (train_fuse.py:153-180): -> dict of pd_q0, pd_q1, pd_q [1, 2, h, w],
    wt, out.  Differentiable in Net's parameters when they ask for it."""
    _one_shot(f_s)
    Wb = W.view(1, 2, -1)
    with torch.no_grad():
        pd_q0 = classify(Wb, f_q)
        B, _, h, w = fs_mid.shape
        l_corr0 = get_corr(fq_mid, fs_mid).reshape(B, 1, h, w, h, w)
        h_corr = get_corr(f_q, f_s).reshape(B, h, w, h, w)
        l_corr, weighted_v = CorrNet.corr_forward(l_corr0, f_s, ret_attn=True)
        l_corr = l_corr.reshape(B, h, w, h, w)
        weighted_v = weighted_v.contiguous(memory_format=torch.channels_last)
        pd_q1 = classify(Wb, weighted_v)
        s_mask = support_mask(s_label, Net.im_size, align_corners)
    wt = Net([l_corr, h_corr], s_mask, [pd_q0, pd_q1])
    out = fuse_blend(weighted_v, f_q, wt)
    if out.requires_grad:   # W . out under autograd: the exact-fp32 linear and its backward to out
        from .detr import linear_t
        C = out.shape[1]
        pd_q = linear_t(out.permute(0, 2, 3, 1).reshape(h * w, C), W.detach()).t().reshape(1, 2, h, w)
    else:
        pd_q = classify(Wb, out)
    return dict(pd_q0=pd_q0, pd_q1=pd_q1, pd_q=pd_q, wt=wt, out=out, l_corr=l_corr, h_corr=h_corr, s_mask=s_mask,
                weighted_v=weighted_v)


def train_step(args, model, CorrNet, FusionNet, optimizer, scheduler, batch, dev, record: dict | None = None,
               features=None) -> dict:
    """One episode of train_fuse.py:131-192 up to and including the optimiser and scheduler steps.
    Returns device tensors (loss, low-resolution logits, counts); nothing is read back.
    ``features`` = (W, f_s, f_q, fs_mid, fq_mid) skips the extractor and the inner loop (from-features runs)."""
    qry_img, q_label, spt_imgs, s_label = batch[:4]
    sl = s_label[0].to(dev, non_blocking=True).long()
    ql = q_label.to(dev, non_blocking=True).long()
    if sl.shape[0] != 1:
        _one_shot(sl)
    if features is None:
        model.eval()
        f_s, fs_lst, f_q, fq_lst = _features(model, spt_imgs[0], qry_img, dev)
        W = _adapt(args, f_s, sl, dev)
        fs_mid, fq_mid = mid_feature(args, fs_lst), mid_feature(args, fq_lst)
    else:
        W, f_s, f_q, fs_mid, fq_mid = features
    CorrNet.eval()
    FusionNet.train()
    r = fuse_forward(W, f_s, f_q, fs_mid, fq_mid, sl, CorrNet, FusionNet, align_corners=True)
    q_loss, iut, disagree = fuse_loss_head(r["pd_q"], r["pd_q0"], r["pd_q1"], ql)
    optimizer.zero_grad()
    q_loss.backward()
    optimizer.step()
    if _a(args, "scheduler", None) == "cosine" and scheduler is not None:
        scheduler.step()
    out = dict(q_loss=q_loss.detach(), iut=iut, disagree=disagree, pred_q0=r["pd_q0"], pred_q1=r["pd_q1"],
               pred_q=r["pd_q"].detach(), wt=r["wt"].detach(), q_label=ql, W=W)
    if record is not None:   # the step's inputs, for teacher-forced checks
        record.update(out, f_s=f_s, f_q=f_q, fs_mid=fs_mid, fq_mid=fq_mid, s_label=sl, l_corr=r["l_corr"],
                      h_corr=r["h_corr"], s_mask=r["s_mask"], weighted_v=r["weighted_v"])
    return out


def _miou_pairs(iut_h):
    """[3, 3, 2] counts -> [(IoU background, IoU foreground)] of pred_q, pred_q0, pred_q1"""
    return [tuple(iut_h[k, 0] / (iut_h[k, 1] + 1e-10)) for k in range(3)]


def train_epoch(args, train_loader, model, CorrNet, FusionNet, optimizer, scheduler, epoch: int, log=print,
                records: list | None = None, val_hook=None):
    """train_fuse.py:121-229 for one epoch (batch_size 1): every episode through train_step, the
    reference's three IoU meters and log lines; ``val_hook()`` every ``args.val_iter`` (the reference:
    1190) iterations when given.  Returns (mIoU0, mIoU1, mIoU, loss) averaged over the epoch."""
    if int(_a(args, "batch_size", 1)) != 1:
        raise NotImplementedError("batch_size must be 1 (scripts/train_fuse.sh)")
    dev = torch.device("cuda", torch.cuda.current_device())
    loss_m, iou_m, iou_m0, iou_m1 = AverageMeter(), AverageMeter(), AverageMeter(), AverageMeter()
    val_iter = int(_a(args, "val_iter", 1190) or 0)
    it = iter(train_loader)
    for i in range(1, len(train_loader) + 1):
        rec = {} if records is not None else None
        r = train_step(args, model, CorrNet, FusionNet, optimizer, scheduler, _next(it), dev, rec)
        if records is not None:
            records.append(rec)
        (IoUb, IoUf), (IoUb0, IoUf0), (IoUb1, IoUf1) = _miou_pairs(r["iut"].cpu().numpy())
        loss = float(r["q_loss"].item())
        _lib.check_status()   # after the readback's sync: surface an inner-loop barrier timeout
        loss_m.update(loss, 1)
        iou_m.update((IoUf + IoUb) / 2, 1)
        iou_m0.update((IoUf0 + IoUb0) / 2, 1)
        iou_m1.update((IoUf1 + IoUb1) / 2, 1)
        if i % 100 == 0 or (epoch == 1 and i <= 1190):
            wt0 = r["wt"][:, 0:1]
            log("Epoch {} Iter {} IoUf0 {:.2f} IoUb0 {:.2f} IoUf {:.2f} IoUb {:.2f} IoUf1 {:.2f} IoUb1 {:.2f} "
                "q_loss {:.2f} avg_wt {:.2f} std_wt {:.2f} lr {:.4f}".format(
                    epoch, i, IoUf0, IoUb0, IoUf, IoUb, IoUf1, IoUb1, loss, float(wt0.mean()), float(wt0.std()),
                    optimizer.lr))
        if val_iter and i % val_iter == 0 and val_hook is not None:
            val_hook()
    log("===========Epoch {}===========: The mIoU0 {:.2f}, mIoU1 {:.2f}, mIoU {:.2f}, loss {:.2f}===========".format(
        epoch, iou_m0.avg, iou_m1.avg, iou_m.avg, loss_m.avg))
    return iou_m0.avg, iou_m1.avg, iou_m.avg, loss_m.avg


@torch.no_grad()
def validate_epoch(args, val_loader, model, CorrNet, Net, episodes_out: list | None = None, log=print, features=None):
    """train_fuse.py:254-360: ``args.test_num`` episodes with Net in eval mode (the support mask resized
    with align_corners=False, as the reference does here); the class-wise FG IoU of pred_q0, pred_q1 and
    pred_q.  Returns (mIoU0, mIoU1, mIoU, loss_avg); the loss is the plain CE(ignore 255) of pred_q.
    ``features(batch)`` -> (W, f_s, f_q, fs_mid, fq_mid) replaces the extractor and the inner loop."""
    from .util import seg_metrics
    log("==> Start testing")
    dev = torch.device("cuda", torch.cuda.current_device())
    if model is not None:
        model.eval()
    CorrNet.eval()
    Net.eval()
    t0 = time.time()
    loss_meter = AverageMeter()
    inter = [defaultdict(float) for _ in range(3)]
    union = [defaultdict(float) for _ in range(3)]
    n_test = int(_a(args, "test_num", 1000))
    it = None

    def miou(k):
        return float(np.mean([inter[k][c] / (union[k][c] + 1e-10) for c in union[k]])) if union[k] else 0.0

    for e in range(1, n_test + 1):
        if it is None:
            it = iter(val_loader)
        try:
            batch = _next(it)
        except StopIteration:
            it = iter(val_loader)
            batch = _next(it)
        qry_img, q_label, spt_imgs, s_label, subcls = batch[:5]
        sl = s_label[0].to(dev, non_blocking=True).long()
        ql = q_label.to(dev, non_blocking=True).long()
        if features is None:
            _class_weight_check(s_label)
            f_s, fs_lst, f_q, fq_lst = _features(model, spt_imgs[0], qry_img, dev)
            W = _adapt(args, f_s, sl, dev)
            fs_mid, fq_mid = mid_feature(args, fs_lst), mid_feature(args, fq_lst)
        else:
            W, f_s, f_q, fs_mid, fq_mid = features(batch)
        r = fuse_forward(W, f_s, f_q, fs_mid, fq_mid, sl, CorrNet, Net, align_corners=False)
        _, iut, _ = fuse_loss_head(r["pd_q"], r["pd_q0"], r["pd_q1"], ql)
        _, ce = seg_metrics(r["pd_q"], ql, with_ce=True)
        iut_h, ce_h = iut.cpu().numpy(), ce.cpu().numpy()[0]
        _lib.check_status()
        cls = int(subcls[0].item())
        for k, src in enumerate((1, 2, 0)):   # meters in the reference's order: pred_q0, pred_q1, pred_q
            inter[k][cls] += float(iut_h[src, 0, 1])   # FG only
            union[k][cls] += float(iut_h[src, 1, 1])
        loss_meter.update(float(ce_h[0] / ce_h[1]) if ce_h[1] > 0 else float("nan"))
        if episodes_out is not None:
            episodes_out.append(dict(cls=cls, pred_q0=r["pd_q0"].cpu(), pred_q1=r["pd_q1"].cpu(), pred_q=r["pd_q"].cpu(),
                                     iut=iut.cpu(), wt=r["wt"].cpu(), s_mask=r["s_mask"].cpu(), loss=loss_meter.val))
        if e % 200 == 0:
            log("Test: [{}/{}] mIoU0 {:.4f} mIoU1 {:.4f} mIoU {:.4f} Loss {:.4f} ({:.4f}) ".format(
                e, n_test, miou(0), miou(1), miou(2), loss_meter.val, loss_meter.avg))
    mIoU0, mIoU1, mIoU = miou(0), miou(1), miou(2)
    log("mIoU---Val result: mIoU0 {:.4f}, mIoU1 {:.4f}, mIoU {:.4f} | time used {:.1f}m.".format(
        mIoU0, mIoU1, mIoU, (time.time() - t0) / 60))
    for c in union[2]:
        log("Class {} : {:.4f}".format(c, inter[2][c] / (union[2][c] + 1e-10)))
    return mIoU0, mIoU1, mIoU, loss_meter.avg
