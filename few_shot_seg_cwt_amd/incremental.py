"""Class-incremental (base + novel) episodes: the device counterparts of the reference's
``train_cca.py`` -- its training step and epoch (src/train_cca.py:110-256) and its validation path
(src/train_cca.py:267-390) -- and of the helpers it takes from ``model_util.py`` -- reset_cls_wt,
reset_spt_label, pred2bmask, compress_pred -- around the N-way inner loop
(``PSPNet.increment_inner_loop``, pspnet.py:207-221).

One episode, starting from features (``incremental_episode``):
  reset_cls_wt          base rows from pre_cls_wt, a fresh row idx_cls from the host RNG
  classify the supports W . f_s (cwt_linear)
  reset_spt_label       background -> the base classes' pseudo-label, 1 -> idx_cls (cwt_relabel_support)
  increment_inner_loop  adapt_iter N-way SGD steps (cwt_inner_adapt_nway)
  pred_q0 = W . f_q     scored as a binary mask argmax == idx_cls (cwt_seg_metrics_nway)
  with the MMN head ``Trans`` in eval mode: (fq, att_fq) = Trans(fq_lst, fs_lst, f_q, f_s),
                        pred_q1 = W . att_fq and pred_q = W . fq, scored the same way, and
                        pred_q2 = softmax(pred_q0) (1 - att_wt) + softmax(pred_q1) att_wt
                        (cwt_seg_metrics_nway_mix).

One training episode (``train_step``, train_cca.py:119-205), idx_cls = subcls[0], a classifier of
max(num_classes_tr, idx_cls + 1) rows:
  reset_cls_wt -> classify the supports -> reset_spt_label -> increment_inner_loop, as above
  Trans.train(); (fq, att_fq) = Trans(fq_lst, fs_lst, f_q, f_s)   one call over the shot support rows
  q_loss1 = seg_head_loss_nway(W, att_fq), q_loss = seg_head_loss_nway(W, fq), q_loss0 on f_q
            under no_grad: SegLoss(loss_type)(compress_pred(., idx_cls, 'lg'), q_label, 'pb')
            (cwt_seg_head_loss_nway), which also gives the meters' IoU counts of the mask p > 0.5
  loss = q_loss1 (+ aux q_loss); backward, optimizer.step(), zero_grad(set_to_none=True),
  scheduler.step() (cosine, per iteration)
``train_epoch`` adds the reference's meters and log lines; host readback happens only where the
reference prints or fills a meter.

Declared differences: use_amp (fp16 autocast + GradScaler) is not reproduced, the step runs at fp32
width; batch_size is 1; loss_shot == 'sum' raises NotImplementedError: at train_cca.py:168-171 the
reference sends the N-channel logits with 'lg' into the two-channel SegLoss, which fails on a shape
or weight-size mismatch for wt_dc / wt_ce and is a different loss for ce -- there is nothing
well-defined to mirror.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from .detr import linear
from .episode import _a, inner_adapt_nway
from .seg_loss import seg_head_loss_nway
from .util import AverageMeter


def reset_cls_wt(W: torch.Tensor, pre_cls_wt: torch.Tensor, num_classes_tr: int, idx_cls: int) -> torch.Tensor:
    """model_util.py:112-116, in place on W [N,C]: rows [0, num_classes_tr) from pre_cls_wt, row
    idx_cls uniform(-1/sqrt(C), 1/sqrt(C)) drawn on the host from the global torch RNG (as
    episode.new_binary_classifier_weight draws)."""
    Cc = W.shape[1]
    W[:num_classes_tr].copy_(pre_cls_wt.reshape(num_classes_tr, Cc))
    std = 1.0 / math.sqrt(Cc)
    W[idx_cls].copy_(torch.empty(Cc).uniform_(-std, std))
    return W


def classify_nway(W: torch.Tensor, f: torch.Tensor) -> torch.Tensor:
    """W [N,C] . f [B,C,h,w] (channels_last) -> logits [B,N,h,w] (cwt_linear over the pixels)."""
    B, Cc, h, w = f.shape
    x = f.permute(0, 2, 3, 1).reshape(B * h * w, Cc)
    if not x.is_contiguous():
        x = x.contiguous()
    out = linear(x, W)
    return out.reshape(B, h, w, W.shape[0]).permute(0, 3, 1, 2).contiguous()


def _check_nway(logits, lbl, idx_cls):
    _lib.require(logits, "logits")
    _lib.require(lbl, "label", torch.int64)
    B, N, h, w = logits.shape
    S = lbl.shape[-1]
    if lbl.shape != (B, S, S):
        raise ValueError(f"label must be [B,S,S] with B = {B}")
    return B, N, h, w, S, logits.contiguous(), lbl.contiguous()


def reset_spt_label(s_label: torch.Tensor, pred: torch.Tensor, idx_cls: int) -> torch.Tensor:
    """model_util.py:119-127 on low-resolution logits pred [B,N,h,w]; returns the new labels
    (s_label is left as it is)."""
    B, N, h, w, S, lg, sl = _check_nway(pred, s_label, idx_cls)
    out = torch.empty_like(sl)
    _lib.check(_lib.lib().cwt_relabel_support(_lib.ctx(lg.device.index), _lib.ptr(lg), _lib.ptr(sl), B, N, h, w, S,
                                              int(idx_cls), _lib.ptr(out), _lib.stream_ptr(lg.device)),
               "cwt_relabel_support")
    return out


def pred2bmask_metrics(pred: torch.Tensor, q_label: torch.Tensor, idx_cls: int, with_ce: bool = True):
    """pred2bmask + intersectionAndUnionGPU(., 2, 255) (+ compress_pred's NLL) of pred [B,N,h,w]
    against q_label [B,S,S] in {0, 1, 255}: iut [B,3,2] float32, ce [B,2] float64 (sum, count)."""
    B, N, h, w, S, lg, ql = _check_nway(pred, q_label, idx_cls)
    iut = torch.empty((B, 3, 2), device=lg.device, dtype=torch.float32)
    ce = torch.empty((B, 2), device=lg.device, dtype=torch.float64) if with_ce else None
    _lib.check(_lib.lib().cwt_seg_metrics_nway(_lib.ctx(lg.device.index), _lib.ptr(lg), _lib.ptr(ql), B, N, h, w, S,
                                               int(idx_cls), _lib.ptr(iut), _lib.ptr(ce),
                                               _lib.stream_ptr(lg.device)), "cwt_seg_metrics_nway")
    return iut, ce


def compress_pred_nll(pred: torch.Tensor, q_label: torch.Tensor, idx_cls: int) -> torch.Tensor:
    """Mean NLL of log(compress_pred(pred)) against q_label (train_cca.py:352-356), a 0-d float64."""
    _, ce = pred2bmask_metrics(pred, q_label, idx_cls)
    return ce[:, 0].sum() / ce[:, 1].sum()


def pred_mix_metrics(pred0: torch.Tensor, pred1: torch.Tensor, att_wt: float, q_label: torch.Tensor,
                     idx_cls: int) -> torch.Tensor:
    """pred_q2 of train_cca.py:347, 353: pred2bmask(softmax(pred0) (1 - att_wt) + softmax(pred1) att_wt)
    on the upsampled logits [B,N,h,w], + intersectionAndUnionGPU(., 2, 255): iut [B,3,2] float32."""
    B, N, h, w, S, l0, ql = _check_nway(pred0, q_label, idx_cls)
    _lib.require(pred1, "logits")
    if pred1.shape != pred0.shape:
        raise ValueError(f"the two predictions differ in shape: {tuple(pred0.shape)} and {tuple(pred1.shape)}")
    l1 = pred1.contiguous()
    iut = torch.empty((B, 3, 2), device=l0.device, dtype=torch.float32)
    _lib.check(_lib.lib().cwt_seg_metrics_nway_mix(_lib.ctx(l0.device.index), _lib.ptr(l0), _lib.ptr(l1),
                                                   float(att_wt), _lib.ptr(ql), B, N, h, w, S, int(idx_cls),
                                                   _lib.ptr(iut), _lib.stream_ptr(l0.device)),
               "cwt_seg_metrics_nway_mix")
    return iut


def increment_inner_loop(f_s: torch.Tensor, s_label: torch.Tensor, W: torch.Tensor, cls_idx: int, args) -> torch.Tensor:
    """PSPNet.increment_inner_loop (pspnet.py:207-221), in place on W [N,C]."""
    return inner_adapt_nway(f_s, s_label, W, float(_a(args, "cls_lr", 0.1)), int(_a(args, "adapt_iter", 200)),
                            int(cls_idx), float(_a(args, "tp", 1.0)))


def incremental_episode(args, f_s, s_label, f_q, q_label, W_base, idx_cls: int, Trans=None, fs_lst=None,
                        fq_lst=None) -> dict:
    """One episode of train_cca.py:306-370 from features: f_s [n,C,h,w], s_label [n,S,S] (0, 1, 255),
    f_q [1,C,h,w], q_label [1,S,S], W_base [num_classes_tr,C]; the classifier has idx_cls + 1 rows
    (idx_cls = num_classes_tr, the novel class).  Trans: the MMN head (match.MMN) in eval mode, with
    the per-layer features fs_lst / fq_lst of extract_features; Trans(fq_lst, fs_lst, f_q, f_s) is
    the reference's per-shot calls, their mean over the shots and the blend
    fq = f_q (1 - att_wt) + att_fq att_wt (train_cca.py:331-340).  Returns W, the relabelled supports
    and, per prediction, its iut [1,3,2] and ce [1,2]: pred_q0 = W . f_q ('iut0', 'ce0'), and with
    Trans pred_q1 = W . att_fq ('iut1', 'ce1': the reference's loss is on this one) and
    pred_q = W . fq ('iut', 'ce'), and 'iut2' of pred_q2, the softmax mix of pred_q0 and pred_q1 at
    args.att_wt (Trans.att_wt where args has none)."""
    ntr = W_base.shape[0]
    N = max(ntr, idx_cls + 1)
    W = torch.zeros((N, W_base.shape[1]), device=f_s.device, dtype=torch.float32)
    reset_cls_wt(W, W_base, ntr, idx_cls)
    new_label = reset_spt_label(s_label, classify_nway(W, f_s), idx_cls)
    increment_inner_loop(f_s, new_label, W, idx_cls, args)
    pred_q0 = classify_nway(W, f_q)
    out = {"W": W, "s_label": new_label, "pred_q0": pred_q0}
    out["iut0"], out["ce0"] = pred2bmask_metrics(pred_q0, q_label, idx_cls)
    if Trans is not None:
        if Trans.training:
            raise ValueError("incremental_episode scores with Trans in eval mode")
        if fs_lst is None or fq_lst is None:
            raise ValueError("incremental_episode: Trans needs the per-layer features fs_lst and fq_lst")
        with torch.no_grad():
            fq, att_fq = Trans(fq_lst, fs_lst, f_q, f_s)
        out["pred_q1"], out["pred_q"] = classify_nway(W, att_fq), classify_nway(W, fq)
        out["iut1"], out["ce1"] = pred2bmask_metrics(out["pred_q1"], q_label, idx_cls)
        out["iut"], out["ce"] = pred2bmask_metrics(out["pred_q"], q_label, idx_cls)
        out["iut2"] = pred_mix_metrics(pred_q0, out["pred_q1"], float(_a(args, "att_wt", Trans.att_wt)), q_label,
                                       idx_cls)
    return out


def validate_epoch(args, val_loader, model, W_base, Trans=None, episodes_out: list | None = None) -> dict:
    """train_cca.py:286-390: args.test_num episodes (default: one pass over val_loader) around
    incremental_episode, with the reference's class-wise foreground IoU meters.  val_loader yields
    (qry_img, q_label, spt_imgs [1,n,3,S,S], s_label [1,n,S,S], subcls, ...); model.extract_features
    gives (f [B,C,h,w], per-layer features).  Returns the mIoU and class IoUs of pred_q0 ('0') and,
    with Trans, of pred_q1 ('1'), pred_q ('') and pred_q2 ('2'), and the mean NLL of compress_pred(pred_q1) -- of
    pred_q0 without Trans.  episodes_out collects every episode's result."""
    from .mmn_train import _features
    names = ("0",) + (("1", "", "2") if Trans is not None else ())
    inter = {k: {} for k in names}
    union = {k: {} for k in names}
    loss = AverageMeter()
    idx_cls = int(_a(args, "num_classes_tr", W_base.shape[0]))
    dev = W_base.device
    model.eval()
    if Trans is not None:
        Trans.eval()
    n_test = _a(args, "test_num", None)
    it, e = iter(val_loader), 0
    while n_test is None or e < int(n_test):
        try:
            batch = next(it)
        except StopIteration:
            if n_test is None:
                break
            it = iter(val_loader)
            batch = next(it)
        e += 1
        qry_img, q_label, spt_imgs, s_label, subcls = batch[:5]
        cls = int(subcls[0]) if not isinstance(subcls, int) else subcls
        f_s, fs_lst, f_q, fq_lst = _features(model, spt_imgs[0], qry_img, dev)
        r = incremental_episode(args, f_s, s_label[0].to(dev).long(), f_q, q_label.to(dev).long(), W_base, idx_cls,
                                Trans, fs_lst, fq_lst)
        for k in names:
            iut = r["iut" + k].cpu().numpy()[0]
            inter[k][cls] = inter[k].get(cls, 0.0) + float(iut[0, 1])   # the foreground alone
            union[k][cls] = union[k].get(cls, 0.0) + float(iut[1, 1])
        ce = r["ce1" if Trans is not None else "ce0"].cpu().numpy()[0]
        loss.update(ce[0] / max(ce[1], 1.0))
        if episodes_out is not None:
            episodes_out.append(r)
    res = {"loss": loss.avg}
    for k in names:
        iou = {c: inter[k][c] / (union[k][c] + 1e-10) for c in inter[k]}
        res["class_iou" + k] = iou
        res["mIoU" + k] = float(np.mean(list(iou.values()))) if iou else 0.0
    return res


def _iou_from_iut(iut_h):
    """(IoU background, IoU foreground) from a host [3, 2] intersection / union / target table."""
    return iut_h[0] / (iut_h[1] + 1e-10)


def train_step(args, model, Trans, optimizer, scheduler, batch, W_base, dev, record: dict | None = None) -> dict:
    """One episode of train_cca.py:119-205 up to and including the optimiser and scheduler steps;
    W_base [num_classes_tr, C] is pre_cls_wt.  Returns device tensors (losses, low-resolution logits,
    the heads' iut tables); nothing is read back."""
    if _a(args, "loss_shot", "avg") != "avg":
        raise NotImplementedError(
            "loss_shot == 'sum': train_cca.py:168-171 sends N-channel logits with 'lg' into the two-channel SegLoss "
            "(a shape / weight-size mismatch for wt_dc and wt_ce, another loss for ce); there is nothing "
            "well-defined to mirror")
    from .mmn_train import _features
    qry_img, q_label, spt_imgs, s_label, subcls = batch[:5]
    idx_cls = int(subcls[0]) if not isinstance(subcls, int) else subcls
    loss_type = _a(args, "loss_type", "wt_ce")
    aux = _a(args, "aux", False)
    ntr = int(_a(args, "num_classes_tr", W_base.shape[0]))
    model.eval()
    sl = s_label[0].to(dev, non_blocking=True).long()
    ql = q_label.to(dev, non_blocking=True).long()
    f_s, fs_lst, f_q, fq_lst = _features(model, spt_imgs[0], qry_img, dev)
    W = torch.zeros((max(ntr, idx_cls + 1), W_base.shape[1]), device=dev, dtype=torch.float32)
    reset_cls_wt(W, W_base, ntr, idx_cls)
    new_label = reset_spt_label(sl, classify_nway(W, f_s), idx_cls)
    increment_inner_loop(f_s, new_label, W, idx_cls, args)
    with torch.no_grad():
        q_loss0, pred_q0, iut0 = seg_head_loss_nway(W, f_q, ql, idx_cls, loss_type, True, True)
    Trans.train()
    fq, att_fq = Trans(fq_lst, fs_lst, f_q, f_s)
    q_loss1, pred_q1, iut1 = seg_head_loss_nway(W, att_fq, ql, idx_cls, loss_type, True, True)
    if aux is False or aux is None:
        with torch.no_grad():
            q_loss, pred_q, iut = seg_head_loss_nway(W, fq.detach(), ql, idx_cls, loss_type, True, True)
        loss = q_loss1
    else:
        q_loss, pred_q, iut = seg_head_loss_nway(W, fq, ql, idx_cls, loss_type, True, True)
        loss = q_loss1 + float(aux) * q_loss
    loss.backward()
    optimizer.step()
    optimizer.zero_grad(set_to_none=True)
    if _a(args, "scheduler", None) == "cosine" and scheduler is not None:
        scheduler.step()
    out = dict(q_loss0=q_loss0, q_loss1=q_loss1.detach(), q_loss=q_loss.detach(), pred_q0=pred_q0, pred_q1=pred_q1,
               pred_q=pred_q, iut0=iut0, iut1=iut1, iut=iut, q_label=ql, W=W, idx_cls=idx_cls, s_label=new_label)
    if record is not None:   # the step's inputs, for teacher-forced checks
        record.update(out, f_s=f_s, f_q=f_q, fs_lst=fs_lst, fq_lst=fq_lst)
    return out


def train_epoch(args, train_loader, model, Trans, W_base, optimizer, scheduler, epoch: int, log=print,
                records: list | None = None, val_hook=None):
    """train_cca.py:110-256 for one epoch (batch_size 1): every episode of ``train_loader`` through
    train_step, the reference's meters and log lines; IoUb / IoUf come from the loss heads' iut
    tables (pred.argmax(1) of the compressed prediction).  Every ``args.log_iter`` iterations
    (i % log_iter == 1, as the reference counts) the CompareMeter line is logged and ``val_hook()``
    (validate_epoch and the model selection around it) runs when given.
    Returns (mIoU0, mIoU1, loss0, loss1) averaged over the epoch."""
    from .mmn_train import CompareMeter, _next
    if int(_a(args, "batch_size", 1)) != 1:
        raise NotImplementedError("batch_size must be 1")
    dev = W_base.device
    loss_m0, loss_m1, iou_m0, iou_m1 = AverageMeter(), AverageMeter(), AverageMeter(), AverageMeter()
    compare = CompareMeter()
    aux = _a(args, "aux", False)
    log_iter = int(_a(args, "log_iter", 0) or 0)
    it = iter(train_loader)
    for i in range(1, len(train_loader) + 1):
        rec = {} if records is not None else None
        r = train_step(args, model, Trans, optimizer, scheduler, _next(it), W_base, dev, rec)
        if records is not None:
            records.append(rec)
        IoUb, IoUf = {}, {}
        for idx, key in enumerate(("iut0", "iut1", "iut")):
            IoUb[idx], IoUf[idx] = _iou_from_iut(r[key].cpu().numpy()[0])
        l0, l1 = float(r["q_loss0"].item()), float(r["q_loss1"].item())
        _lib.check_status()
        loss_m0.update(l0, 1)
        iou_m0.update((IoUf[0] + IoUb[0]) / 2, 1)
        loss_m1.update(l1, 1)
        iou_m1.update((IoUf[1] + IoUb[1]) / 2, 1)
        compare.update(IoUf[1], IoUf[0])
        if i % 100 == 0 or (epoch == 1 and i <= 1000 and i % 20 == 0):
            msg = ("Ep{}/{} IoUf0 {:.2f} IoUb0 {:.2f} IoUf1 {:.2f} IoUb1 {:.2f} IoUf {:.2f} IoUb {:.2f} "
                   "loss0 {:.2f} loss1 {:.2f} d {:.2f} lr {:.4f}").format(
                epoch, i, IoUf[0], IoUb[0], IoUf[1], IoUb[1], IoUf[2], IoUb[2], l0, l1, l1 - l0, optimizer.lr)
            if aux is not False and aux is not None:
                msg += "auxL {:.2f}".format(float(r["q_loss"].item()))
            log(msg)
        if log_iter and i % log_iter == (1 if log_iter > 1 else 0):
            log("------Ep{}/{} FG IoU1 compared to IoU0 win {}/{} avg diff {:.2f}".format(
                epoch, i, compare.win_cnt, compare.cnt, compare.diff_avg))
            compare.reset()
            if val_hook is not None:
                val_hook()
    log("===========Epoch {}===========: The mIoU0 {:.2f}, mIoU1 {:.2f}, loss0 {:.2f}, loss1 {:.2f}===========\n".format(
        epoch, iou_m0.avg, iou_m1.avg, loss_m0.avg, loss_m1.avg))
    return iou_m0.avg, iou_m1.avg, loss_m0.avg, loss_m1.avg
