"""The MMN trainer's episode step and validation on the device: the build's counterparts of
src/train_kshot.py:119-192 (the step scripts/train_mmn.sh runs) and ``validate_epoch``
(src/train_kshot.py:254-356), with ``get_scheduler`` (src/optimizer.py:20-35) over HipSGD.

Order of operations per training episode (train_kshot.py:128-192):
  extract_features(support ++ query)   one backbone pass, rmid features beside the feature map
  inner_adapt(f_s, s_label, W0)        the support-set inner loop (weighted CE)
  pred_q0 = W . f_q                    low-resolution logits (the IoU logging upsamples them)
  Trans.train(); MMN(fq_lst, fs_lst, f_q, f_s)
      loss_shot 'avg': one call over the B = shot support rows -- the same function as the
                       reference's per-shot calls, mean(0) and blend
      loss_shot 'sum': per-shot calls, a seg_head_loss each
  q_loss1 = seg_head_loss(W, att_fq), q_loss = seg_head_loss(W, fq); loss = q_loss1 + aux q_loss
  backward, optimizer.step(), zero_grad(set_to_none=True), scheduler.step() (cosine)
Host readback happens only where the reference prints or fills its meters.

Declared differences: use_amp (fp16 autocast + GradScaler) is not reproduced, the step runs at
fp32 width; meta_aug stays out; under WeightAverage's
dropouts the query feature is averaged once per MMN call, not once per expanded support row.
"""
from __future__ import annotations

import time
from collections import defaultdict

import numpy as np
import torch

from . import _lib
from .episode import _a, _class_weight_check, classify, inner_adapt, new_binary_classifier_weight
from .match import _MMNBlendFn
from .pretrain import cosine_lr
from .seg_loss import seg_head_loss
from .transformer import as_tokens
from .util import AverageMeter, seg_metrics


class CompareMeter:
    """How often, and by how much on average, score1 beats score0 (the trainer's FG IoU of the
    attended prediction against the plain one)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.cnt, self.win_cnt, self.diff_sum, self.diff_avg = 0, 0, 0.0, 0.0

    def update(self, score1, score0):
        self.cnt += 1
        self.win_cnt += int(score1 > score0)
        self.diff_sum += float(score1 - score0)
        self.diff_avg = self.diff_sum / self.cnt


class _Scheduler:
    """Closed forms of torch's CosineAnnealingLR / StepLR / MultiStepLR over ``optimizer.lr``."""

    def __init__(self, optimizer, kind, base_lr, **kw):
        self.optimizer, self.kind, self.base_lr, self.kw, self.last_epoch = optimizer, kind, float(base_lr), kw, 0

    def get_lr(self) -> float:
        t = self.last_epoch
        if self.kind == "cosine":
            return cosine_lr(self.base_lr, t, self.kw["T_max"], self.kw["eta_min"])
        if self.kind == "step":
            return self.base_lr * self.kw["gamma"] ** (t // self.kw["step_size"])
        return self.base_lr * self.kw["gamma"] ** sum(1 for m in self.kw["milestones"] if m <= t)

    def step(self):
        self.last_epoch += 1
        self.optimizer.lr = self.get_lr()

    def get_last_lr(self):
        return [self.optimizer.lr]


def get_scheduler(args, optimizer, batches: int):
    """optimizer.py:20-35: 'cosine' (stepped every iteration: CosineAnnealingLR(T_max = batches *
    epochs, eta_min = 1e-6)), 'step', 'multi_step' (stepped every epoch by the caller) or None."""
    kind = _a(args, "scheduler", None)
    if kind is None:
        return None
    base = optimizer.lr
    if kind == "cosine":
        return _Scheduler(optimizer, kind, base, T_max=int(batches) * int(_a(args, "epochs")), eta_min=1e-6)
    if kind == "step":
        return _Scheduler(optimizer, kind, base, step_size=int(_a(args, "lr_stepsize")), gamma=float(_a(args, "gamma")))
    if kind == "multi_step":
        return _Scheduler(optimizer, kind, base, milestones=sorted(int(m) for m in _a(args, "milestones")),
                          gamma=float(_a(args, "gamma")))
    raise KeyError(kind)


def _next(it):
    return it.next() if hasattr(it, "next") else next(it)


def _features(model, spt_imgs, qry_img, dev):
    """One extractor pass over supports + query (eval-mode BN: batching is exact), split into
    (f_s, fs_lst, f_q, fq_lst)."""
    shot = spt_imgs.shape[0]
    imgs = torch.cat([spt_imgs, qry_img], 0).to(dev, non_blocking=True)
    with torch.no_grad():
        f_all, lst = model.extract_features(imgs)
    fs_lst = {k: [t[:shot] for t in v] for k, v in lst.items()}
    fq_lst = {k: [t[shot:] for t in v] for k, v in lst.items()}
    return f_all[:shot], fs_lst, f_all[shot:], fq_lst


def _adapt(args, f_s, s_label, dev):
    """model.inner_loop: a fresh binary classifier (drawn from the host RNG, as the reference's
    nn.Conv2d is) trained on the supports; returns W [2, 512]."""
    W0 = new_binary_classifier_weight().to(dev)
    return inner_adapt(f_s, s_label, W0, float(_a(args, "cls_lr", 0.1)), int(_a(args, "adapt_iter", 200)))


def _iou_pair(logits, q_label):
    """(IoU background, IoU foreground) of upsampled-argmax logits, on the host."""
    iut, _ = seg_metrics(logits, q_label, with_ce=False)
    iut = iut.cpu().numpy()[0]
    return iut[0] / (iut[1] + 1e-10)


def train_step(args, model, Trans, optimizer, scheduler, batch, dev, record: dict | None = None) -> dict:
    """One episode of train_kshot.py:119-192 up to and including the optimiser and scheduler
    steps.  Returns device tensors (losses, low-resolution logits); nothing is read back."""
    qry_img, q_label, spt_imgs, s_label = batch[:4]
    shot = int(_a(args, "shot", spt_imgs.shape[1]))
    loss_type = _a(args, "loss_type", "wt_ce")
    aux = _a(args, "aux", False)
    model.eval()
    sl = s_label[0].to(dev, non_blocking=True).long()
    ql = q_label.to(dev, non_blocking=True).long()
    f_s, fs_lst, f_q, fq_lst = _features(model, spt_imgs[0], qry_img, dev)
    W = _adapt(args, f_s, sl, dev)
    with torch.no_grad():
        pred_q0 = classify(W.view(1, 2, -1), f_q)
        q_loss0 = seg_head_loss(W, f_q, ql, loss_type)
    Trans.train()
    if _a(args, "loss_shot", "avg") == "avg":
        fq, att_fq = Trans(fq_lst, fs_lst, f_q, f_s)
        q_loss1, pred_q1 = seg_head_loss(W, att_fq, ql, loss_type, return_logits=True)
    else:   # 'sum': a loss per shot on that shot's attended feature (train_kshot.py:159-162)
        att, q_loss1 = [], 0
        for k in range(shot):
            single = {key: [t[k:k + 1] for t in v] for key, v in fs_lst.items()}
            _, a = Trans(fq_lst, single, f_q, f_s[k:k + 1])
            att.append(a)
            q_loss1 = q_loss1 + seg_head_loss(W, a, ql, loss_type)
        # mean over the shots and the blend (train_kshot.py:164-166) as the device op MMN itself uses
        fq, att_fq = _MMNBlendFn.apply(as_tokens(f_q), as_tokens(torch.cat(att, 0)), Trans.att_wt)
        with torch.no_grad():
            pred_q1 = classify(W.view(1, 2, -1), att_fq.detach())
    if aux is False or aux is None:
        q_loss = None
        with torch.no_grad():
            pred_q = classify(W.view(1, 2, -1), fq.detach())
        loss = q_loss1
    else:
        q_loss, pred_q = seg_head_loss(W, fq, ql, loss_type, return_logits=True)
        loss = q_loss1 + float(aux) * q_loss
    loss.backward()
    optimizer.step()
    optimizer.zero_grad(set_to_none=True)
    if _a(args, "scheduler", None) == "cosine" and scheduler is not None:
        scheduler.step()
    out = dict(q_loss0=q_loss0, q_loss1=q_loss1.detach(), q_loss=None if q_loss is None else q_loss.detach(),
               pred_q0=pred_q0, pred_q1=pred_q1, pred_q=pred_q, q_label=ql, W=W)
    if record is not None:   # the step's inputs, for teacher-forced checks
        record.update(out, f_s=f_s, f_q=f_q, fs_lst=fs_lst, fq_lst=fq_lst)
    return out


def train_epoch(args, train_loader, model, Trans, optimizer, scheduler, epoch: int, log=print,
                records: list | None = None, val_hook=None):
    """train_kshot.py:112-243 for one epoch (batch_size 1): every episode of ``train_loader``
    through train_step, the reference's meters and log lines; ``val_hook()`` (validate_epoch and
    the model selection around it) runs every ``args.log_iter`` iterations when given.
    Returns (mIoU0, mIoU1, loss0, loss1) averaged over the epoch."""
    if int(_a(args, "batch_size", 1)) != 1:
        raise NotImplementedError("batch_size must be 1 (scripts/train_mmn.sh)")
    dev = torch.device("cuda", torch.cuda.current_device())
    loss_m0, loss_m1, iou_m0, iou_m1 = AverageMeter(), AverageMeter(), AverageMeter(), AverageMeter()
    compare = CompareMeter()
    aux = _a(args, "aux", False)
    log_iter = int(_a(args, "log_iter", 0) or 0)
    epochs = int(_a(args, "epochs", 1))
    it = iter(train_loader)
    for i in range(1, len(train_loader) + 1):
        rec = {} if records is not None else None
        r = train_step(args, model, Trans, optimizer, scheduler, _next(it), dev, rec)
        if records is not None:
            records.append(rec)
        IoUb, IoUf = {}, {}
        for idx, key in enumerate(("pred_q0", "pred_q1", "pred_q")):
            IoUb[idx], IoUf[idx] = _iou_pair(r[key], r["q_label"])
        l0, l1 = float(r["q_loss0"].item()), float(r["q_loss1"].item())
        _lib.check_status()   # after the readback's sync: surface an inner-loop barrier timeout
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
        if log_iter and i % log_iter == 0:
            log("------Ep{}/{} FG IoU1 compared to IoU0 win {}/{} avg diff {:.2f}".format(
                epoch, i, compare.win_cnt, compare.cnt, compare.diff_avg))
            compare.reset()
            if val_hook is not None:
                val_hook()
    log("===========Epoch {}===========: The mIoU0 {:.2f}, mIoU1 {:.2f}, loss0 {:.2f}, loss1 {:.2f}===========\n".format(
        epoch, iou_m0.avg, iou_m1.avg, loss_m0.avg, loss_m1.avg))
    return iou_m0.avg, iou_m1.avg, loss_m0.avg, loss_m1.avg


@torch.no_grad()
def validate_epoch(args, val_loader, model, Net, episodes_out: list | None = None, log=print):
    """train_kshot.py:254-356: ``args.test_num`` episodes with Net in eval mode; class-wise FG
    IoU of pred_q0 (plain classifier), pred_q1 (attended feature) and pred_q (blend), and the
    CE(ignore 255) of pred_q1.  Returns (mIoU, mIoU1, loss_avg); with ``episodes_out`` appends
    per-episode records (low-resolution logits, [3, 2] intersection / union / target counts)."""
    log("==> Start testing")
    dev = torch.device("cuda", torch.cuda.current_device())
    model.eval()
    Net.eval()
    t0 = time.time()
    loss_meter = AverageMeter()
    inter = [defaultdict(float) for _ in range(3)]
    union = [defaultdict(float) for _ in range(3)]
    compare = CompareMeter()
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
        _class_weight_check(s_label)
        sl = s_label[0].to(dev, non_blocking=True).long()
        ql = q_label.to(dev, non_blocking=True).long()
        f_s, fs_lst, f_q, fq_lst = _features(model, spt_imgs[0], qry_img, dev)
        W = _adapt(args, f_s, sl, dev)
        Wb = W.view(1, 2, -1)
        pred_q0 = classify(Wb, f_q)
        fq, att_fq = Net(fq_lst, fs_lst, f_q, f_s)   # B = shot rows: the per-shot calls, mean(0) and blend
        pred_q1, pred_q = classify(Wb, att_fq), classify(Wb, fq)
        iuts = []
        for k, pred in enumerate((pred_q0, pred_q1, pred_q)):
            iut, ce = seg_metrics(pred, ql, with_ce=(k == 1))
            iuts.append(iut)
            if k == 1:
                ce1 = ce
        iuts_h = [t.cpu().numpy()[0] for t in iuts]
        ce_h = ce1.cpu().numpy()[0]
        _lib.check_status()
        cls = int(subcls[0].item())
        for k in range(3):
            inter[k][cls] += float(iuts_h[k][0, 1])   # FG only
            union[k][cls] += float(iuts_h[k][1, 1])
        with np.errstate(divide="ignore", invalid="ignore"):
            compare.update(iuts_h[1][0, 1] / iuts_h[1][1, 1], iuts_h[0][0, 1] / iuts_h[0][1, 1])
        loss_meter.update(float(ce_h[0] / ce_h[1]) if ce_h[1] > 0 else float("nan"))
        if episodes_out is not None:
            episodes_out.append(dict(cls=cls, pred_q0=pred_q0.cpu(), pred_q1=pred_q1.cpu(), pred_q=pred_q.cpu(),
                                     iut0=iuts[0].cpu(), iut1=iuts[1].cpu(), iut=iuts[2].cpu(), W=W.cpu(),
                                     loss1=loss_meter.val))
        if e % 200 == 0:
            log("Test: [{}/{}] mIoU0 {:.4f} mIoU1 {:.4f} mIoU {:.4f} Loss {:.4f} ({:.4f}) ".format(
                e, n_test, miou(0), miou(1), miou(2), loss_meter.val, loss_meter.avg))
    mIoU0, mIoU1, mIoU = miou(0), miou(1), miou(2)
    log("mIoU---Val result: mIoU0 {:.4f}, mIoU1 {:.4f} mIoU {:.4f} | time used {:.1f}m.".format(
        mIoU0, mIoU1, mIoU, (time.time() - t0) / 60))
    for c in union[2]:
        log("Class {} : {:.4f}".format(c, inter[2][c] / (union[2][c] + 1e-10)))
    log("------Val FG IoU1 compared to IoU0 win {}/{} avg diff {:.2f}".format(compare.win_cnt, compare.cnt,
                                                                                compare.diff_avg))
    return mIoU, mIoU1, loss_meter.avg
