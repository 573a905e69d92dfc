"""Device-event time of one fusion-trainer (train_fuse) step from features at the 473^2 geometry
(h = w = 60, S = 473, one shot, FuseNet1(im_size=30, mid_dim=256), mid feature 2048 channels), split
into the 4-D stack's forward (both correlations; training form and fused eval form), the stack's
backward, the attention net (forward + backward), the loss head (forward + gradient), the trainable
part as a whole (FuseNet1, blend, classifier, loss, backward, SGD) and the whole step (with get_corr and
the frozen MatchNet).  Beside each, the same formula in eager torch on the same GPU and in the same
process (the reference's CenterPivotConv4d from conv2d with its materialised [16][3600][900] layer, the cat
of 2704 channels and the 1x1 convs, interpolate + cross_entropy), sampled in alternation with the device
path, one sample of each per round.  Each figure is the median (with min and max) of `reps` samples.

    python tools/time_fuse_step.py [reps] [out.json]      (default profiles/r13/fuse_step.json)
"""
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from few_shot_seg_cwt_amd import fuse  # noqa: E402
from few_shot_seg_cwt_amd.fuse_train import train_step  # noqa: E402
from few_shot_seg_cwt_amd.match import MatchNet, init_match_params  # noqa: E402
from few_shot_seg_cwt_amd.optimizer import HipSGD  # noqa: E402
from few_shot_seg_cwt_amd.transformer import FuseNet1  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 11
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r13", "fuse_step.json")
dev = torch.device("cuda", 0)
h, S, m, mid, C, CM = 60, 473, 30, 256, 512, 2048
P, n2 = h * h, m * m


def stats(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 3), "min_ms": round(v[0], 3), "max_ms": round(v[-1], 3)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


# ---- the eager formulas (the reference's own modules, restated) ----
def eager_cp4d(x, w1, b1, w2, b2, stride):
    B, Cc, ha, wa, hb, wb = x.shape
    xp = x[..., ::stride, ::stride] if stride > 1 else x
    mb, nb = xp.shape[-2:]
    ya = F.conv2d(xp.permute(0, 4, 5, 1, 2, 3).reshape(B * mb * nb, Cc, ha, wa), w1, b1, padding=1)
    ya = ya.reshape(B, mb, nb, -1, ha, wa).permute(0, 3, 4, 5, 1, 2)
    yb = F.conv2d(x.permute(0, 2, 3, 1, 4, 5).reshape(B * ha * wa, Cc, hb, wb), w2, b2, stride=stride, padding=1)
    return ya + yb.reshape(B, ha, wa, -1, mb, nb).permute(0, 3, 1, 2, 4, 5)


def eager_stack(x, p):
    y = torch.relu(eager_cp4d(x.unsqueeze(1), p[0], p[1], p[2], p[3], 2))
    return torch.relu(eager_cp4d(y, p[4], p[5], p[6], p[7], 1)).reshape(1, h, h, n2).permute(0, 3, 1, 2)


def eager_att(y2l, y2h, s_mask, pd0, pd1, p):
    x = torch.cat([y2l, y2h, s_mask.reshape(1, n2, 1, 1).expand(-1, -1, h, h), pd0, pd1], 1)
    return F.softmax(F.conv2d(torch.relu(F.conv2d(x, p[8], p[9])), p[10], p[11]), 1)


def eager_loss(pd_q, pd_q0, pd_q1, lbl):
    up = lambda t: F.interpolate(t, size=(S, S), mode="bilinear", align_corners=True)   # noqa: E731
    wt_mask = ((up(pd_q0).argmax(1) != up(pd_q1).argmax(1)) & (lbl != 255)).float()
    wt_mask[wt_mask == 0.0] = 0.001
    return (F.cross_entropy(up(pd_q), lbl, ignore_index=255, reduction="none") * wt_mask).sum() / wt_mask.sum()


# ---- the case ----
g = torch.Generator().manual_seed(3)
mk = lambda c: (torch.rand(1, c, h, h, generator=g) - 0.3).to(dev).contiguous(memory_format=torch.channels_last)   # noqa: E731
f_s, f_q, fs_mid, fq_mid = mk(C), mk(C), mk(CM), mk(CM)
W = ((torch.rand(2, C, generator=g) * 2 - 1) / C ** 0.5).to(dev)
q_label = (torch.rand(1, S, S, generator=g) < 0.3).long()
q_label[:, :4] = 255
s_label = (torch.rand(1, 1, S, S, generator=g) < 0.3).long()
batch = (None, q_label, None, s_label)
corr_net = MatchNet(temp=20.0, cv_type="red", sym_mode=True, device=dev)
init_match_params(corr_net, 1)
torch.manual_seed(5)
net = FuseNet1(im_size=m, mid_dim=mid, device=dev)
opt = HipSGD(list(net.parameters()), lr=1e-3, momentum=0.9, weight_decay=1e-4, nesterov=True)
args = dict(scheduler=None)

rec = {}
train_step(args, None, corr_net, net, opt, None, batch, dev, rec, features=(W, f_s, f_q, fs_mid, fq_mid))
l_corr, h_corr, s_mask, wv = rec["l_corr"], rec["h_corr"], rec["s_mask"], rec["weighted_v"]
pd0, pd1, ql = rec["pred_q0"], rec["pred_q1"], rec["q_label"]
params = net._params()
conv = [p.detach() for p in params[:8]]
ldx = (2 * n2 + 4 + 3) // 4 * 4
X = torch.zeros(P, ldx, device=dev)
dX = torch.rand(P, ldx, generator=g).to(dev) - 0.5
kept = {}


def dev_stack_train():
    kept["y1"] = [fuse.fuse_stack(c, conv, X, i * n2, save=True) for i, c in enumerate((l_corr, h_corr))]


def dev_stack_fused():
    for i, c in enumerate((l_corr, h_corr)):
        fuse.fuse_stack(c, conv, X, i * n2, save=False)


grads = [torch.empty_like(p) for p in conv]


def dev_stack_bwd():
    for i, c in enumerate((l_corr, h_corr)):
        fuse.fuse_stack_backward(c, conv, kept["y1"][i], X, dX, i * n2, grads, i > 0)


def dev_att():
    wt, saved = fuse.att_forward(X, n2, [p.detach() for p in params[8:]], s_mask.reshape(-1), pd0, pd1,
                                 net._packed_att0(n2, ldx))   # the repacked att.0.weight, kept as FuseNet1 keeps it
    fuse.att_backward(saved, kept["d_wt"])


def dev_loss():
    q = kept["pd_q"].detach().requires_grad_(True)
    fuse.fuse_loss_head(q, pd0, pd1, ql)[0].backward()


def dev_fusion_part():
    wt = net([l_corr, h_corr], s_mask, [pd0, pd1])
    out = fuse.fuse_blend(wv, f_q, wt)
    from few_shot_seg_cwt_amd.detr import linear_t
    pd_q = linear_t(out.permute(0, 2, 3, 1).reshape(P, C), W).t().reshape(1, 2, h, h)
    opt.zero_grad()
    fuse.fuse_loss_head(pd_q, pd0, pd1, ql)[0].backward()
    opt.step()


def dev_step():
    train_step(args, None, corr_net, net, opt, None, batch, dev, None, features=(W, f_s, f_q, fs_mid, fq_mid))


tp = [p.detach().clone().requires_grad_(True) for p in params]
topt = torch.optim.SGD(tp, lr=1e-3, momentum=0.9, weight_decay=1e-4, nesterov=True)


def eager_stack_fwd(grad=True):
    with torch.set_grad_enabled(grad):
        kept["ey2"] = [eager_stack(c, tp) for c in (l_corr, h_corr)]


def eager_stack_fwd_bwd():
    eager_stack_fwd()
    G = dX[:, :2 * n2].reshape(1, h, h, 2, n2)
    loss = sum((kept["ey2"][i] * G[:, :, :, i].permute(0, 3, 1, 2)).sum() for i in range(2))
    torch.autograd.grad(loss, tp[:8])


def eager_att_fb():
    y = [t.detach() for t in kept["ey2"]]
    wt = eager_att(y[0], y[1], s_mask, pd0, pd1, tp)
    torch.autograd.grad((wt * kept["d_wt"]).sum(), tp[8:])


def eager_loss_fb():
    q = kept["pd_q"].detach().requires_grad_(True)
    eager_loss(q, pd0, pd1, ql).backward()


def eager_fusion_part():
    y = [eager_stack(c, tp) for c in (l_corr, h_corr)]
    wt = eager_att(y[0], y[1], s_mask, pd0, pd1, tp)
    out = wv * wt[:, 0:1] + f_q * wt[:, 1:2]
    pd_q = F.conv2d(out, W.reshape(2, C, 1, 1))
    topt.zero_grad()
    eager_loss(pd_q, pd0, pd1, ql).backward()
    topt.step()


kept["d_wt"] = torch.rand(1, 2, h, h, generator=g).to(dev) - 0.5
kept["pd_q"] = rec["pred_q"]
pairs = [("stack_forward", dev_stack_train, lambda: eager_stack_fwd(True)),
         ("stack_forward_eval", dev_stack_fused, lambda: eager_stack_fwd(False)),
         ("stack_backward", dev_stack_bwd, None),
         ("attention_net", dev_att, eager_att_fb),
         ("loss_head", dev_loss, eager_loss_fb),
         ("fusion_part", dev_fusion_part, eager_fusion_part),
         ("step", dev_step, None)]
for _ in range(2):
    for _, a, b in pairs:
        a()
        if b:
            b()
    eager_stack_fwd_bwd()
torch.cuda.synchronize()
ts = {}
for _ in range(reps):
    for name, a, b in pairs:
        ts.setdefault(name, []).append(timed(a))
        if b:
            ts.setdefault(name + "_torch_eager", []).append(timed(b))
    ts.setdefault("stack_forward_backward_torch_eager", []).append(timed(eager_stack_fwd_bwd))
row = {"h": h, "S": S, "im_size": m, "mid_dim": mid, "reps": reps}
row.update({k: stats(v) for k, v in ts.items()})
med = lambda k: row[k]["median_ms"]   # noqa: E731
# eager torch's backward cannot run without its forward: compare forward + backward on both sides
row["stack_forward_backward"] = {"median_ms": round(med("stack_forward") + med("stack_backward"), 3)}
row["speedup_vs_torch"] = {k: round(med(k + "_torch_eager") / med(k), 2)
                           for k in ("stack_forward", "stack_forward_eval", "stack_forward_backward", "attention_net",
                                     "loss_head", "fusion_part")}
# the device's y2 against eager torch's on the same inputs
dev_stack_fused()
eager_stack_fwd(False)
ref = torch.cat([t.permute(0, 2, 3, 1).reshape(P, n2) for t in kept["ey2"]], 1)
row["y2_rel_diff_vs_torch"] = float((X[:, :2 * n2] - ref).abs().max() / ref.abs().max())
row["saved_y1_bytes"] = 2 * 4 * fuse.stack_saved_floats(1, h, h, h, h)
print(json.dumps(row), flush=True)
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as fh:
    json.dump({"device": torch.cuda.get_device_name(0), "reps": reps, "rows": [row]}, fh, indent=1)
