"""Device-event time of one class-incremental (train_cca) training step from features at the 473^2
geometry (h = w = 60, S = 473; rmid l34, wa, agg cat, loss wt_dc, aux 0.5), split into MMN forward,
loss head (seg_head_loss_nway: forward + gradient, both heads), MMN backward and SGD, at 1 and 5
shots and N = 16 and N = 62 classes.  In the same process, sampled in alternation with the step
(one sample of each per round, so a drift of the clocks or of the machine's load falls on all of
them alike), two comparison lines for the loss-head phase:
  torch_eager   the same formula in plain torch on the GPU (conv2d, interpolate, softmax, the dice
                loss on [1 - p, p], backward to the feature) -- what the reference launches
  two_way_head  the 2-way seg_head_loss at the same shape
Each figure is the median (with min and max) of `reps` samples after warm-up.

    python tools/time_cca_step.py [reps] [out.json]      (default profiles/r12/cca_step.json)

Exits non-zero unless the new head is faster than torch_eager at N = 16, 1 shot."""
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from few_shot_seg_cwt_amd.match import MMN, init_match_params  # noqa: E402
from few_shot_seg_cwt_amd.optimizer import HipSGD  # noqa: E402
from few_shot_seg_cwt_amd.seg_loss import seg_head_loss, seg_head_loss_nway  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r12", "cca_step.json")
dev = torch.device("cuda", 0)
h, S, aux = 60, 473, 0.5
PHASES = ("mmn_forward", "loss_head", "mmn_backward", "sgd")


def dice_pb(q, target):
    """weighted_dice_loss(q, target, reduction='sum', input_type='pb') (model_util.py:40-73)."""
    B = q.shape[0]
    t = torch.stack([target == 0, target == 1], dim=1).float().reshape(2 * B, -1)
    q = q.reshape(2 * B, -1)
    part = (q ** 2).sum(-1) + (t ** 2).sum(-1)
    return (1 - 2 * (t * q).sum(-1) / torch.clamp(part, min=1e-8)).sum() / B


def eager_head(W4, f, target, idx):
    z = F.interpolate(F.conv2d(f, W4), size=target.shape[-2:], mode="bilinear", align_corners=True)
    p = F.softmax(z, dim=1)[:, idx]
    return dice_pb(torch.stack([1.0 - p, p], dim=1), target)


def stats(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 3), "min_ms": round(v[0], 3), "max_ms": round(v[-1], 3)}


def bracket(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


rows = []
for shots in (1, 5):
    args = dict(rmid="l34", layers=50, all_lr="l", temp=20.0, att_wt=0.2, conv4d="red", att_drop=0.0, proj_drop=0.0)
    net = MMN(args, agg="cat", wa=True, device=dev).train()
    init_match_params(net, 1)
    opt = HipSGD(list(net.parameters()), lr=1e-3, momentum=0.9, weight_decay=1e-4, nesterov=True)
    g = torch.Generator().manual_seed(3)
    mk = lambda n, c: torch.rand(n, c, h, h, generator=g).to(dev).contiguous(memory_format=torch.channels_last)  # noqa
    fq_lst = {3: [mk(1, 1024)], 4: [mk(1, 2048)]}
    fs_lst = {3: [mk(shots, 1024)], 4: [mk(shots, 2048)]}
    f_q, f_s = mk(1, 512), mk(shots, 512)
    q_label = (torch.rand(1, S, S, generator=g) < 0.3).long()
    q_label[:, :4] = 255
    q_label = q_label.to(dev)
    for N in (16, 62):
        idx = N - 1
        W = ((torch.rand(N, 512, generator=g) * 2 - 1) / 512 ** 0.5).to(dev)
        W4 = W.reshape(N, 512, 1, 1)
        W2 = W[N - 2:].contiguous()
        kept = {}

        def step():
            """One step; returns the five events that bracket its four phases."""
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            ev[0].record()
            fq, att_fq = net(fq_lst, fs_lst, f_q, f_s)
            ev[1].record()
            # the loss head forms d loss / d feature in its forward call; autograd's backward then only
            # scales and adds the two kept gradients, so run the heads on detached leaves and time them alone
            a, b = att_fq.detach().requires_grad_(True), fq.detach().requires_grad_(True)
            loss = seg_head_loss_nway(W, a, q_label, idx, "wt_dc") + aux * seg_head_loss_nway(W, b, q_label, idx, "wt_dc")
            loss.backward()
            ev[2].record()
            torch.autograd.backward([att_fq, fq], [a.grad, b.grad])
            ev[3].record()
            opt.step()
            opt.zero_grad(set_to_none=True)
            ev[4].record()
            kept["a"], kept["b"] = a.detach(), b.detach()
            return ev

        def heads(fn):
            """Both heads of the step, forward + gradient, on the step's own features."""
            a, b = kept["a"].detach().requires_grad_(True), kept["b"].detach().requires_grad_(True)
            (fn(a) + aux * fn(b)).backward()
            return a.grad, b.grad

        eager = lambda: heads(lambda x: eager_head(W4, x, q_label, idx))   # noqa: E731
        two = lambda: heads(lambda x: seg_head_loss(W2, x, q_label, "wt_dc"))   # noqa: E731
        for _ in range(3):
            step()
            eager()
            two()
        torch.cuda.synchronize()
        ts = {p: [] for p in PHASES + ("step", "torch_eager", "two_way_head")}
        for _ in range(reps):
            ev = step()
            torch.cuda.synchronize()
            for i, p in enumerate(PHASES):
                ts[p].append(ev[i].elapsed_time(ev[i + 1]))
            ts["step"].append(ev[0].elapsed_time(ev[4]))
            for name, fn in (("torch_eager", eager), ("two_way_head", two)):
                e0, e1 = bracket(fn)
                torch.cuda.synchronize()
                ts[name].append(e0.elapsed_time(e1))
        # the new head's gradient against the eager formula's on the same features
        ga, _ = heads(lambda x: seg_head_loss_nway(W, x, q_label, idx, "wt_dc"))
        gt, _ = eager()
        row = {"shots": shots, "N": N, "h": h, "S": S, "aux": aux, "loss_type": "wt_dc", "reps": reps}
        row.update({p: stats(v) for p, v in ts.items()})
        row["d_f_rel_diff_vs_torch"] = float((ga - gt).abs().max() / gt.abs().max())
        row["speedup_vs_torch"] = round(row["torch_eager"]["median_ms"] / row["loss_head"]["median_ms"], 2)
        row["ratio_to_two_way_head"] = round(row["loss_head"]["median_ms"] / row["two_way_head"]["median_ms"], 2)
        row["loss_head_share"] = round(row["loss_head"]["median_ms"] / row["step"]["median_ms"], 4)
        print(json.dumps(row), flush=True)
        rows.append(row)
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as fh:
    json.dump({"device": torch.cuda.get_device_name(0), "reps": reps, "rows": rows}, fh, indent=1)
gate = next(r for r in rows if r["shots"] == 1 and r["N"] == 16)
sys.exit(0 if gate["loss_head"]["median_ms"] < gate["torch_eager"]["median_ms"] else 1)
