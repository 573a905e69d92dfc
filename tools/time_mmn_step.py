"""Device-event time of one MMN training step from features at the 473^2 geometry (h = w = 60,
S = 473; rmid l34, wa, agg cat, loss wt_dc, aux 0.5, WeightAverage dropouts 0.5), split into
MMN forward, loss head (forward + gradient, both heads), MMN backward and SGD.
python tools/time_mmn_step.py [shots] [steps] [--out FILE]"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from few_shot_seg_cwt_amd.match import MMN, init_match_params  # noqa: E402
from few_shot_seg_cwt_amd.optimizer import HipSGD  # noqa: E402
from few_shot_seg_cwt_amd.seg_loss import seg_head_loss  # noqa: E402

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
if out_path:
    argv.remove(out_path)
shots = int(argv[0]) if len(argv) > 0 else 1
steps = max(20, int(argv[1])) if len(argv) > 1 else 20
dev = torch.device("cuda", 0)
h, S, aux = 60, 473, 0.5
args = dict(rmid="l34", layers=50, all_lr="l", temp=20.0, att_wt=0.2, conv4d="red", att_drop=0.5, proj_drop=0.5)
net = MMN(args, agg="cat", wa=True, device=dev).train()
init_match_params(net, 1)
opt = HipSGD(list(net.parameters()), lr=1e-3, momentum=0.9, weight_decay=1e-4, nesterov=True)
g = torch.Generator().manual_seed(3)
mk = lambda n, c: torch.rand(n, c, h, h, generator=g).to(dev).contiguous(memory_format=torch.channels_last)  # noqa
fq_lst = {3: [mk(1, 1024)], 4: [mk(1, 2048)]}
fs_lst = {3: [mk(shots, 1024)], 4: [mk(shots, 2048)]}
f_q, f_s = mk(1, 512), mk(shots, 512)
W = ((torch.rand(2, 512, generator=g) * 2 - 1) / 512 ** 0.5).to(dev)
q_label = (torch.rand(1, S, S, generator=g) < 0.3).long()
q_label[:, :4] = 255
q_label = q_label.to(dev)
PHASES = ("mmn_forward", "loss_head", "mmn_backward", "sgd")


def step():
    """One step; returns the five events that bracket its four phases."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    ev[0].record()
    fq, att_fq = net(fq_lst, fs_lst, f_q, f_s)
    ev[1].record()
    # the loss head forms d loss / d feature in its forward call; autograd's backward then only
    # scales and adds the two kept gradients, so run the heads on detached leaves and time them alone
    a, b = att_fq.detach().requires_grad_(True), fq.detach().requires_grad_(True)
    loss = seg_head_loss(W, a, q_label, "wt_dc") + aux * seg_head_loss(W, b, q_label, "wt_dc")
    loss.backward()
    ev[2].record()
    torch.autograd.backward([att_fq, fq], [a.grad, b.grad])
    ev[3].record()
    opt.step()
    opt.zero_grad(set_to_none=True)
    ev[4].record()
    return ev


for _ in range(3):
    step()
torch.cuda.synchronize()
ts = {p: [] for p in PHASES + ("step",)}
for _ in range(steps):
    ev = step()
    torch.cuda.synchronize()
    for i, p in enumerate(PHASES):
        ts[p].append(ev[i].elapsed_time(ev[i + 1]))
    ts["step"].append(ev[0].elapsed_time(ev[4]))
med = lambda v: round(sorted(v)[len(v) // 2], 3)  # noqa: E731
out = {"h": h, "S": S, "shots": shots, "steps": steps, "att_drop": 0.5, "proj_drop": 0.5, "aux": aux}
out.update({p + "_ms": med(v) for p, v in ts.items()})
out.update({"loss_head_min_ms": round(min(ts["loss_head"]), 3), "loss_head_max_ms": round(max(ts["loss_head"]), 3)})
out["loss_head_share"] = round(out["loss_head_ms"] / out["step_ms"], 4)
line = json.dumps(out)
print(line)
if out_path:
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")
