"""Wall time of the MMN head at the 473^2 geometry (h = w = 60): MMN.forward (rmid l34, wa,
agg cat; one query, `shots` supports) and MatchNet.corr_forward alone (the head's in_channel, v 512
channels).  --rmid / --all-lr / --layers choose the correlation channels as the reference's configs do
(mmn.py:39): the default l34 / l is 2 channels, l34 / 34 is 9 (R50) or 26 (R101), l234 / 234 is 13 or 30.
python tools/time_match.py [shots] [reps] [--rmid l34] [--all-lr 34] [--layers 50]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from few_shot_seg_cwt_amd.match import MMN, init_match_params  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("shots", type=int, nargs="?", default=1)
ap.add_argument("reps", type=int, nargs="?", default=10)
ap.add_argument("--rmid", default="l34")
ap.add_argument("--all-lr", default="l")
ap.add_argument("--layers", type=int, default=50, choices=[50, 101])
opt = ap.parse_args()
shots, reps = opt.shots, opt.reps
dev = torch.device("cuda", 0)
h = 60
args = dict(rmid=opt.rmid, layers=opt.layers, all_lr=opt.all_lr, temp=20.0, att_wt=0.2, conv4d="red")
net = MMN(args, agg="cat", wa=True, device=dev)
init_match_params(net, 1)
g = torch.Generator().manual_seed(3)
mk = lambda n, c: torch.rand(n, c, h, h, generator=g).to(dev).contiguous(memory_format=torch.channels_last)  # noqa
chans = {2: 512, 3: 1024, 4: 2048}
# per layer of rmid every bottleneck's feature if all_lr names the layer, else the last one's
nfeat = {b: net.nbottlenecks[b - 1] if str(b) in opt.all_lr else 1 for b in net.bid_lst}
fq_lst = {b: [mk(1, chans[b]) for _ in range(n)] for b, n in nfeat.items()}
fs_lst = {b: [mk(shots, chans[b]) for _ in range(n)] for b, n in nfeat.items()}
f_q, f_s = mk(1, 512), mk(shots, 512)
L = net.corr_net.in_channel
corr = torch.rand(shots, L, h * h, h * h, generator=g).to(dev)


def timed(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return round(ts[len(ts) // 2], 3)


G = torch.rand(1, 512, h, h, generator=g).to(dev)


def train_step():
    """the head's forward + backward as the MMN trainers run it (train_cca.py:158-196)"""
    net.zero_grad(set_to_none=True)
    fq, att_fq = net(fq_lst, fs_lst, f_q, f_s)
    (att_fq * G).sum().backward()


with torch.no_grad():
    out = {"h": h, "shots": shots, "rmid": opt.rmid, "all_lr": opt.all_lr, "layers": opt.layers, "channels": L,
           "mmn_forward_ms": timed(lambda: net(fq_lst, fs_lst, f_q, f_s)),
           "corr_forward_ms": timed(lambda: net.corr_net._run(corr, h, h, f_s)),
           "weight_average_l4_ms": timed(lambda: net.wa_4(fq_lst[4][-1]))}
out["mmn_forward_backward_ms"] = timed(train_step)
print(json.dumps(out))
