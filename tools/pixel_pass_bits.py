"""SHA-256 of every output of the hi-res pixel pass's entry points on seeded inputs: seg_metrics (one
and two logits tensors, with and without CE), seg_head_loss and seg_head_loss_nway (three loss types;
loss, logits, d_f, iut), and the N-way metrics, mix metrics and support relabel.  Two builds of the
library compute the same bits exactly when the files this writes are identical.  The file holds one
digest per (entry point, shape, label kind), over every output tensor of every call in that group;
--full writes one digest per call instead, to find the call that moved.

    python tools/pixel_pass_bits.py OUT.json [--full]

Shapes (B, C, h, w, S): S - 1 = 8 (h - 1) and not, one and several blocks per image, h != w.
Labels: rows of 255, an all-255 label, a label without foreground.  Logits: random, and one pair of
identical planes (the argmax tie)."""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from few_shot_seg_cwt_amd.incremental import pred2bmask_metrics, pred_mix_metrics, reset_spt_label  # noqa: E402
from few_shot_seg_cwt_amd.seg_loss import seg_head_loss, seg_head_loss_nway  # noqa: E402
from few_shot_seg_cwt_amd.util import seg_metrics, seg_metrics_pair  # noqa: E402

dev = torch.device("cuda", 0)
SHAPES = ((1, 512, 5, 5, 33), (2, 64, 7, 7, 49), (1, 512, 6, 6, 50), (1, 64, 5, 8, 41))
LABELS = ("rows255", "all255", "nofg")
LOSSES = ("wt_ce", "wt_dc", "ce")
WAYS = (2, 3, 16, 64)
TIES = {"rows255": (False, True), "all255": (False,), "nofg": (False,)}
FULL = "--full" in sys.argv
out, calls = {}, 0


def put(key, *tensors):
    """the call's outputs in order (an absent output hashes as its position) into its group's digest:
    the first three parts of the key, or the whole key with --full"""
    global calls
    calls += 1
    hsh = out.setdefault(key if FULL else "/".join(key.split("/")[:3]), hashlib.sha256())
    hsh.update(key.encode())
    for i, t in enumerate(tensors):
        hsh.update(b"%d:" % i)
        if t is not None:
            hsh.update(t.detach().cpu().contiguous().numpy().tobytes())


def label(g, B, S, kind):
    t = (torch.rand(B, S, S, generator=g) < 0.3).long()
    t[:, 2:4] = 255
    t[:, S // 2, 1::3] = 255
    if kind == "all255":
        t[B - 1] = 255
    elif kind == "nofg":
        t[B - 1][t[B - 1] == 1] = 0
    return t.to(dev)


def head_outputs(fn, f):
    """loss (and logits, iut) without a gradient, then the loss and d_f with one"""
    with torch.no_grad():
        plain = fn(f)
    fg = f.clone().requires_grad_(True)
    res = fn(fg)
    res[0].backward()
    return (*plain, res[0], fg.grad)


for B, C, h, w, S in SHAPES:
    g = torch.Generator().manual_seed(1000 * S + h)
    f = (torch.rand(B, C, h, w, generator=g) * 2 - 1).to(dev).contiguous(memory_format=torch.channels_last)
    lg2 = (torch.randn(B, 2, h, w, generator=g) * 3).to(dev)
    lg2b = (torch.randn(B, 2, h, w, generator=g) * 3).to(dev)
    lg2[:, 1, 0] = lg2[:, 0, 0]      # a tied row
    W2 = ((torch.rand(2, C, generator=g) * 2 - 1) / C ** 0.5 * 8).to(dev)
    for kind in LABELS:
        tg = label(g, B, S, kind)
        tag = f"B{B}C{C}h{h}w{w}S{S}/{kind}"
        put(f"seg_metrics/{tag}/ce", *seg_metrics(lg2, tg, True))
        put(f"seg_metrics/{tag}/noce", *seg_metrics(lg2, tg, False))
        put(f"seg_metrics_pair/{tag}", *seg_metrics_pair(lg2, lg2b, tg))
        put(f"seg_metrics_pair/{tag}/tied", *seg_metrics_pair(lg2b, torch.stack([lg2[:, 0], lg2[:, 0]], 1), tg))
        for lt in LOSSES:
            for tie in TIES[kind]:
                Wt = torch.stack([W2[0], W2[0]]) if tie else W2
                put(f"seg_head_loss/{tag}/{lt}/tie{int(tie)}",
                    *head_outputs(lambda x: seg_head_loss(Wt, x, tg, lt, return_logits=True), f))
        for N in WAYS:
            W = ((torch.rand(N, C, generator=g) * 2 - 1) / C ** 0.5 * 8).to(dev)
            lgN = (torch.randn(B, N, h, w, generator=g) * 3).to(dev)
            lgNb = (torch.randn(B, N, h, w, generator=g) * 3).to(dev)
            for idx in sorted({0, N // 2, N - 1}):
                other = (idx + 1) % N
                for tie in TIES[kind]:
                    Wt, la, lb = W, lgN, lgNb
                    if tie:     # class idx and its neighbour: identical planes
                        Wt, la, lb = W.clone(), lgN.clone(), lgNb.clone()
                        Wt[other] = Wt[idx]
                        la[:, other] = la[:, idx]
                        lb[:, other] = lb[:, idx]
                    nt = f"{tag}/N{N}i{idx}/tie{int(tie)}"
                    for lt in LOSSES:
                        put(f"seg_head_loss_nway/{nt}/{lt}",
                            *head_outputs(lambda x: seg_head_loss_nway(Wt, x, tg, idx, lt, True, True), f))
                    put(f"nway_metrics/{nt}/ce", *pred2bmask_metrics(la, tg, idx, True))
                    put(f"nway_metrics/{nt}/noce", *pred2bmask_metrics(la, tg, idx, False))
                    put(f"nway_mix/{nt}", pred_mix_metrics(la, lb, 0.3, tg, idx))
                    put(f"relabel/{nt}", reset_spt_label(tg, la, idx))
torch.cuda.synchronize()
path = next(a for a in sys.argv[1:] if not a.startswith("--"))
os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
with open(path, "w") as fh:
    json.dump({k: v.hexdigest() for k, v in out.items()}, fh, indent=0, sort_keys=True)
    fh.write("\n")
print(f"{calls} calls, {len(out)} digests -> {path}")
