"""Wall time of the N-way inner loop (inner_adapt_nway, 200 steps) at 1-shot and 5-shot 473^2 for
N = 2, 16, 17, 62, beside two baselines measured in the same process and session: (a) the 2-way
loop's step launches (CWT_ADAPT_PERSIST=0) and (b) the same N-way loop in plain torch on the GPU
(conv2d, interpolate, cross_entropy, backward, SGD) -- what the reference launches.  Each figure is
the median of `reps` event-timed samples after warm-up runs, the variants sampled in alternation,
W reset before each run.

    python tools/time_adapt_nway.py [reps] [out.json]      (default profiles/r8/adapt_nway.json)

Exits non-zero unless the kernel's loop is faster than (b) at N = 16, 1-shot."""
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["CWT_ADAPT_PERSIST"] = "0"   # baseline (a); the N-way loop has step launches only
from few_shot_seg_cwt_amd.episode import inner_adapt, inner_adapt_nway  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r8", "adapt_nway.json")
S, ITERS, LR = 473, 200, 0.1
h = (S - 1) // 8 + 1
dev = torch.device("cuda", 0)


def timed(variants):
    """{name: (fn, calls per sample)} -> {name: median / min / max ms per call}.  The variants are
    warmed up, then sampled in alternation (one sample of each per round), so a drift of the clocks
    or of the machine's load falls on all of them alike; a sample is `calls` back-to-back calls
    between two events, so that the short 2-way loop is timed over a window of 10 ms or more."""
    for fn, calls in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in variants}
    for _ in range(reps):
        for k, (fn, calls) in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1) / calls)
    out = {}
    for k, v in ts.items():
        v.sort()
        out[k] = {"median_ms": round(v[len(v) // 2], 3), "min_ms": round(v[0], 3), "max_ms": round(v[-1], 3)}
    return out


def torch_loop(f, lbl, W0, fg, iters):
    N = W0.shape[0]
    cnt = torch.bincount(lbl.view(-1), minlength=256)
    weight = torch.ones(N, device=dev)
    weight[fg] = (cnt[:N].sum() - cnt[fg]) / cnt[fg]
    W = W0.clone().reshape(N, 512, 1, 1).requires_grad_(True)
    opt = torch.optim.SGD([W], lr=LR)
    for _ in range(iters):
        out = F.interpolate(F.conv2d(f, W), size=lbl.shape[-2:], mode="bilinear", align_corners=True)
        loss = F.cross_entropy(out, lbl, weight=weight, ignore_index=255)
        opt.zero_grad()
        loss.backward()
        opt.step()
    return W.detach().reshape(N, 512)


rows = []
g = torch.Generator().manual_seed(2021)
for n in (1, 5):
    f = (0.1 * torch.randn(n, 512, h, h, generator=g)).to(dev).contiguous(memory_format=torch.channels_last)
    for N in (2, 16, 17, 62):
        fg = N - 1
        lbl = torch.randint(0, N, (n, S // 16 + 1, S // 16 + 1), generator=g).repeat_interleave(16, 1).repeat_interleave(
            16, 2)[:, :S, :S].contiguous()
        lbl[torch.rand(n, S, S, generator=g) < 0.05] = 255
        lbl = lbl.to(dev)
        W0 = (0.04 * torch.randn(N, 512, generator=g)).to(dev)
        row = {"shots": n, "S": S, "N": N, "steps": ITERS}
        variants = {"nway": (lambda: inner_adapt_nway(f, lbl, W0.clone(), LR, ITERS, fg), 1),
                    "torch_eager": (lambda: torch_loop(f, lbl, W0, fg, ITERS), 1)}
        if N == 2:
            variants["two_way_steps"] = (lambda: inner_adapt(f, lbl, W0.clone(), LR, ITERS), 10)
        row.update(timed(variants))
        Wk, Wt = inner_adapt_nway(f, lbl, W0.clone(), LR, ITERS, fg), torch_loop(f, lbl, W0, fg, ITERS)
        row["max_abs_diff_vs_torch"] = float((Wk - Wt).abs().max())
        if N == 2:
            row["ratio_to_two_way_steps"] = round(row["nway"]["median_ms"] / row["two_way_steps"]["median_ms"], 3)
        row["speedup_vs_torch"] = round(row["torch_eager"]["median_ms"] / row["nway"]["median_ms"], 2)
        print(json.dumps(row), flush=True)
        rows.append(row)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump({"device": torch.cuda.get_device_name(0), "reps": reps, "rows": rows}, fh, indent=1)
gate = next(r for r in rows if r["shots"] == 1 and r["N"] == 16)
sys.exit(0 if gate["nway"]["median_ms"] < gate["torch_eager"]["median_ms"] else 1)
