#!/usr/bin/env python3
"""Episodes/s of the CWT inference episode (BASELINE.json metric, config #2: PASCAL-shaped
split-0 1-shot ResNet-50, 473x473, batch_size_val = 1, adapt_iter 200, heads 4) on MI355X.

A step = one full episode (test.py:138-219): feature extraction of support + query, the
200-step inner loop, normalize + CWT + classifier, upsample/argmax/IoU/CE for pred_q and
pred_q0.  Inputs (images, labels, W0) are resident in HBM before the timed region.
N GPUs = N independent replicas, episodes sharded by rank (weak scaling, no data-path
collective).

    python bench.py [--gpus N --steps K --warmup W] [--shot 5] [--layers 101 --size 641]

A plain run sets up, warms up, times the K steps and prints the headline result line.
--dump-outputs DIR also writes the last timed step's results as DIR/<name>.npy (the inputs are
seeded, so two builds can be compared output for output).  --full adds every side study to the
line: the sequential leg, the batched pipeline, the exact-fp32 and bf16x3 legs, the per-launch
and roofline records, the inner loop's latency floor and the CPU baseline.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_FP32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: FP32 matrix (= vector) peak
PEAK_BF16_MFMA_TFLOPS = 2516.6  # MI355X_MICROARCH.md: dense bf16 MFMA (no sparsity)
PEAK_HBM_GBPS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
PEAK_X6_TFLOPS = round(PEAK_BF16_MFMA_TFLOPS / 6, 1)   # fp32 width as six bf16 MFMA products
PEAK_X3_TFLOPS = round(PEAK_BF16_MFMA_TFLOPS / 3, 1)   # the bf16x3 approximation's three products
ARITH_X3S, ARITH_F32, ARITH_X6 = 0, 1, 2                # CWT_CONV_ARITH_* (include/cwt.h)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


DUMP_BUDGET_BYTES = 60 << 20   # array bytes; with the .npy headers the files stay under 64 MB (10^6)
DUMP_SAMPLE_SEED = 2021


def dump_outputs(dirname: str, result: dict) -> dict:
    """--dump-outputs: write every tensor of the last timed step's result (what the timed path
    handed its caller) as dirname/<name>.npy, float32 (float64 for float64 and integer tensors),
    DUMP_BUDGET_BYTES in all.  An array larger than its share of the budget is stored as a fixed
    sample: the elements at the sorted flat indices default_rng(DUMP_SAMPLE_SEED).integers(0,
    size, share), the same in every run of the same arguments.  Returns {name: stored shape}."""
    os.makedirs(dirname, exist_ok=True)
    arrs = {}
    for name, t in result.items():
        if not torch.is_tensor(t):
            continue
        t = t.detach()
        wide = t.dtype == torch.float64 or not t.dtype.is_floating_point
        arrs[name] = t.to(torch.float64 if wide else torch.float32).cpu().numpy()
    share = DUMP_BUDGET_BYTES // max(len(arrs), 1)
    shapes = {}
    for name, a in arrs.items():
        if a.nbytes > share:
            idx = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).integers(0, a.size, share // a.itemsize))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(dirname, name + ".npy"), np.ascontiguousarray(a))
        shapes[name] = list(a.shape)
    return shapes


def host_cpu_info() -> dict:
    """The host's CPU facts SURVEY.md §8(d) asks the CPU baseline to state: `nproc` (GNU
    coreutils: the CPUs this process may use, capped by OMP_NUM_THREADS where the launcher sets
    it -- the gpurun box grants 16 per GPU), os.cpu_count() (every CPU of the machine), the CPU
    model and OMP_NUM_THREADS."""
    import subprocess
    try:
        nproc = int(subprocess.run(["nproc"], capture_output=True, text=True, timeout=10).stdout.strip())
    except Exception:
        nproc = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    model = None
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return {"nproc": nproc, "os_cpu_count": os.cpu_count(), "cpu_model": model,
            "OMP_NUM_THREADS": os.environ.get("OMP_NUM_THREADS")}


def cpu_baseline(cfg, sd, tsd, budget_s: float = 25.0, min_eps: int = 5, max_eps: int = 8):
    """The oracle (CPU restatement of the reference path) on the host cores: >= 5 episodes
    after one warm-up, torch.set_num_threads(nproc), bounded by budget_s."""
    from few_shot_seg_cwt_amd import synthetic as syn
    from oracle import cwt_oracle as O
    info = host_cpu_info()
    threads = info["nproc"]
    torch.set_num_threads(threads)
    sdt, tsdt = O.to_torch_state(sd), O.to_torch_state(tsd)
    eps = [syn.make_episode(2021, 100 + i, cfg["image_size"], cfg["shot"]) for i in range(max_eps + 1)]
    W0 = torch.from_numpy(syn.normal(2021, "cpuW0", (2, 512, 1, 1), 0.04))
    O.run_inference_episode(eps[0], sdt, tsdt, W0, cfg)   # warm-up
    t0 = time.time()
    n = 0
    for ep in eps[1:]:
        O.run_inference_episode(ep, sdt, tsdt, W0, cfg)
        n += 1
        if n >= min_eps and time.time() - t0 > budget_s:
            break
    dt = time.time() - t0
    return {"value": n / dt, "unit": "episodes/s", "cores": threads, "kind": "port", **info,
            "sample": f"{n} episodes (after 1 warm-up) of the same workload through oracle/cwt_oracle.py "
                      f"run_inference_episode (torch CPU fp32, torch.set_num_threads(nproc = {threads})); "
                      f"s/episode {dt / n:.2f}"}


def cpu_baseline_train(cfg, sd, tsd, budget_s: float = 25.0, min_eps: int = 5, max_eps: int = 6):
    """The oracle's training episode (inference pieces + CWT loss/gradients + SGD) on the
    host cores: >= 5 episodes after one warm-up, torch.set_num_threads(nproc)."""
    from few_shot_seg_cwt_amd import synthetic as syn
    from oracle import cwt_oracle as O
    info = host_cpu_info()
    threads = info["nproc"]
    torch.set_num_threads(threads)
    sdt, tsdt = O.to_torch_state(sd), O.to_torch_state(tsd)
    classes = syn.coco_val_classes(0) if cfg["layers"] == 101 else None
    eps = [syn.make_episode(2021, 100 + i, cfg["image_size"], cfg["shot"], classes) for i in range(max_eps + 1)]
    W0 = torch.from_numpy(syn.normal(2021, "cpuW0", (2, 512, 1, 1), 0.04))

    def one(ep):
        r = O.run_inference_episode(ep, sdt, tsdt, W0, cfg)
        _, grads, _ = O.cwt_train_step_grads(r["W"], r["f_q"], torch.from_numpy(ep["q_label"]), tsdt, cfg["heads"])
        O.sgd_nesterov(tsdt, grads, {}, 0.001, 0.9, 1e-4)

    one(eps[0])
    t0 = time.time()
    n = 0
    for ep in eps[1:]:
        one(ep)
        n += 1
        if n >= min_eps and time.time() - t0 > budget_s:
            break
    dt = time.time() - t0
    return {"value": n / dt, "unit": "training episodes/s", "cores": threads, "kind": "port", **info,
            "sample": f"{n} training episodes (after 1 warm-up) through oracle/cwt_oracle.py (inference episode + "
                      f"cwt_train_step_grads + sgd_nesterov, torch CPU fp32, {threads} threads); s/episode {dt / n:.2f}"}


def _pmc_summaries():
    import glob
    return sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "pmc_summary.json")),
                  key=lambda p: (int("".join(c for c in p.split(os.sep)[-2][1:3] if c.isdigit()) or 0), p),
                  reverse=True)


def pmc_traffic(dom_name: str):
    """HBM-side bytes per launch of a kernel from the newest committed PMC summary
    (profiles/r*/pmc_summary.json, made by tools/pmc.sh + tools/pmc_summary.py: FETCH_SIZE x 2 +
    WRITE_SIZE, gfx950-corrected).  dom_name: a conv record name "conv_igemm_<kind><bm,bn,stage>"
    or a kernel name prefix (e.g. "adapt_persist_kernel<1").  None if no summary covers it."""
    import re
    mt = re.match(r"conv_igemm_(\w+)<(\d+),(\d+),(\d+)>", dom_name)
    for path in _pmc_summaries():
        for k, e in json.load(open(path)).items():
            if "traffic_bytes" not in e:
                continue
            if mt:
                # kernel names carry <BM, BN, WAVES_M, WAVES_N, NSTG, STAGE, PF>
                kind, bm, bn, stage = mt.group(1), mt.group(2), mt.group(3), mt.group(4)
                if kind in ("x6w", "x6w4"):   # the Winograd forms: their batched GEMM (stage 7 / 8; the bottleneck 6)
                    kind, stage = "x6", ("8" if kind == "x6w4" else "6" if stage == "6" else "7")
                targs = k.split(">(")[0].split("<", 1)[-1].split(", ")
                hit = (f"conv_igemm_{kind}<" in k and len(targs) >= 6 and targs[0] == bm and targs[1] == bn
                       and targs[5] == stage)
            else:
                hit = dom_name in k
            if hit:
                src = os.path.relpath(path, ROOT)
                if mt and mt.group(1).startswith("x6w"):
                    src += " (the Winograd form's batched GEMM launch; its transforms are separate launches)"
                return int(e["traffic_bytes"]), src
    return None, None


def reference_conv_flops(layers: int, S: int) -> float:
    """FLOPs of the reference extractor per image as written (pspnet.py:93-129, resnet.py:57-147):
    every conv once, the bottleneck over the full 4096-channel PPM concat.  323.2 GFLOP for
    R50@473, 837.7 for R101@641."""
    blocks = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3)}[layers]
    conv = lambda H, ci, co, k: 2.0 * H * H * ci * co * k * k  # noqa: E731
    Hs = (S - 1) // 2 + 1
    fl = conv(Hs, 3, 64, 3) + conv(Hs, 64, 64, 3) + conv(Hs, 64, 128, 3)
    H, inp = (Hs - 1) // 2 + 1, 128
    for li, (planes, nb) in enumerate(zip((64, 128, 256, 512), blocks)):
        for b in range(nb):
            Ho = (H - 1) // 2 + 1 if (li == 1 and b == 0) else H
            fl += conv(H, inp, planes, 1) + conv(Ho, planes, planes, 3) + conv(Ho, planes, planes * 4, 1)
            if b == 0:
                fl += conv(Ho, inp, planes * 4, 1)
            inp, H = planes * 4, Ho
    fl += sum(conv(b, 2048, 512, 1) for b in (1, 2, 3, 6)) + conv(H, 4096, 512, 3)
    return fl


def reference_cwt_flops(hw: int, heads: int = 4, C: int = 512) -> float:
    """MultiHeadAttentionOne.forward as written (transformer.py:54-83): q/k/v projections of
    2 + 2*hw tokens through w_qkvs, QK^T and AV for 2 queries, fc, per episode."""
    return 2.0 * (2 + 2 * hw) * C * C * heads + 2.0 * 2 * 2 * hw * C * heads + 2.0 * 2 * C * heads * C


def conv_roofline(fine, peak_tflops):
    """Per-conv roofline of the stack from one episode's per-launch records (profile level 2):
    each conv launch's bound is max(flops / MFMA peak, algorithmic bytes / HBM peak) (bytes =
    input + weights + output [+ residual], each once: 4 B per element for fp32 / the bf16x3
    S-layout, 2 B for the bf16 stack);
    roofline_frac = sum of bounds / sum of measured launch times (1.0 = every conv at its roof).
    The per-launch event pairs cost time BETWEEN the brackets (the level-2 extract bracket is
    ~0.5 ms longer than the level-1 one), not inside them: rocprofv3's kernel durations for the
    same stack sum to within ~4 % of conv_kernel_ms (profiles/r3)."""
    convs = [r for r in fine if r[0].startswith("conv_igemm")]
    if not convs:
        return {}
    roof = t = 0.0
    n_hbm = 0
    for name, fl, by, ms in convs:
        tm, tb = fl / (peak_tflops * 1e12), by / (PEAK_HBM_GBPS * 1e9)
        n_hbm += tb > tm
        roof += max(tm, tb)
        t += ms * 1e-3
    return {"roofline_frac": round(roof / t, 4), "conv_kernel_ms": round(t * 1e3, 4),
            "conv_floor_ms": round(roof * 1e3, 4), "convs": len(convs), "hbm_bound_convs": n_hbm,
            "roofline_basis": f"per conv max(flops/{peak_tflops} TF, bytes/{PEAK_HBM_GBPS / 1e3:.0f} TB/s), "
                              "summed over the stack's conv launches (one episode, per-launch events)"}


def wino_executed(recs, dn, dms, peak):
    """The Winograd bottleneck priced on the work it executes (SURVEY §8(d):
    algebraic shortcuts reported separately from the reference-formulation figure).  The conv's
    record (conv_igemm_x6w...) brackets the input transform, the batched GEMMs and the output
    transform; the library's sub-records (wino_in / wino_gemm / wino_out, api.hip run_wino_conv,
    profile level 3: one extra untimed extraction, whose event pairs do not touch the timed
    brackets) carry the GEMMs' executed FLOPs (2 x P x tiles x Ci x Co: 4/9 of the direct conv at
    F(2x2,3x3)) and the transforms' algorithmic bytes.  recs: that extraction's records, of the
    bottleneck conv (the last Winograd conv of the pass); dn / dms: the timed region's bottleneck
    launches and their summed time."""
    sub = {k: [r for r in recs if r[0].startswith(k + " ")][-1:] for k in ("wino_in", "wino_gemm", "wino_out")}
    if not dn or not all(sub.values()):
        return {}
    n = len(sub["wino_gemm"])
    ms = {k: sum(r[3] for r in v) / len(v) for k, v in sub.items()}
    by = {k: sum(r[2] for r in v) / len(v) for k, v in sub.items()}
    fl_ex = sum(r[1] for r in sub["wino_gemm"]) / n
    launch_ms = dms / dn
    return {"winograd": {
        "form": "F(2x2,3x3): input transform -> 16 batched x6 GEMMs -> output transform (DESIGN.md §3)",
        "flops_executed_per_launch": fl_ex,
        "frac_executed": round(fl_ex / (launch_ms * 1e-3) / 1e12 / peak, 4),
        "frac_executed_note": "the GEMMs' executed FLOPs / the timed region's conv bracket (transforms included) / "
                              "the x6 roof; the parts below from one extra extraction with per-part events",
        "gemm_ms": round(ms["wino_gemm"], 4),
        "gemm_tflops_executed": round(fl_ex / (ms["wino_gemm"] * 1e-3) / 1e12, 2),
        "gemm_frac_executed": round(fl_ex / (ms["wino_gemm"] * 1e-3) / 1e12 / peak, 4),
        "input_transform_ms": round(ms["wino_in"], 4), "input_transform_bytes": round(by["wino_in"]),
        "output_transform_ms": round(ms["wino_out"], 4), "output_transform_bytes": round(by["wino_out"]),
        "transforms_GBps": round((by["wino_in"] + by["wino_out"]) / ((ms["wino_in"] + ms["wino_out"]) * 1e-3) / 1e9, 1),
        "gemm_bytes": round(by["wino_gemm"]),
        "bytes_executed_per_launch": round(by["wino_in"] + by["wino_gemm"] + by["wino_out"]),
        "records": n}}


class adapt_leg:
    """Launch the inner loops of a side leg (timing studies, the exact-fp32 leg) as their own
    instantiation of the persistent kernel (CWT_ADAPT_DBG: 128 = the SIDE instantiation, code
    identical to the product one; 64 = the latency-floor study), so rocprofv3's per-kernel
    statistics of the timed kernel hold only the timed region's launches (and warm-up)."""

    def __init__(self, flags: int):
        self.flags = flags

    def __enter__(self):
        self.old = os.environ.get("CWT_ADAPT_DBG")
        if self.flags:
            os.environ["CWT_ADAPT_DBG"] = str(self.flags)
        return self

    def __exit__(self, *exc):
        if self.flags:
            if self.old is None:
                os.environ.pop("CWT_ADAPT_DBG", None)
            else:
                os.environ["CWT_ADAPT_DBG"] = self.old
        return False


ADAPT_SIDE, ADAPT_FLOOR = 128, 64


def _free_port() -> int:
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def spawn_ranks(n: int) -> int:
    """``bench.py --gpus N`` outside torchrun: start N fresh child processes of this script, one
    per GPU, with the torchrun environment (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*), before
    this parent has touched the GPU (it never does), and return the worst exit code.  Rank 0's
    JSON line reaches stdout through the inherited descriptor."""
    import signal
    import subprocess
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *sys.argv[1:]], env=env))
    codes = [None] * n
    while any(c is None for c in codes):
        for i, p in enumerate(procs):
            if codes[i] is None:
                codes[i] = p.poll()
        bad = [c for c in codes if c not in (None, 0)]
        if bad:   # one rank died: the collective would hang the others
            for i, p in enumerate(procs):
                if codes[i] is None:
                    p.send_signal(signal.SIGTERM)
            for i, p in enumerate(procs):
                if codes[i] is None:
                    try:
                        codes[i] = p.wait(timeout=30)
                    except subprocess.TimeoutExpired:
                        p.kill()
                        codes[i] = p.wait()
            break
        time.sleep(0.2)
    return max((abs(c) for c in codes), default=0)


def cpu_baseline_pretrain(layers, S, nc, budget_s: float = 25.0):
    """The oracle's pretraining iteration (torch CPU fp32 autograd) on a bounded batch."""
    from few_shot_seg_cwt_amd import synthetic as syn
    from oracle.pretrain_oracle import pretrain_step
    info = host_cpu_info()
    threads = info["nproc"]
    torch.set_num_threads(threads)
    sd = {k: torch.from_numpy(np.array(v)) for k, v in syn.make_pspnet_state(layers, 2021, num_classes_tr=nc).items()}
    B = 2
    x = torch.from_numpy(syn.normal(7, "cpu_pt", (B, 3, S, S), 1.0))
    t = torch.from_numpy((syn.uniform01(7, "cpu_pt_l", B * S * S) * nc).astype(np.int64).reshape(B, S, S))
    t0 = time.time()
    n = 0
    while n == 0 or (time.time() - t0 < budget_s and n < 3):
        pretrain_step(sd, x, t, nc, layers)
        n += 1
    dt = time.time() - t0
    return {"value": n * B / dt, "unit": "images/s", "cores": threads, "kind": "port", **info,
            "sample": f"{n} iterations of batch {B} ({S}x{S}, R{layers}, {nc} classes) through "
                      f"oracle/pretrain_oracle.py pretrain_step (torch CPU fp32 autograd, {threads} threads); "
                      f"s/iteration {dt / n:.2f}"}


def main_pretrain(args, dev, rank, world, cdist):
    """Stage-1 pretraining throughput: images/s of whole iterations
    (forward with training BN, loss, backward of every parameter, both SGD groups).  Several
    ranks run independent replicas (the reference's pretrain.py is single-process)."""
    from few_shot_seg_cwt_amd import _lib
    from few_shot_seg_cwt_amd import synthetic as syn
    from few_shot_seg_cwt_amd.pretrain import PretrainPSPNet
    _lib.load_library()
    S, layers, B, nc = args.size, args.layers, args.batch, args.num_classes
    cfg = dict(layers=layers, num_classes_tr=nc, lr=0.0025, scale_lr=2.0, momentum=0.9, weight_decay=1e-4,
               nesterov=True, smoothing=True, dropout=0.1)
    model = PretrainPSPNet(cfg, syn.make_pspnet_state(layers, 2021, num_classes_tr=nc), dev)
    batches = []
    for i in range(2):
        x = torch.from_numpy(syn.normal(100 + rank * 10 + i, "pt_bench", (B, 3, S, S), 1.0)).to(dev)
        # blocky labels: 8x8 regions of one class, 5 % ignored
        lab = (syn.uniform01(200 + rank * 10 + i, "pt_lab", B * ((S + 7) // 8) ** 2) * nc).astype(np.int64)
        lab = np.repeat(np.repeat(lab.reshape(B, (S + 7) // 8, (S + 7) // 8), 8, 1), 8, 2)[:, :S, :S].copy()
        lab[syn.uniform01(300 + i, "pt_ign", B * S * S).reshape(B, S, S) < 0.05] = 255
        batches.append((x, torch.from_numpy(lab).to(dev)))
    for i in range(args.warmup):
        model.train_step(*batches[i % 2], lr=0.0025)
    torch.cuda.synchronize()
    cdist.barrier()
    torch.cuda.synchronize()
    st = torch.cuda.current_stream(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(st)
    losses = [model.train_step(*batches[i % 2], lr=0.0025) for i in range(args.steps)]
    e1.record(st)
    torch.cuda.synchronize()
    cdist.barrier()
    dt = cdist.all_reduce_max_scalar(time.perf_counter() - t0)
    ev_ms = e0.elapsed_time(e1) / args.steps
    flops_step = 3.0 * reference_conv_flops(layers, S) * B   # conv forward + input gradient + weight gradient
    achieved = flops_step / (ev_ms * 1e-3) / 1e12
    out = {
        "metric": f"pretraining images/sec ({S}x{S}, R{layers} PSPNet, batch {B}, {nc} classes)",
        "value": round(world * args.steps * B / dt, 3),
        "unit": "images/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(dt / args.steps * 1e3, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "fp32 (exact f32 MFMA for every conv forward / input gradient / weight gradient)",
        "data": "synthetic (PRNG weights, PRNG images, blocky PRNG labels)",
        "config": {"workload": "stage-1 pretraining iteration (pretrain.py:104-121): model.train(), PSPNet "
                               "forward, label-smoothed CE, backward of every parameter, SGD nesterov two groups",
                   "image_size": S, "layers": layers, "batch": B, "num_classes_tr": nc,
                   "parallelism": f"{world} independent replicas"},
        "roofline": {"bound": "mfma", "kernel": "whole iteration (conv fwd + dgrad + wgrad FLOPs of the reference "
                                                "formulation; PPM / BN / loss kernels in the time)",
                     "achieved": round(achieved, 2), "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s",
                     "frac": round(achieved / PEAK_FP32_MFMA_TFLOPS, 4), "traffic": None,
                     "flops_per_step": flops_step, "event_ms_per_step": round(ev_ms, 3)},
        "loss_last": round(float(losses[-1]), 5),
    }
    if rank == 0 and args.dump_outputs:
        out["dumped_outputs"] = dump_outputs(args.dump_outputs, {"loss": losses[-1]})
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline_pretrain(layers, S, nc)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


def make_after(flat, opt, cdist, on_step=None):
    """The training step's exchange point, run after each episode's CWT backward (SURVEY.md
    §8(e); train.py:248-251 under DDP): the mean all-reduce of the flat gradient bucket over the
    ranks, the identical SGD step everywhere, the gradient cleared.  on_step(flat) observes the
    replica after each step (the CPU stand-in's digest)."""
    def after():
        cdist.all_reduce_mean_(flat.grad)
        opt.step()
        flat.grad.zero_()
        if on_step is not None:
            on_step(flat)
    return after


def timed_region(run_steps, sync, cdist):
    """barrier + sync on both sides of the K timed steps; the max over ranks of the wall time."""
    cdist.barrier()
    sync()
    t0 = time.perf_counter()
    out = run_steps()
    sync()
    cdist.barrier()
    return cdist.all_reduce_max_scalar(time.perf_counter() - t0), out


class CpuStandinTrainEngine:
    """Test hook (CWT_BENCH_CPU_STANDIN=1, tests/test_bench_launch.py): the --train step's episode
    replaced by a seeded CPU stand-in, so bench.py's own multi-rank path (process group, per-rank
    episodes, make_after's all-reduce + SGD, timed_region's max-over-ranks clock, the JSON line)
    runs under gloo without a device.  The stand-in's gradient depends on the rank's episode and
    on the current parameters, as the real CWT gradient does."""

    def __init__(self, flat: torch.Tensor):
        self.flat = flat

    def step(self, seed: int):
        g = torch.Generator().manual_seed(seed)
        noise = torch.randn(self.flat.shape, generator=g)
        with torch.no_grad():
            self.flat.grad = 0.01 * self.flat.detach() + noise
        return {"loss": torch.tensor(float(noise[:64].square().mean()))}


def main_cpu_standin(args, rank, world, cdist):
    """bench.py --train on the CPU stand-in episode (see CpuStandinTrainEngine)."""
    import hashlib
    if not args.train:
        raise SystemExit("CWT_BENCH_CPU_STANDIN covers --train only")
    n = 4 * 512 * 512 + 4 * 512 + 2 * 512   # a CWT-sized flat bucket (w_qkvs + layer norm + fc, H = 4)
    flat = torch.zeros(n).uniform_(-0.05, 0.05, generator=torch.Generator().manual_seed(2021 + rank))
    flat.requires_grad_(True)
    cdist.broadcast_params_(flat)                 # DDP's start-of-training broadcast
    opt = torch.optim.SGD([flat], lr=0.0025, momentum=0.9, weight_decay=1e-4, nesterov=True)
    digests = []
    after = make_after(flat, opt, cdist, lambda f: digests.append(
        hashlib.sha256(f.detach().numpy().tobytes()).hexdigest()[:16]))
    eng = CpuStandinTrainEngine(flat)

    def step(i):
        r = eng.step(rank * 1000 + i)   # each rank its own episodes
        after()
        return r["loss"]

    for i in range(args.warmup):
        step(i)
    dt, losses = timed_region(lambda: [step(args.warmup + i) for i in range(args.steps)], lambda: None, cdist)
    print(json.dumps({"rank": rank, "digests": digests, "dt_max": dt}), flush=True)
    if rank == 0:
        print(json.dumps({"metric": f"training episodes/sec ({args.size}x{args.size}, {args.shot}-shot, "
                                    f"R{args.layers}) [CPU stand-in episode]",
                          "value": round(world * args.steps / dt, 6), "unit": "training episodes/s",
                          "n_gpus": cdist.rank_world()[1], "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(dt / args.steps * 1e3, 6), "data": "cpu stand-in (test hook)",
                          "loss_last": float(losses[-1])}), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shot", type=int, default=1)
    ap.add_argument("--layers", type=int, default=50)
    ap.add_argument("--size", type=int, default=473)
    ap.add_argument("--pool", type=int, default=4, help="distinct resident episodes cycled through")
    ap.add_argument("--inflight", type=int, default=1,
                    help="independent episodes processed together per step (EpisodeEngine.run_batch, <= 16)")
    ap.add_argument("--pipeline", type=int, default=2,
                    help="EpisodePipeline with this many extractor streams (0: one episode after the other): the "
                         "next episodes' extractor passes overlap the current episode's inner loop; every "
                         "episode is still processed alone (batch 1), by the same kernels")
    ap.add_argument("--conv-dtype", default="fp32", choices=["fp32", "bf16"],
                    help="conv-stack arithmetic: fp32 (reference numerics) or bf16 (config #5)")
    ap.add_argument("--train", action="store_true",
                    help="training episodes (do_epoch step: inner loop, CWT fwd/bwd, RCCL gradient all-reduce, SGD); "
                         "BASELINE config #4 is --train --layers 101 --size 641")
    ap.add_argument("--pretrain", action="store_true",
                    help="stage-1 pretraining iterations (pretrain.py:104-121: whole-PSPNet forward + backward + "
                         "SGD, training BN, label-smoothed CE), batch --batch of --size images, --num-classes")
    ap.add_argument("--batch", type=int, default=10, help="--pretrain: images per iteration (pascal_pretrain.yaml: 10)")
    ap.add_argument("--num-classes", type=int, default=16, help="--pretrain: num_classes_tr (16 PASCAL, 61 COCO)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--exact-steps", type=int, default=20,
                    help="episodes of the exact-fp32 conv leg (cwt_ctx_set_conv_arith F32 on every extractor "
                         "context; through the same episode pipeline as the headline, and sequential); 0 = skip")
    ap.add_argument("--x3-steps", type=int, default=20,
                    help="episodes of the bf16x3 leg (the declared ~16-bit-operand approximation, "
                         "cwt_ctx_set_conv_arith BF16X3; pipelined); 0 = skip")
    ap.add_argument("--pair-steps", type=int, default=20,
                    help="steps of the batched-pipeline leg (two episodes share one extractor pass, "
                         "EpisodePipeline.submit_batch; reported beside the headline); 0 = skip")
    ap.add_argument("--profile-json", default=None, help="write per-launch records here (rank 0; needs --full)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run every side study (the sequential leg, the batched "
                         "pipeline, the exact-fp32 and bf16x3 legs, per-launch and roofline records, the latency "
                         "floor, the CPU baseline) and report them in the result line; a plain run sets up, warms "
                         "up, times the steps and prints the headline fields only")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps write what the last timed step returned to its caller as "
                         "DIR/<name>.npy (float32 / float64, rank 0)")
    args = ap.parse_args()
    if args.profile_json and not args.full:
        ap.error("--profile-json holds the per-launch records of --full's extra episodes: add --full")

    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        ngpu = torch.cuda.device_count()     # does not initialise the GPU
        if 0 < ngpu < args.gpus:
            raise SystemExit(f"--gpus {args.gpus} but only {ngpu} GPUs are visible")
        sys.exit(spawn_ranks(args.gpus))
    if env_world is not None and int(env_world) != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} disagrees with WORLD_SIZE={env_world} from the launcher")

    from few_shot_seg_cwt_amd import dist as cdist
    rank, local, world = cdist.init_from_env()
    if world != args.gpus:
        raise SystemExit(f"process group has {world} ranks, --gpus asks for {args.gpus}")
    if os.environ.get("CWT_BENCH_CPU_STANDIN") == "1":   # multi-rank path without a device (tests)
        return main_cpu_standin(args, rank, world, cdist)
    if os.environ.get("CWT_BENCH_DRYRUN"):   # launch check without a device (tests/test_bench_launch.py)
        tot = cdist.all_reduce_sum_np(np.array([1.0]))[0]
        print(json.dumps({"rank": rank, "world": world, "ranks_seen": int(tot)}), flush=True)
        if world > 1:
            torch.distributed.destroy_process_group()
        return
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if args.pretrain:
        return main_pretrain(args, dev, rank, world, cdist)

    from few_shot_seg_cwt_amd import MultiHeadAttentionOne, _lib, get_model
    from few_shot_seg_cwt_amd import synthetic as syn
    from few_shot_seg_cwt_amd.episode import EpisodeEngine, EpisodePipeline, TrainEngine
    from few_shot_seg_cwt_amd.optimizer import get_optimizer

    _lib.load_library()
    S, shot, layers = args.size, args.shot, args.layers
    cfg = syn.cfg_defaults(image_size=S, shot=shot, layers=layers, conv_dtype=args.conv_dtype)
    seed = 2021
    sd = syn.make_pspnet_state(layers, seed)
    tsd = syn.make_transformer_state(4, 512, seed)
    model = get_model(cfg)
    model.load_state_dict(sd)
    trans = MultiHeadAttentionOne(4, 512, 512, 512, dropout=0.5)
    trans.load_state_dict(tsd)
    engine = EpisodeEngine(model, trans, cfg)
    if args.inflight != 1:
        args.pipeline = 0   # the batched throughput mode runs its E episodes in one pass
    pipe = EpisodePipeline(engine, extract_streams=args.pipeline) if args.pipeline else None
    if args.train and args.inflight != 1:
        raise SystemExit("--train runs one episode per rank per step (train.py batch_size 1)")
    if args.train:
        tengine = TrainEngine(model, trans, cfg)
        cdist.broadcast_params_(trans.flat)          # DDP's start-of-training broadcast
        opt = get_optimizer(cfg, [dict(params=[trans.flat], lr=cfg["trans_lr"] * cfg["scale_lr"])])

    # resident inputs: a pool of distinct episodes per rank + one W0 buffer per step
    classes = syn.coco_val_classes(0) if layers == 101 else None
    E = args.inflight
    pool = []
    for i in range(args.pool):
        eps = [syn.make_episode(seed, rank * 1000 + i * E + e, S, shot, classes) for e in range(E)]
        imgs = torch.from_numpy(np.concatenate([ep["spprt_imgs"][0] for ep in eps] + [ep["qry_img"] for ep in eps]))
        sl = torch.from_numpy(np.stack([ep["s_label"][0] for ep in eps]))
        ql = torch.from_numpy(np.concatenate([ep["q_label"] for ep in eps]))
        pool.append((imgs.to(dev), sl.to(dev), ql.to(dev)))
    g = torch.Generator().manual_seed(seed + rank)
    nW = args.warmup + args.steps
    bound = 1.0 / np.sqrt(512)
    W0 = ((torch.rand((nW, E, 2, 512), generator=g) * 2 - 1) * bound).to(dev)
    torch.cuda.synchronize()
    newest = {}   # "result": what the newest step handed its caller (--dump-outputs reads the last timed one)

    def step(i: int, Wbuf, last: bool = False):
        imgs, sl, ql = pool[i % len(pool)]
        if args.train:   # do_epoch iteration (train.py:188-267 + the all-reduce point of SURVEY §8(e))
            after = make_after(trans.flat, opt, cdist)
            if pipe is not None:
                r = pipe.submit_train(tengine, imgs, sl[0], ql, Wbuf[0], after)
            else:
                r = tengine.step(imgs, sl[0], ql, Wbuf[0])
                after()
            newest["result"] = r
            return r["loss"].view(1, 1, 1).expand(1, 2, 2)
        if pipe is not None:
            r = pipe.submit(imgs, sl[0], ql, Wbuf[0], last=last)
        elif E == 1:
            r = engine.run(imgs, sl[0], ql, Wbuf[0])
        else:
            r = engine.run_batch(imgs, sl, ql, Wbuf)
        newest["result"] = r
        return r["iut"]

    # warm-up runs exactly the timed loop's code (lazy kernel loading, graph capture, workspaces)
    warm_iut = [step(s, W0[s], last=s == args.warmup - 1) for s in range(args.warmup)]
    if pipe is not None:
        pipe.wait()
    torch.cat(warm_iut).sum(0)
    torch.cuda.synchronize()

    _lib.profile_enable(1)   # coarse: phases + bottleneck conv (no per-launch event gaps)
    t_marks = {}

    def run_steps():
        t_marks["t0"] = time.perf_counter()
        out = [step(s, W0[args.warmup + s], last=s == args.steps - 1) for s in range(args.steps)]
        t_marks["sub"] = time.perf_counter()   # the host has enqueued every step (host-boundness diagnostic)
        if pipe is not None:
            pipe.wait()
        return out

    dt, iuts = timed_region(run_steps, torch.cuda.synchronize, cdist)
    t0, t_sub = t_marks["t0"], t_marks["sub"]
    value = world * args.steps * E / dt
    seq = None
    recs = _lib.profile_records()
    _lib.profile_enable(0)
    dom = [r for r in recs if r[0].startswith("conv_igemm")]     # the bottleneck conv (level 1 records only it)
    dom_name = dom[0][0].split(" ")[0] if dom else "n/a"
    conv_x3 = dom_name.startswith("conv_igemm_bf16x3") or dom_name.startswith("conv_igemm_x3s")
    conv_x6 = dom_name.startswith("conv_igemm_x6")
    conv_b16 = dom_name.startswith("conv_igemm_b16")
    iu = torch.cat(iuts).sum(0)
    head = {
        "metric": (f"training episodes/sec ({S}x{S}, {shot}-shot, R{layers})" if args.train else
                   "episodes/sec (473x473, 1-shot, R50) at 1/2/4/8 MI355X; mIoU vs ref"
                   if (S, shot, layers) == (473, 1, 50) else f"episodes/sec ({S}x{S}, {shot}-shot, R{layers})")
        + (" [bf16 conv stack]" if args.conv_dtype == "bf16" else ""),
        "value": round(value, 3),
        "unit": "training episodes/s" if args.train else "episodes/s",
        "n_gpus": cdist.rank_world()[1],
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(dt / args.steps * 1e3, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": ("fp32 (conv stack at fp32 width on the bf16 MFMA: every fp32 operand split exactly into bf16 "
                  "hi + mid + lo, the six products >= 2^-24 |a||b| summed in fp32; inner loop, CWT, classifier "
                  "fp32)") if conv_x6
        else "fp32 (conv stack: bf16x3 split-fp32 on bf16 MFMA, ~16-bit operands)" if conv_x3
        else "bf16 conv stack (fp32 accumulate) + fp32 inner loop / CWT / classifier" if conv_b16 else "fp32",
        "data": "synthetic (PRNG weights + PASCAL-shaped episodes, few_shot_seg_cwt_amd/synthetic.py)",
        "config": {"workload": (f"CWT training episode (do_epoch, batch_size=1, RCCL mean all-reduce of the "
                                f"8.39 MB gradient bucket + nesterov SGD per step): " if args.train else
                                f"CWT inference episode (validate_transformer, batch_size_val=1): ") +
                               f"{'PASCAL split-0' if layers == 50 else 'COCO-20i split-0'} {shot}-shot "
                               f"ResNet-{layers} PSPNet {S}x{S}, adapt_iter 200, heads 4",
                   "image_size": S, "shot": shot, "layers": layers, "episodes_per_step_per_gpu": E,
                   "parallelism": f"{world} episode-sharded replicas" + (f", {E} episodes in flight per GPU" if E > 1 else "")
                   + (f", episode pipeline ({args.pipeline} extractor stream(s) beside the inner-loop / CWT stream: "
                      "episode i+1's extractor pass overlaps episode i's inner loop, each episode alone)"
                      if pipe is not None else "")},
        "iou_fg_timed": None if args.train else round(float((iu[0, 1] / iu[1, 1].clamp_min(1)).item()), 4),
        "host_submit_ms_per_step": round((t_sub - t0) / args.steps * 1e3, 3),
        "full": args.full,
    }
    if rank == 0 and args.dump_outputs:   # before any other leg reuses the workspaces behind these tensors
        head["dumped_outputs"] = dump_outputs(args.dump_outputs, newest["result"])
    if not args.full:   # a plain run: the headline alone (the side studies and the CPU baseline: --full)
        _lib.check_status()   # every launch has completed: surface an inner-loop barrier timeout
        if rank == 0:
            print(json.dumps(head), flush=True)
        if world > 1:
            torch.distributed.destroy_process_group()
        return
    seq_recs = None
    if pipe is not None:   # the same episodes one after the other on one stream (no overlap), same run
        pipe_saved, pipe = pipe, None
        _lib.profile_enable(1)
        cdist.barrier()
        torch.cuda.synchronize()
        ts0 = time.perf_counter()
        seq_out = [step(s, W0[args.warmup + s]) for s in range(args.steps)]
        torch.cuda.synchronize()
        cdist.barrier()
        dts = cdist.all_reduce_max_scalar(time.perf_counter() - ts0)
        seq_recs = _lib.profile_records()
        _lib.profile_enable(0)
        seq = {"value": round(world * args.steps / dts, 3), "ms_per_step": round(dts / args.steps * 1e3, 3),
               "note": "the same K steps one episode after the other on one stream (--pipeline 0)"}
        del seq_out
        pipe = pipe_saved
    # ---- batched pipeline: two episodes per extractor pass (M = 4*h*w
    # rows per conv at 1-shot), their inner loops in one persistent launch, tails batched; the
    # same pipeline and streams.  A throughput form reported beside the headline, not in it ----
    pairs = None
    if pipe is not None and not args.train and E == 1 and args.pair_steps > 0:
        EP = 2
        pool2 = []
        for i in range(2):
            eps = [syn.make_episode(seed, rank * 1000 + 500 + i * EP + e, S, shot, classes) for e in range(EP)]
            imgs = torch.from_numpy(np.concatenate([ep["spprt_imgs"][0] for ep in eps] + [ep["qry_img"] for ep in eps]))
            sl = torch.from_numpy(np.stack([ep["s_label"][0] for ep in eps]))
            ql = torch.from_numpy(np.concatenate([ep["q_label"] for ep in eps]))
            pool2.append((imgs.to(dev), sl.to(dev), ql.to(dev)))
        P = args.pair_steps
        W02 = ((torch.rand((P + 2, EP, 2, 512), generator=g) * 2 - 1) * bound).to(dev)
        with adapt_leg(ADAPT_SIDE):
            for s_ in range(2):
                im, sl_, ql_ = pool2[s_ % 2]
                pipe.submit_batch(im, sl_, ql_, W02[s_].clone(), last=s_ == 1)
            pipe.wait()
            torch.cuda.synchronize()
            _lib.profile_enable(1)
            cdist.barrier()
            torch.cuda.synchronize()
            tp0 = time.perf_counter()
            pouts = [pipe.submit_batch(pool2[s_ % 2][0], pool2[s_ % 2][1], pool2[s_ % 2][2], W02[2 + s_],
                                       last=s_ == P - 1)["iut"] for s_ in range(P)]
            pipe.wait()
            torch.cuda.synchronize()
            cdist.barrier()
            dtp = cdist.all_reduce_max_scalar(time.perf_counter() - tp0)
            precs = _lib.profile_records()
            _lib.profile_enable(2)
            model.extract_features(pool2[0][0])
            torch.cuda.synchronize()
            pfine = _lib.profile_records()
            _lib.profile_enable(0)
        pex = [r for r in precs if r[0].startswith("extract_features")]
        pairs = {"value": round(world * P * EP / dtp, 3), "unit": "episodes/s", "steps": P, "episodes_per_step": EP,
                 "ms_per_episode": round(dtp / (P * EP) * 1e3, 3),
                 "mode": "EpisodePipeline.submit_batch: two episodes' support + query images in ONE extractor pass "
                         f"({EP * (shot + 1)} images, conv GEMM rows M = {EP * (shot + 1)}*h*w), their inner loops "
                         "in one persistent launch, the fused tails batched; exact per episode (eval-mode BN)",
                 "extract_ms_per_step": round(sum(r[3] for r in pex) / P, 3),
                 "conv_stack": {"note": f"one {EP * (shot + 1)}-image extractor pass alone, per-launch records",
                                **conv_roofline(pfine, PEAK_BF16_MFMA_TFLOPS if args.conv_dtype == "bf16"
                                                else PEAK_X6_TFLOPS)}}
        del pouts

    def total(prefix):
        sel = [r for r in recs if r[0].startswith(prefix)]
        return len(sel), sum(r[1] for r in sel), sum(r[3] for r in sel)

    n_ex, ex_fl, ex_ms = total("extract_features")
    n_ad, _, ad_ms = total("inner_adapt x")      # the phase bracket (label prep + setup + the loop)
    ad_bytes = sum(r[2] for r in recs if r[0].startswith("inner_adapt x"))
    n_at, _, at_ms = total("attention")       # the module-by-module CWT (CWT_FUSED_TAIL=0)
    n_tl, _, tl_ms = total("post_loop_tail")  # the one-launch tail (CWT + classifier + metrics)
    n_tk, _, tk_ms = total("episode_tail_kernel")
    tk_sel = [r for r in recs if r[0].startswith("episode_tail_kernel")]
    dn, dfl, dms = len(dom), sum(r[1] for r in dom), sum(r[3] for r in dom)
    achieved = (dfl / dn) / (dms / dn * 1e-3) / 1e12
    if conv_x6:   # fp32 width as 6 bf16 MFMA products: the roof is the dense bf16 rate / 6
        peak, peak_basis = PEAK_X6_TFLOPS, "bf16x6: 2516.6 TF dense bf16 MFMA / 6 products"
    elif conv_x3:   # fp32 GEMM done as 3 bf16 MFMA products: the roof is the dense bf16 rate / 3
        peak, peak_basis = round(PEAK_BF16_MFMA_TFLOPS / 3, 1), "bf16x3: 2516.6 TF dense bf16 MFMA / 3 products"
    elif conv_b16:
        peak, peak_basis = PEAK_BF16_MFMA_TFLOPS, "dense bf16 MFMA 2516.6 TF"
    else:
        peak, peak_basis = PEAK_FP32_MFMA_TFLOPS, "fp32 MFMA 157.3 TF"

    traffic, traffic_src = pmc_traffic(dom_name)
    # the inner loop (one persistent launch per episode group; the bracket also holds the label
    # prep and setup kernels): algorithmic bytes per launch = 200 x n x (f_s + labels), SURVEY.md §8(d)
    # the instantiation the timed region ran (the record name carries it: "inner_adapt x200 [adapt_persist_kernel<2]");
    # with the pipeline's drain the burst's last loop runs the whole-chip geometry: the roofline
    # figures are over the launches of the named (majority) instantiation
    # roofline: the persistent kernel's own launches ("inner_adapt_kernel [...]" records: the
    # kernel alone, as rocprofv3 times it), else the phase bracket
    kpref = "inner_adapt_kernel [" if any(r[0].startswith("inner_adapt_kernel [") for r in recs) else "inner_adapt x"
    ad_names = [r[0] for r in recs if r[0].startswith(kpref) and "[" in r[0]]
    ad_kernel = (max(set(ad_names), key=ad_names.count).split("[", 1)[1].rstrip("]") if ad_names
                 else "adapt_persist_kernel<")
    ad_sel = [r for r in recs if r[0].startswith(kpref) and (not ad_names or ad_kernel + "]" in r[0])]
    ad_launches = max(len(ad_sel), 1)
    ad_bytes_launch = sum(r[2] for r in ad_sel) / ad_launches
    ad_ms_launch = sum(r[3] for r in ad_sel) / ad_launches
    ad_achieved = ad_bytes_launch / (ad_ms_launch * 1e-3) / 1e9 if ad_ms_launch else 0.0
    seq_ad = None
    if seq_recs:
        s_sel = [r for r in seq_recs if r[0].startswith(kpref)]
        if s_sel:
            s_ms = sum(r[3] for r in s_sel) / len(s_sel)
            s_by = sum(r[2] for r in s_sel) / len(s_sel)
            s_name = s_sel[0][0].split("[", 1)[1].rstrip("]") if "[" in s_sel[0][0] else "?"
            seq_ad = {"kernel": s_name + ", ...>", "avg_launch_ms": round(s_ms, 4),
                      "achieved": round(s_by / (s_ms * 1e-3) / 1e9, 1),
                      "frac": round(s_by / (s_ms * 1e-3) / 1e9 / PEAK_HBM_GBPS, 4),
                      "note": "the same inner loop in the sequential leg (no extractor pass beside it; "
                              "default geometry)"}
    ad_traffic, ad_traffic_src = pmc_traffic(ad_kernel)
    h_feat = (S - 1) // 8 + 1
    images = (shot + 1) * E
    ref_ex_fl = reference_conv_flops(layers, S) * images * args.steps

    # per-launch table from one extra (untimed) episode at profile level 2
    _lib.profile_enable(2)
    with adapt_leg(ADAPT_SIDE):
        step(0, W0[0].clone())
        if pipe is not None:
            pipe.wait()
        torch.cuda.synchronize()
    fine = _lib.profile_records()
    # the Winograd conv's parts (input transform, batched GEMMs, output transform): profile level 3,
    # one untimed extraction
    _lib.profile_enable(3)
    model.extract_features(pool[0][0])
    torch.cuda.synchronize()
    wino_recs = _lib.profile_records()
    _lib.profile_enable(0)
    _lib.check_status()   # every launch so far has completed: surface an inner-loop barrier timeout

    # ---- the inner loop's latency floor: the same persistent kernel at the
    # same G with every unit's arithmetic and atomics skipped (CWT_ADAPT_DBG & 64) -- the per-step
    # exchange alone (slot zeroing, arrival, poll, replica reads, W update) x adapt_iter ----
    latency_floor = None
    if not args.train and E == 1 and ad_kernel.startswith("adapt_persist"):   # (also the fused loop + tail)
        imgs0, sl0, ql0 = pool[0]
        with torch.no_grad():
            f_s0 = model.extract_features(imgs0)[0][:shot]
        from few_shot_seg_cwt_amd.episode import inner_adapt

        def time_loop(ctx_sel, dbg, reps=5):
            """median of the persistent kernel's own bracket (inner_adapt_kernel records, as the
            timed region's roofline uses) over reps launches after one warm-up"""
            with adapt_leg(dbg):
                _lib.profile_enable(1)
                for r in range(reps + 1):
                    if ctx_sel is None:
                        inner_adapt(f_s0, sl0[0], W0[0, 0].clone(), cfg["cls_lr"], cfg["adapt_iter"])
                    else:
                        with _lib.using_ctx(ctx_sel):
                            inner_adapt(f_s0, sl0[0], W0[0, 0].clone(), cfg["cls_lr"], cfg["adapt_iter"])
                torch.cuda.synchronize()
                ks = [r[3] for r in _lib.profile_records() if r[0].startswith(kpref)]
                _lib.profile_enable(0)
            return float(np.median(ks[1:]))

        geos = [("sequential_leg (default context)", None)]
        if pipe is not None:
            geos.insert(0, ("timed region's geometry (the pipeline's adapt context)", pipe.c_adapt))
        latency_floor = {"basis": "the same persistent kernel at the same G, alone on the GPU (its own launch "
                                  "bracket, as the timed roofline's), with every unit's "
                                  "arithmetic and atomics skipped (CWT_ADAPT_DBG & 64, the FLOOR instantiation "
                                  "adapt_persist_kernel<NRES, 2>; the 'alone' runs beside it are the SIDE "
                                  "instantiation <NRES, 3>, code identical to the timed one): the per-step exchange "
                                  "(slot zeroing, arrival, poll, replica reads, W update) x adapt_iter -- the "
                                  "loop's dependency-chain floor in this design"}
        bytes_floor_ms = ad_bytes_launch / (PEAK_HBM_GBPS * 1e9) * 1e3
        for label, c in geos:
            full = time_loop(c, ADAPT_SIDE)
            floor = time_loop(c, ADAPT_FLOOR)
            latency_floor[label.split(" ")[0]] = {"what": label, "floor_ms": round(floor, 4),
                                                  "alone_ms": round(full, 4),
                                                  "frac_alone_vs_floor": round(max(floor, bytes_floor_ms) / full, 4)}
        lf = latency_floor[geos[0][0].split(" ")[0]]
        latency_floor["bytes_floor_ms"] = round(bytes_floor_ms, 4)
        latency_floor["frac"] = round(max(lf["floor_ms"], bytes_floor_ms) / ad_ms_launch, 4)
        latency_floor["frac_note"] = ("max(bytes floor, latency floor) / the timed region's average launch: how "
                                      "close the measured loop is to ITS floor (the byte frac above prices it as "
                                      "a bandwidth kernel, which it is not)")
        _lib.check_status()

    # ---- the post-loop tail: normalize + pred_q0 + CWT + classifier + both
    # metrics in one launch, priced as the HBM pass it is (algorithmic bytes: f_q read for the
    # norms and again for the CWT / classifier, the CWT weights once, labels + 8-B IoU traffic per
    # pixel) beside the reference formulation's FLOPs (transformer.py:54-83 as written) ----
    tail_roofline = None
    if tk_sel:
        tk_launch_ms = sum(r[3] for r in tk_sel) / len(tk_sel)
        tk_bytes = sum(r[2] for r in tk_sel) / len(tk_sel)
        hw_ = h_feat * h_feat
        exec_fl = E * (2.0 * 2 * 4 * hw_ * 512 * 2 + 2.0 * 2 * hw_ * 512 * 2)   # scores + A.f per head, 2 classifiers
        ref_fl = reference_cwt_flops(hw_) * E
        fused_tail = "tail_kernel" in ad_kernel   # the tail fused behind the loop (cwt_inner_adapt_tail)
        if fused_tail:   # the fused launch's PMC minus the same loop alone (the SIDE instantiation, same code)
            t_f, src_f = pmc_traffic("adapt_persist_tail_kernel<5")
            t_l, _ = pmc_traffic("adapt_persist_kernel<5, 3>")
            tk_traffic = t_f - t_l if t_f is not None and t_l is not None else None
            tk_traffic_src = (src_f + " (adapt_persist_tail_kernel<5> minus adapt_persist_kernel<5, 3>: the fused "
                              "launch less the same loop alone)") if tk_traffic is not None else None
        else:
            tk_traffic, tk_traffic_src = pmc_traffic("episode_tail_kernel")
        tail_roofline = {
            "bound": "hbm",
            "kernel": ("the tail part of adapt_persist_tail_kernel<5> (cwt_inner_adapt_tail: the episode tail fused "
                       "behind the inner loop's last step; its time from in-kernel realtime stamps, the last "
                       "workgroup's loop end to the last workgroup's tail end)" if fused_tail else
                       "episode_tail_kernel (cwt_episode_tail, one launch per episode)"),
            "avg_launch_ms": round(tk_launch_ms, 4), "launches": len(tk_sel),
            "algorithmic_bytes_per_launch": round(tk_bytes),
            "achieved": round(tk_bytes / (tk_launch_ms * 1e-3) / 1e9, 1), "peak": PEAK_HBM_GBPS, "unit": "GB/s",
            "frac": round(tk_bytes / (tk_launch_ms * 1e-3) / 1e9 / PEAK_HBM_GBPS, 4),
            "traffic": tk_traffic, "traffic_unit": "bytes/launch",
            "traffic_source": tk_traffic_src,
            "executed_flops_per_launch": exec_fl,
            "reference_formulation_flops_per_launch": ref_fl,
            "reference_formulation_tflops": round(ref_fl / (tk_launch_ms * 1e-3) / 1e12, 2),
            "reference_formulation_frac_of_fp32_mfma": round(ref_fl / (tk_launch_ms * 1e-3) / 1e12
                                                             / PEAK_FP32_MFMA_TFLOPS, 4),
            "measured_in": ("the timed region (pipelined: run by the inner loop's resident workgroups behind its "
                            "last grid barrier, no launch and no wait for CUs)" if fused_tail else
                            "the timed region (pipelined: launched on the adapt stream while the next episodes' "
                            "extractor passes hold most CUs)"),
            "note": "the CWT runs re-associated (DESIGN.md §3): scores = f . (W_k^T q') and W_v (sum_j a_j f_j) -- "
                    "token work of ~59 MFLOP instead of projecting every token (15.1 GFLOP as written); the kernel "
                    "is latency-bound (grid barriers between its phases), so both fractions are small"}

    # ---- other conv arithmetics through the same episodes and pipeline (cwt_ctx_set_conv_arith on
    # every extractor context): exact_fp32 = v_mfma_f32 (157.3 TF roof), bf16x3 = the declared
    # approximation (16-bit operands, 838.9 TF roof); the headline's own arithmetic is x6 ----
    ext_ctxs = [_lib.ctx(dev.index)] + ([c for c in pipe.c_ext if c is not None] if pipe is not None else [])

    def set_arith(v):
        for c in ext_ctxs:
            _lib.check(_lib.lib().cwt_ctx_set_conv_arith(c, v), "cwt_ctx_set_conv_arith")

    def arith_leg(arith, nx, peak_leg, modes, what):
        set_arith(arith)
        try:
            with adapt_leg(ADAPT_SIDE):
                # warm-up: this arithmetic's plans and workspaces, both paths
                for s_ in range(3):
                    im, sl_, ql_ = pool[s_ % len(pool)]
                    if pipe is not None:
                        pipe.submit(im, sl_[0], ql_, W0[s_, 0].clone(), last=s_ == 2)
                    else:
                        engine.run(im, sl_[0], ql_, W0[s_, 0].clone())
                if pipe is not None:
                    pipe.wait()
                torch.cuda.synchronize()
                legs = {}
                for mode in modes if pipe is not None else ("sequential",):
                    _lib.profile_enable(1)
                    cdist.barrier()
                    torch.cuda.synchronize()
                    tf0 = time.perf_counter()
                    outs = []
                    for s_ in range(nx):
                        im, sl_, ql_ = pool[s_ % len(pool)]
                        w_ = W0[args.warmup + s_ % args.steps, 0].clone()
                        if mode == "pipelined":
                            outs.append(pipe.submit(im, sl_[0], ql_, w_, last=s_ == nx - 1)["iut"])
                        else:
                            outs.append(engine.run(im, sl_[0], ql_, w_)["iut"])
                    if mode == "pipelined":
                        pipe.wait()
                    torch.cuda.synchronize()
                    cdist.barrier()
                    dtf = cdist.all_reduce_max_scalar(time.perf_counter() - tf0)
                    legs[mode] = (dtf, _lib.profile_records())
                    del outs
                _lib.profile_enable(2)
                engine.run(pool[0][0], pool[0][1][0], pool[0][2], W0[0, 0].clone())
                torch.cuda.synchronize()
                ffine = _lib.profile_records()
                _lib.profile_enable(0)
        finally:
            set_arith(ARITH_X6)
        head = "pipelined" if "pipelined" in legs else "sequential"
        dtf, frecs = legs[head]
        fex = [r for r in frecs if r[0].startswith("extract_features")]
        fdom = [r for r in frecs if r[0].startswith("conv_igemm")]
        fex_fl, fex_ms = sum(r[1] for r in fex), sum(r[3] for r in fex)
        f_traffic, f_traffic_src = pmc_traffic(fdom[0][0].split(" ")[0].split("+")[0]) if fdom else (None, None)
        leg = {
            "value": round(world * nx / dtf, 3), "unit": "episodes/s",
            "ms_per_step": round(dtf / nx * 1e3, 3), "steps": nx,
            "mode": (f"{head}: the same episodes through the same "
                     + (f"episode pipeline ({args.pipeline} extractor streams) " if head == "pipelined" else "loop ")
                     + "as the headline, conv stack " + what),
            "conv_stack": {"tflops": round(fex_fl / (fex_ms * 1e-3) / 1e12, 2),
                           "extract_ms_per_step": round(fex_ms / nx, 3),
                           "note": "roofline_frac from one extra episode's per-launch records (level 2, alone)",
                           **conv_roofline(ffine, peak_leg)},
            "conv_roofline": None if not fdom else {
                "kernel": fdom[0][0].split(" ")[0] + " (bottleneck conv)",
                "achieved": round(sum(r[1] for r in fdom) / (sum(r[3] for r in fdom) * 1e-3) / 1e12, 2),
                "peak": peak_leg, "unit": "TFLOP/s",
                "frac": round(sum(r[1] for r in fdom) / (sum(r[3] for r in fdom) * 1e-3) / 1e12 / peak_leg, 4),
                "traffic": f_traffic, "traffic_unit": "bytes/launch", "traffic_source": f_traffic_src,
                "algorithmic_bytes_per_launch": round(fdom[0][2]) if len(fdom[0]) > 2 else None}}
        if "sequential" in legs and head != "sequential":
            dts_, _ = legs["sequential"]
            leg["sequential"] = {"value": round(world * nx / dts_, 3), "ms_per_step": round(dts_ / nx * 1e3, 3)}
        _lib.check_status()
        return leg

    exact_fp32 = bf16x3 = None
    if not args.train and E == 1 and conv_x6 and args.exact_steps > 0:
        exact_fp32 = arith_leg(ARITH_F32, args.exact_steps, PEAK_FP32_MFMA_TFLOPS, ("pipelined", "sequential"),
                               "on v_mfma_f32 (exact fp32 products: the reference's arithmetic without any split)")
    if not args.train and E == 1 and conv_x6 and args.x3_steps > 0:
        bf16x3 = arith_leg(ARITH_X3S, args.x3_steps, PEAK_X3_TFLOPS, ("pipelined",),
                           "in bf16x3 (operands rounded to 16 significant bits, hi + lo, three bf16 MFMA products: "
                           "a DECLARED APPROXIMATION narrower than the reference's fp32, reported beside the "
                           "headline, not in it; logits within 1e-5 of the reference on the golden episodes)")
        bf16x3["arithmetic"] = "bf16x3 (approximation)"

    out = {
        **head,
        "roofline": {"bound": "hbm", "kernel": (ad_kernel + ", ...> (the 200-step inner loop, test.py:164-187; "
                                                "the time-dominant kernel of the episode)"),
                     "achieved": round(ad_achieved, 1), "peak": PEAK_HBM_GBPS, "unit": "GB/s",
                     "frac": round(ad_achieved / PEAK_HBM_GBPS, 4), "traffic": ad_traffic,
                     "traffic_unit": "bytes/launch", "traffic_source": ad_traffic_src,
                     "algorithmic_bytes_per_launch": ad_bytes_launch, "avg_launch_ms": round(ad_ms_launch, 4),
                     "bytes_basis": f"adapt_iter x n x (f_s {h_feat}x{h_feat}x512 fp32 + S^2 labels) per episode "
                                    "(SURVEY.md §8(d) fused-minimal); the persistent kernel keeps f_s in registers, "
                                    "so its real HBM traffic (traffic) is far below: the loop is bound by the "
                                    "per-step grid-wide reduction, not by bytes",
                     "measured_in": "the timed region" + (" (pipelined: the loop shares the GPU with the next "
                                                          "episodes' extractor passes)" if args.pipeline else ""),
                     "sequential_leg": seq_ad, "latency_floor": latency_floor},
        "conv_roofline": {"bound": "mfma", "kernel": dom_name + " (bottleneck conv 4096->512 3x3, pspnet.py:125)",
                          "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s",
                          "frac": round(achieved / peak, 4), "traffic": traffic, "traffic_unit": "bytes/launch",
                          "traffic_source": traffic_src,
                          "peak_basis": peak_basis, "launches_per_step": dn // args.steps,
                          "flops_per_launch": dfl / dn, "avg_launch_ms": round(dms / dn, 4),
                          **wino_executed(wino_recs, dn, dms, peak)},
        "conv_stack": {"tflops": round(ex_fl / (ex_ms * 1e-3) / 1e12, 2),
                       "frac": round(ex_fl / (ex_ms * 1e-3) / 1e12 / peak, 4),
                       "gflop_per_step": round(ex_fl / args.steps / 1e9, 1),
                       "gflop_per_step_reference_formulation": round(ref_ex_fl / args.steps / 1e9, 1),
                       "tflops_reference_formulation": round(ref_ex_fl / (ex_ms * 1e-3) / 1e12, 2),
                       "ms_per_step": round(ex_ms / args.steps, 3),
                       "note": "whole extract_features bracket (convs + stem/maxpool/PPM byte kernels + gaps); "
                               "executed FLOPs exclude the declared PPM fold (DESIGN.md §3), the reference "
                               "formulation counts the 4096-channel bottleneck conv as written",
                       **conv_roofline(fine, peak)},
        "phases_ms_per_step": {"extract": round(ex_ms / args.steps, 3), "inner_adapt": round(ad_ms / args.steps, 3),
                               "attention": round(at_ms / args.steps, 3),
                               "post_loop_tail": round(tl_ms / args.steps, 4),
                               "post_loop_tail_kernel": round(tk_ms / max(n_tk, 1), 4),
                               "post_loop_tail_note": "cwt_episode_tail: normalize + pred_q0 + CWT + classifier + "
                                                      "upsample / argmax / IoU / CE of pred_q and pred_q0 in ONE "
                                                      "launch (DESIGN.md §3); attention = the module path, 0 here"},
        "phases_roofline": {
            "inner_adapt": {"bound": "hbm", "achieved_GBps": round(ad_achieved, 1), "peak_GBps": PEAK_HBM_GBPS,
                            "frac": round(ad_achieved / PEAK_HBM_GBPS, 4),
                            "bytes_per_step": round(ad_bytes / args.steps), "ms_per_step": round(ad_ms / args.steps, 3)},
            "extract": {"bound": "mfma", "peak_TFLOPs": peak, "frac_executed": round(ex_fl / (ex_ms * 1e-3) / 1e12 / peak, 4),
                        "frac_reference_formulation": round(ref_ex_fl / (ex_ms * 1e-3) / 1e12 / peak, 4)},
            "attention": {"ms_per_step": round(at_ms / args.steps, 3),
                          "gflop_reference_formulation_per_step": round(reference_cwt_flops(h_feat * h_feat) * E / 1e9, 2),
                          "note": "executed in the declared re-associated form (DESIGN.md §3, ~59 MFLOP of token work)"}},
        "tail_roofline": tail_roofline,
        "sequential": seq,
        "batched_pipeline": pairs,
        "exact_fp32": exact_fp32,
        "bf16x3": bf16x3,
    }
    if rank == 0 and args.profile_json:
        with open(args.profile_json, "w") as f:
            json.dump({"timed_records": recs, "per_launch_one_episode": fine, "winograd_parts": wino_recs}, f,
                      indent=1)
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline_train(cfg, sd, tsd) if args.train else cpu_baseline(cfg, sd, tsd)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
