"""Time the x6 two-source 1x1 conv (a block's conv3 + downsample conv as one GEMM,
cwt_debug_conv_x6_dual) over every dual form / split-K count for the four fused shapes of an
extractor config, beside the library's own plan.  Writes the file --out names; the fastest rows go into
csrc/conv_plans_x6.inc as {M, Co, K1 + K2, bm, bn, nsplit, var}.

    python tools/conv_dual_sweep.py [--config 50:473:2] [--occupy 59]
"""
import argparse
import json
import os
import sys

import torch

os.environ.setdefault("CWT_DBG_W3_CACHE", "1")   # the timed calls are the conv alone (conv_s_sweep.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import conv_s_sweep as css  # noqa: E402
from few_shot_seg_cwt_amd import _lib  # noqa: E402

FORMS = [(4128, 128), (5128, 128), (5128, 64), (5064, 128)]   # bm = 1000 * var + rows (conv_forms.h dual rows)


def fused_shapes(layers, S, N):
    """(name, K1, K2, Co, H of x, stride, Ho) of the first block of each layer"""
    d2 = lambda x: (x - 1) // 2 + 1  # noqa: E731
    H = d2(d2(S))
    out, inpl = [], 128
    for li, planes in enumerate([64, 128, 256, 512]):
        s = 2 if li == 1 else 1
        Ho = d2(H) if s == 2 else H
        out.append((f"l{li + 1}", planes, inpl, planes * 4, H, s, Ho))
        inpl, H = planes * 4, Ho
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="50:473:2")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--occupy", type=int, default=0, help="CUs held meanwhile (the pipeline's resident inner loop: 59)")
    ap.add_argument("--out", default="conv_dual_sweep.json")
    ap.add_argument("--ab", default="", help="an environment knob read at every launch (CWT_X6_GEMM_BODY): time the "
                    "library's own plan with it at 0 and at 1, alternating in this process")
    ap.add_argument("--pairs", type=int, default=5, help="--ab: timings per arm")
    args = ap.parse_args()
    css.OCCUPY = args.occupy
    layers, S, N = (int(v) for v in args.config.split(":"))
    dev = torch.device("cuda", 0)
    lib, ctx, sp = _lib.lib(), _lib.ctx(0), _lib.stream_ptr()
    res = []
    for name, K1, K2, Co, H, stride, Ho in fused_shapes(layers, S, N):
        M, K = N * Ho * Ho, K1 + K2
        t = torch.randn(N, Ho, Ho, K1, device=dev)
        x = torch.randn(N, H, H, K2, device=dev)
        w3 = torch.randn(Co, K1, device=dev) * (2.0 / K1) ** 0.5
        wd = torch.randn(Co, K2, device=dev) * (2.0 / K2) ** 0.5
        one, zero = torch.ones(Co, device=dev), torch.zeros(Co, device=dev)
        y = torch.empty(N, Ho, Ho, Co, device=dev)

        def dual(bm, bn, ns):
            return lambda: _lib.check(lib.cwt_debug_conv_x6_dual(
                ctx, _lib.ptr(t), N, Ho, Ho, K1, _lib.ptr(x), H, H, K2, stride, _lib.ptr(w3), _lib.ptr(one),
                _lib.ptr(zero), _lib.ptr(wd), _lib.ptr(one), _lib.ptr(zero), Co, 1, _lib.ptr(y), bm, bn, ns, sp))

        if args.ab:
            tm = css.ab_timed(dual(0, 0, 0), args.reps, args.ab, args.pairs)
            m0, m1, gain, spread = css.ab_summary(tm)
            print(f"{name} M={M} Co={Co} K={K1}+{K2}: {args.ab}=0 {m0:.1f}  =1 {m1:.1f} us  gain {gain:+.1f} %  "
                  f"(repeat spread {spread:.1f} %)", flush=True)
            res.append({"name": name, "M": M, "Co": Co, "K1": K1, "K2": K2, "knob": args.ab, "us": tm,
                        "gain_pct": round(gain, 2), "spread_pct": round(spread, 2)})
            continue
        rows = []
        for bm, bn in [(0, 0)] + FORMS:
            for ns in (0,) if bm == 0 else (1, 2, 4):
                if ns > 1 and (K // 32) // ns < 4:
                    continue
                rows.append({"bm": bm % 1000, "bn": bn, "var": bm // 1000, "ns": ns,
                             "us": round(css.timed(dual(bm, bn, ns), args.reps), 2)})
        best = min(rows[1:], key=lambda q: q["us"])
        print(f"{name} M={M} Co={Co} K={K1}+{K2}: auto {rows[0]['us']:.1f}, best "
              f"{best['bm']}x{best['bn']}s{best['ns']}v{best['var']} {best['us']:.1f} us", flush=True)
        res.append({"name": name, "M": M, "Co": Co, "K1": K1, "K2": K2, "plans": rows})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
