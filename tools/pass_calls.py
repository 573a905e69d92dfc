"""Per-call kernel durations of an extractor pass from a rocprofv3 kernel trace of the bench run:
the extractor's kernels in dispatch order, cut into passes at the stem's first conv, averaged over the
timed passes (the first `warm` dropped).  The call list is config #2's (R50, 473, two images per pass:
which convs run split-K 2 follows csrc/conv_plans_x6.inc); a trace that does not match it is reported,
not averaged.  "unfused": CWT_FUSE_DOWN=0 CWT_FUSE_SPLITK_WINO=0 or a build from before the fusions.

    python tools/pass_calls.py unfused|fused run_kernel_trace.csv out.json
"""
import csv
import json
import re
import sys

arm, path, out = sys.argv[1:4]
warm = 5
BLOCKS = [3, 4, 6, 3]


def labels(fused):
    """The extractor's kernels between two stem conv1 launches, by name pattern, in call order"""
    seq = [("conv", "stem2"), ("conv", "stem3"), ("maxpool", "maxpool")]
    for li, nb in enumerate(BLOCKS):
        for bi in range(nb):
            p = f"l{li + 1}b{bi}"
            sk = li >= 2 and bi >= 1      # conv1 runs split-K 2 (Ci = 1024 / 2048 at M = 7200)
            wino = li >= 2                # conv2 in the Winograd form (Ci >= 256; layer2's Ci = 128 is direct)
            seq.append(("conv", p + ".c1"))
            if sk and not fused:
                seq.append(("epi", p + ".c1.epilogue"))
            if wino:
                seq += [("win", p + ".c2.wino_in"), ("conv", p + ".c2.gemm"), ("wout", p + ".c2.wino_out")]
            else:
                seq.append(("conv", p + ".c2"))
                if li == 1:   # layer2 conv2 runs split-K 2 (K = 1152 at M = 7200)
                    seq.append(("epi", p + ".c2.epilogue"))
            if bi == 0 and not fused:
                seq.append(("conv", p + ".down"))
            seq.append(("conv", p + (".c3+down" if bi == 0 and fused else ".c3")))
    return seq


KIND = [("conv", r"conv_igemm_x6"), ("epi", r"conv_s_splitk_epilogue"), ("win", r"wino4?_in_kernel"),
        ("wout", r"wino4?_out_kernel"), ("maxpool", r"maxpool"), ("stem1", r"stem_conv1")]


def kind(name):
    for k, pat in KIND:
        if re.search(pat, name):
            return k
    return None


rows = []
for r in csv.DictReader(open(path)):
    k = kind(r["Kernel_Name"])
    if k:
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Stream_Id"], k, r["Kernel_Name"]))
rows.sort()
by_stream = {}
for r in rows:
    by_stream.setdefault(r[2], []).append(r)
passes = []
for s, rs in by_stream.items():
    cur = None
    for r in rs:
        if r[3] == "stem1":
            cur = []
            passes.append((r[0], cur))
        elif cur is not None:
            cur.append(r)
passes.sort(key=lambda p: p[0])
seq = labels(arm in ("fused", "branch"))
print(arm, "passes", len(passes), "kernels per pass", sorted({len(p[1]) for p in passes}), "expected >=", len(seq))
acc = {}
used = 0
for _, ks in passes[warm:]:
    head = ks[:len(seq)]
    if [k[3] for k in head] != [s[0] for s in seq]:
        bad = next(i for i, (a, b) in enumerate(zip(head, seq)) if a[3] != b[0])
        print("  sequence mismatch at", bad, head[bad][3], head[bad][4][:60], "expected", seq[bad])
        continue
    used += 1
    for (t0, t1, _, _, _), (_, lab) in zip(head, seq):
        acc.setdefault(lab, []).append((t1 - t0) / 1e3)
res = {lab: round(sum(v) / len(v), 2) for lab, v in acc.items()}
tot = {k: round(sum(v for lab, v in res.items() if sel(lab)), 1) for k, sel in
       [("conv", lambda s: not s.endswith(("epilogue", "wino_in", "wino_out", "maxpool"))),
        # the launches that are plain GEMMs (kh = kw = 1, pad = 0): 1x1 convs and the Winograd products
        ("conv_gemm_shaped", lambda s: s.endswith((".c1", ".c3", ".c3+down", ".down", ".c2.gemm"))),
        ("epilogue", lambda s: s.endswith("epilogue")), ("wino_in", lambda s: s.endswith("wino_in")),
        ("wino_out", lambda s: s.endswith("wino_out"))]}
print("  passes used", used, "per-pass sums (us), the bottleneck conv and the PPM not included:", tot)
json.dump({"arm": arm, "passes_used": used, "us_per_call": res, "sum_us": tot}, open(out, "w"), indent=1)
