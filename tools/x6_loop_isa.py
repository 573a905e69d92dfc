"""Count the K-loop of conv_igemm_x6 instantiations by instruction class (CPU only: it compiles, it
does not run).

One translation unit instantiates the named rows of conv_forms.h -- each row's general body and,
where the row is listed in CWT_CONV_GEMM_ROWS_X6, its GEMM-shaped body (PF bit 256) -- and is
compiled with `hipcc -S --cuda-device-only` and the build's own flags.  Per kernel it prints the
loop's instruction counts by opcode prefix (v_mfma, v_pk_, other v_, s_waitcnt, s_barrier, other
s_, ds_, buffer_), the registers, the LDS bytes and the occupancy the compiler reports.

    python tools/x6_loop_isa.py [--rows 128x128:5,128x128:25] [--csrc DIR] [--out FILE.json]

--rows all: every row that has a GEMM-shaped body.  --csrc: another tree's csrc directory (a parent
checkout: rows only, it has no PF bit 256).
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from few_shot_seg_cwt_amd import build as _build  # noqa: E402

CLASSES = ["v_mfma", "v_pk_", "v_", "s_waitcnt", "s_barrier", "s_", "ds_", "buffer_"]
GEMM_PF = 256
STAGE = 6  # names the instantiation only


def classify(op):
    for c in CLASSES:   # ordered: the specific prefixes before "v_" and "s_"
        if op.startswith(c):
            return c
    return "other"


def form_rows(csrc):
    """{(bm, bn, var): (waves_m, waves_n, nstg, pf)} of conv_forms.h and the set of GEMM-body rows."""
    text = open(os.path.join(csrc, "conv_forms.h")).read()
    rows = {}
    for m in re.finditer(r"\bX\((\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\)", text):
        bm, bn, var, wm, wn, ns, pf, _ = map(int, m.groups())
        rows[(bm, bn, var)] = (wm, wn, ns, pf)
    gemm = {tuple(map(int, m.groups())) for m in re.finditer(r"\bG\((\d+), (\d+), (\d+)\)", text)}
    return rows, gemm


def kernel_name(bm, bn, wm, wn, ns, pf):
    return f"x6_loop_probe<{bm}, {bn}, {wm}, {wn}, {ns}, {STAGE}, {pf}>"


def translation_unit(insts):
    lines = ['#include "conv_body.h"', "namespace cwt {",
             "// conv_igemm_x6's own wrapper (conv_x6.hip) under a name of this tool's",
             "template <int BM, int BN, int WAVES_M, int WAVES_N, int NSTG, int STAGE, int PF>",
             "__global__ __launch_bounds__(WAVES_M* WAVES_N * 64) void x6_loop_probe(ConvSArgs a) {",
             "  constexpr int STG = (BM + BN) * 128 + BN * 64;",
             "  constexpr int NS = NSTG * STG <= 163840 ? NSTG : 163840 / STG;",
             "  conv_s_body<BM, BN, WAVES_M, WAVES_N, NS, 6, (PF | 8)>(a);", "}"]
    for bm, bn, wm, wn, ns, pf in insts:
        lines.append(f"template __global__ void x6_loop_probe<{bm}, {bn}, {wm}, {wn}, {ns}, {STAGE}, {pf}>(ConvSArgs);")
    lines.append("}  // namespace cwt")
    return "\n".join(lines) + "\n"


def compile_isa(csrc, insts):
    with tempfile.TemporaryDirectory() as tmp:
        src, asm = os.path.join(tmp, "x6_loop_probe.hip"), os.path.join(tmp, "x6_loop_probe.s")
        with open(src, "w") as f:
            f.write(translation_unit(insts))
        cmd = [_build.HIPCC, *_build.FLAGS, "-I", csrc, "-I", os.path.join(os.path.dirname(os.path.dirname(csrc)), "include"),
               "-S", "--cuda-device-only", src, "-o", asm]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed:\n{r.stdout}\n{r.stderr}")
        return open(asm).read()


def demangle(names):
    r = subprocess.run(["c++filt"] + names, capture_output=True, text=True)
    out = r.stdout.split("\n") if r.returncode == 0 else names
    return dict(zip(names, out))


INSTR = re.compile(r"^\s+([a-z][a-z0-9_]+)\b")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)")


def k_loop(body):
    """The instructions of the K-loop: a label and a later branch back to it.  Of the loops that hold
    the most MFMAs, one that also holds the operand DMA (buffer_ loads), the smallest such: on the
    deeper rings the loop header has a second, shorter back edge that skips the refill (the drain
    of the last tiles), which is not the steady state."""
    label_at, best = {}, None
    for i, ln in enumerate(body):
        m = LABEL.match(ln)
        if m:
            label_at[m.group(1)] = i
            continue
        m = BRANCH.match(ln)
        if m and m.group(1) in label_at:
            lo = label_at[m.group(1)]
            ops = [INSTR.match(x).group(1) for x in body[lo:i + 1] if INSTR.match(x)]
            key = (-sum(o.startswith("v_mfma") for o in ops), not any(o.startswith("buffer_") for o in ops), len(ops))
            if best is None or key < best[0]:
                best = (key, ops)
    return best[1] if best else []


def analyse(asm):
    """{demangled kernel name: {"loop": {class: count}, "loop_total", "vgpr", "agpr", "sgpr", "lds", "spill", "occupancy"}}"""
    lines = asm.split("\n")
    starts = [(i, m.group(1)) for i, ln in enumerate(lines) for m in [re.match(r"^(_Z\w*x6_loop_probe\w*):", ln)] if m]
    names = demangle([n for _, n in starts])
    out = {}
    for i, sym in starts:
        end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
        ops = k_loop(lines[i:end + 1])
        counts = {c: 0 for c in CLASSES}
        for o in ops:
            c = classify(o)
            counts[c] = counts.get(c, 0) + 1
        # the kernel's resource comments follow its code
        tail = "\n".join(lines[end:end + 400])
        num = lambda pat: int(re.search(pat, tail).group(1))  # noqa: E731
        name = re.sub(r"^void cwt::|\(cwt::ConvSArgs\)$", "", names[sym])
        out[name] = {"loop": counts, "loop_total": len(ops),
                     "vgpr": num(r"; NumVgprs: (\d+)"), "agpr": num(r"; NumAgprs: (\d+)"),
                     "sgpr": num(r"; TotalNumSgprs: (\d+)"), "lds": num(r"; LDSByteSize: (\d+)"),
                     "spill": num(r"; ScratchSize: (\d+)"), "occupancy": num(r"; Occupancy: (\d+)")}
    return out


def loop_isa(rows, csrc=_build.CSRC):
    """rows: [(bm, bn, var)] -> {(bm, bn, var, pf_extra): analysis}; pf_extra 0 the general body, 256
    the GEMM-shaped one (only for rows the tree lists as having it)."""
    table, gemm = form_rows(csrc)
    insts, keys = [], []
    for row in rows:
        if row not in table:
            raise SystemExit(f"no row {row} in {csrc}/conv_forms.h")
        wm, wn, ns, pf = table[row]
        for extra in (0, GEMM_PF) if row in gemm else (0,):
            insts.append((row[0], row[1], wm, wn, ns, pf | extra))
            keys.append(row + (extra,))
    res = analyse(compile_isa(csrc, insts))
    return {k: res[kernel_name(*i)] for k, i in zip(keys, insts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="128x128:5", help="BMxBN:VAR,... or all")
    ap.add_argument("--csrc", default=_build.CSRC)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.rows == "all":
        rows = sorted(form_rows(args.csrc)[1])
    else:
        rows = [tuple(int(v) for v in re.split("[x:]", r)) for r in args.rows.split(",")]
    res = loop_isa(rows, args.csrc)
    doc = []
    for (bm, bn, var, extra), r in res.items():
        body = "gemm" if extra else "general"
        print(f"{bm}x{bn} var {var} {body:7s}: loop {r['loop_total']:4d} = " +
              " ".join(f"{c}:{r['loop'][c]}" for c in CLASSES) +
              f" | vgpr {r['vgpr']} agpr {r['agpr']} sgpr {r['sgpr']} lds {r['lds']} scratch {r['spill']} occ {r['occupancy']}")
        doc.append({"bm": bm, "bn": bn, "var": var, "body": body, **r})
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
