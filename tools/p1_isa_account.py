#!/usr/bin/env python3
"""Instruction account of the partition kernel (msp_p1b_kernel) from its gfx950 assembly.  No GPU.

Compiles cfrk_amd/csrc/msp.hip to assembly, cuts out one instantiation of msp_p1b_kernel (default
<18, 4, false>, the one the headline workload runs) and prints

  * static totals: vector / LDS / global / scalar instructions, plain vector moves, VGPRs, LDS and
    scratch bytes (cold paths included);
  * the vector instructions a wave issues ALONG THE HOT PATH, per phase of p1_tile.

The hot path.  p1_tile marks its phases with assembly comments (P1_PHASE_A, _B1, _B2, _C, _D) and its
cold paths with P1_COLD comments (byte-wise tail loader, direct append, parking, arena overflow); they
emit no instruction.  The tool splits the kernel into basic blocks, follows branches and fall-through
from the entry and never enters a block that holds a P1_COLD comment or a call: what it does not reach
is cold.  A block's phase is the last phase comment on the way to it.  Every hot block counts once --
both sides of a wave-uniform branch (the front end's k-dependent steps), the unrolled P1B_TR trips of
B2 and C as the straight-line code they are -- except blocks inside a loop (the compiler's own
"in Loop" / "Loop Header" comments), which count `trips` times:

  B1  listing loop   --list-trips    max over lanes of runs per lane (measured 5.5 at W = 18)
  D   copy-out loop  records per tile / 512 threads; records per tile = waves x 64 x --runs-per-wave
                     (3.5 at W = 18): the average over the workgroup's waves of ceil() per wave

The estimate is an upper bound for the straight-line part and ignores instructions that lanes skip
with an empty exec mask; compare it with SQ_INSTS_VALU / SQ_WAVES of the kernel (tools/pmc.sh).
Instruction classes are matched by prefix only: v_, ds_, global_ / buffer_ / flat_ / scratch_, s_.

usage: tools/p1_isa_account.py [--w 18] [--tr 4] [--sub 0] [--asm FILE] [--json]
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "cfrk_amd", "csrc", "msp.hip")
PHASES = ["pre", "A", "B1", "B2", "C", "D"]
PHASE_NAMES = {
    "pre": "prologue, histogram clear",
    "A": "front end (load, pack, validity, hashes, minima, change mask)",
    "B1": "staging + run-start listing",
    "B2": "build + bin histogram",
    "C": "reservation, scan, arena write, copy-out table",
    "D": "copy-out",
}


def find_hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


def compile_asm(hipcc, out):
    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", SRC, "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def cut_kernel(text, w, tr, sub):
    """lines of the kernel's body, and its .amdhsa_ / metadata figures"""
    tag = "msp_p1b_kernelILi%dELi%dELb%dEE" % (w, tr, 1 if sub else 0)
    lines = text.split("\n")
    start = end = None
    sym = None
    for i, ln in enumerate(lines):
        if start is None and tag in ln and re.match(r"^_Z\w+:", ln):
            start, sym = i + 1, ln.split(":")[0]
        elif start is not None and ln.startswith(".Lfunc_end"):
            end = i
            break
    if start is None or end is None:
        raise SystemExit("no instantiation %s in the assembly" % tag)
    res = {}
    in_desc = False
    for ln in lines[end:]:
        if ln.strip().startswith(".amdhsa_kernel") and sym in ln:
            in_desc = True
        elif in_desc and ln.strip().startswith(".end_amdhsa_kernel"):
            break
        elif in_desc:
            m = re.match(r"\s*\.amdhsa_(\w+)\s+(\S+)", ln)
            if m:
                res[m.group(1)] = m.group(2)
    # the resolved register / LDS / scratch figures are in the metadata (the descriptor holds expressions)
    meta = {}
    at = text.find(".name:", text.find("amdhsa.kernels"))
    blocks = re.split(r"\n  - \.", text[text.find("amdhsa.kernels"):])
    for b in blocks:
        if re.search(r"\.name:\s+%s\b" % re.escape(sym), b):
            for key in ("vgpr_count", "sgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
                        "vgpr_spill_count", "sgpr_spill_count"):
                m = re.search(r"\.%s:\s+(\d+)" % key, b)
                if m:
                    meta[key] = int(m.group(1))
    del at
    return lines[start:end], meta


def klass(op):
    if op.startswith("v_"):
        return "vector"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "global"
    if op.startswith("s_"):
        return "scalar"
    return None


def parse_blocks(body):
    """basic blocks in layout order: dict(label, ops, marks, loop, succ)"""
    blocks = [dict(label="entry", ops=[], marks=[], loop=None, header=False)]
    for ln in body:
        s = ln.strip()
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m or s.startswith("; %bb."):
            label = m.group(1) if m else s.split()[1].rstrip(":")
            blocks.append(dict(label=label, ops=[], marks=[], loop=None, header=False))
            lm = re.search(r"in Loop: Header=(BB\d+_\d+)", ln)
            if lm:
                blocks[-1]["loop"] = ".L" + lm.group(1)
            if "Loop Header" in ln:
                blocks[-1]["loop"] = label
                blocks[-1]["header"] = True
            continue
        if s.startswith(";"):
            mm = re.match(r"^;\s*(P1_PHASE_\w+|P1_COLD)", s)
            if mm:
                blocks[-1]["marks"].append((len(blocks[-1]["ops"]), mm.group(1)))
            lm = re.search(r"in Loop: Header=(BB\d+_\d+)", s)
            if lm and not blocks[-1]["ops"]:
                blocks[-1]["loop"] = ".L" + lm.group(1)
            continue
        if not s or s.startswith("."):
            continue
        op = s.split()[0]
        if klass(op):
            arg = s.split()[1] if len(s.split()) > 1 else ""
            blocks[-1]["ops"].append((op, arg))
            # a branch ends the block: what follows it is a block of its own (the compiler names it in a comment)
    # successors
    index = {b["label"]: i for i, b in enumerate(blocks)}
    for i, b in enumerate(blocks):
        succ = []
        fall = True
        for op, arg in b["ops"]:
            if op.startswith("s_cbranch"):
                if arg in index:
                    succ.append(index[arg])
            elif op == "s_branch":
                if arg in index:
                    succ.append(index[arg])
                fall = False
            elif op.startswith(("s_endpgm", "s_setpc")):
                fall = False
        if fall and i + 1 < len(blocks):
            succ.insert(0, i + 1)                  # fall-through first: the walk follows the layout
        b["succ"] = succ
        b["call"] = any(op.startswith("s_swappc") for op, _ in b["ops"])
        b["cold"] = b["call"] or any(mk == "P1_COLD" for _, mk in b["marks"])
    return blocks


def account(blocks, list_trips, copy_trips):
    """walk the hot blocks from the entry; per phase: vector instructions x trips"""
    per = {p: dict(vector=0.0, lds=0.0, glob=0.0, scalar=0.0, moves=0.0, static_vector=0) for p in PHASES}
    loops = []
    seen = {}
    stack = [(0, "pre")]
    while stack:
        i, ph = stack.pop()
        if i in seen or blocks[i]["cold"]:
            continue
        seen[i] = ph
        b = blocks[i]
        # phase of every instruction of the block
        marks = [(at, mk[len("P1_PHASE_"):]) for at, mk in b["marks"] if mk.startswith("P1_PHASE_")]
        trips = 1.0
        if b["loop"]:
            lph = seen.get(next((j for j, x in enumerate(blocks) if x["label"] == b["loop"]), i), ph)
            trips = list_trips if lph == "B1" else copy_trips if lph == "D" else 1.0
            if b["header"]:
                loops.append((b["label"], lph, trips))
        for n, (op, _) in enumerate(b["ops"]):
            while marks and marks[0][0] <= n:
                ph = marks.pop(0)[1]
            c = klass(op)
            acc = per[ph]
            if c == "vector":
                acc["vector"] += trips
                acc["static_vector"] += 1
                if op == "v_mov_b32_e32":
                    acc["moves"] += trips
            elif c == "lds":
                acc["lds"] += trips
            elif c == "global":
                acc["glob"] += trips
            elif c == "scalar":
                acc["scalar"] += trips
        for _, mk in marks:
            ph = mk
        for j in reversed(b["succ"]):
            stack.append((j, ph))
    return per, loops, seen


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--w", type=int, default=18)
    ap.add_argument("--tr", type=int, default=4)
    ap.add_argument("--sub", type=int, default=0)
    ap.add_argument("--asm", help="assembly of msp.hip made earlier (skips the compile)")
    ap.add_argument("--list-trips", type=float, default=5.5, help="trips of the run-start listing loop per wave")
    ap.add_argument("--runs-per-wave", type=float, default=3.5 * 64, help="records a wave emits per tile")
    ap.add_argument("--json", action="store_true", help="one JSON object instead of the table")
    a = ap.parse_args()

    if a.asm:
        text = open(a.asm).read()
    else:
        hipcc = find_hipcc()
        if not hipcc:
            raise SystemExit("hipcc not found (set HIPCC)")
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "msp.s")
            compile_asm(hipcc, out)
            text = open(out).read()
    body, meta = cut_kernel(text, a.w, a.tr, a.sub)
    blocks = parse_blocks(body)
    copy_trips = 8 * a.runs_per_wave / 512.0
    per, loops, seen = account(blocks, a.list_trips, copy_trips)

    static = dict(vector=0, lds=0, glob=0, scalar=0, moves=0)
    for b in blocks:
        for op, _ in b["ops"]:
            c = klass(op)
            static["glob" if c == "global" else c] += 1
            if op == "v_mov_b32_e32":
                static["moves"] += 1
    hot_total = sum(p["vector"] for p in per.values())
    emission = sum(per[p]["vector"] for p in ("B1", "B2", "C", "D"))
    result = dict(kernel="msp_p1b_kernel<%d, %d, %s>" % (a.w, a.tr, "true" if a.sub else "false"),
                  static=static, vgprs=meta.get("vgpr_count"), sgprs=meta.get("sgpr_count"),
                  lds_bytes=meta.get("group_segment_fixed_size"), scratch_bytes=meta.get("private_segment_fixed_size"),
                  vgpr_spills=meta.get("vgpr_spill_count", 0), sgpr_spills=meta.get("sgpr_spill_count", 0),
                  hot_blocks=len(seen), blocks=len(blocks), phases=per, hot_vector_per_wave=hot_total,
                  emission_vector_per_wave=emission, list_trips=a.list_trips, copy_trips=copy_trips)
    if a.json:
        print(json.dumps(result))
        return 0
    print(result["kernel"])
    print("static: %d vector (%d plain moves), %d LDS, %d global, %d scalar instructions" %
          (static["vector"], static["moves"], static["lds"], static["glob"], static["scalar"]))
    print("        %s VGPRs, %s SGPRs, %s B LDS, %s B scratch, spills %s VGPR / %s SGPR" %
          (result["vgprs"], result["sgprs"], result["lds_bytes"], result["scratch_bytes"], result["vgpr_spills"], result["sgpr_spills"]))
    print("hot path: %d of %d blocks; loops: %s" %
          (len(seen), len(blocks), ", ".join("%s in %s x %.2f" % l for l in loops) or "none"))
    print("%-4s %9s %8s %7s %7s %7s %7s  %s" % ("", "vector/wv", "(static)", "moves", "LDS", "global", "scalar", ""))
    for p in PHASES:
        q = per[p]
        print("%-4s %9.1f %8d %7.1f %7.1f %7.1f %7.1f  %s" %
              (p, q["vector"], q["static_vector"], q["moves"], q["lds"], q["glob"], q["scalar"], PHASE_NAMES[p]))
    print("hot-path vector instructions per wave: %.1f (emission B1 + B2 + C + D: %.1f)" % (hot_total, emission))
    return 0


if __name__ == "__main__":
    sys.exit(main())
