#!/usr/bin/env python3
"""Instruction account of the leaf kernel's scan of the complete stream (msp_p3_kernel, p3_body phase 1a) from its
gfx950 assembly.  No GPU.

Compiles cfrk_amd/csrc/msp.hip to assembly, cuts out one instantiation of msp_p3_kernel (default <true, false>, the
one the headline workload runs) and prints, per marked part of the scan, the vector, scalar, LDS and global
instructions the kernel's text holds, plus the kernel's VGPRs, SGPRs, LDS and scratch.

The parts.  p3_body marks the parts of the scan with assembly comments (P3_MARK: they emit no instruction):

  LOAD    loop control and the global loads of a step        HOME    slot hash, table read, compare, add
  CACHE   the look into the displaced-run cache               APPEND  leftovers handed to the wave's set (ds_permute)
  DRAIN   the probe loop over a full set + cache install      SEED    warm-up: the first records go straight to DRAIN
  MERGE   the cache's counts added to the table after the scan

A marker opens a SEGMENT that runs, in the order of the kernel's text, to the next marker; `before` is everything in
front of the first marker (prologue, table clear) and `after` everything behind P3_PART_END (skeleton, expansion,
copy-out).  `after` is marked too and listed part by part in a second table (JSON: "phase2"):

  LIST    occupied slots of the record table ranked            ANCHOR  truncated runs look their complete twin up
  GROUP   notes grouped, lists written                         CEXP    loop over the listed runs
  XSETUP / XWALK / XSTEP   count_record_v2: a lane's share and first k-mer / walk over the notes / a step of two k-mers
  TRUNC   truncated runs without a twin                        OUT     copy-out

The scan is inlined several times (two steps per trip of the main loop, the peeled tail, the general loop
next to the specialised one), so a part has several segments: the table gives their number, the sum and the SMALLEST and
LARGEST segment.  What one call of a part issues is about one segment, not the sum.

This is an account of the TEXT, classified by mnemonic prefix only (v_, s_, ds_, global_ / buffer_ / flat_ / scratch_):
the compiler moves instructions across the comments (a hoisted address computation lands in the part in front), blocks
it lays out elsewhere are counted where they lie, and a loop's body counts once however often it runs (DRAIN's probe loop
runs as many trips as the longest chain among the wave's lanes).  Set it against SQ_INSTS_VALU / _SALU / _LDS per wave of
the P3 launches (tools/pmc.sh) and the path frequencies of an ablation build.

usage: tools/p3_isa_account.py [--canon 1] [--shared 0] [--asm FILE] [--define NAME=VALUE ...] [--json]
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
PARTS = ["before", "SEED", "LOAD", "HOME", "CACHE", "APPEND", "DRAIN", "MERGE", "after",
         "LIST", "ANCHOR", "GROUP", "CEXP", "XSETUP", "XWALK", "XSTEP", "TRUNC", "OUT"]
PHASE2 = PARTS[PARTS.index("after"):]              # behind P3_PART_END: not part of the scan
PART_NAMES = {
    "before": "prologue, stream bounds, table clear",
    "SEED": "warm-up: first records straight into the probe loop",
    "LOAD": "loads and loop overhead",
    "HOME": "home-slot step",
    "CACHE": "cache look",
    "APPEND": "leftover append",
    "DRAIN": "drain / insert loop (+ cache install)",
    "MERGE": "cache merge after the scan",
    "after": "skeleton, expansion, copy-out (second table: up to phase 2's first marker -- export, pool-wide table)",
    "LIST": "phase 2: the record table's occupied slots read and ranked by length",
    "ANCHOR": "phase 2: truncated runs look their complete twin up",
    "GROUP": "phase 2: notes grouped by slot, lists written, key subsets",
    "CEXP": "phase 2: loop over the listed runs (list and table reads)",
    "XSETUP": "expansion: a lane's share of a record, first k-mer, reverse complement",
    "XWALK": "expansion: the walk(s) over the noted lengths",
    "XSTEP": "expansion: one step of two k-mers (roll, canonicalise, hash, k-mer table)",
    "TRUNC": "phase 2: truncated runs without a twin / of the sorted list",
    "OUT": "copy-out to the result list",
}
CLASSES = ("vector", "scalar", "lds", "global")


def find_hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


def compile_asm(hipcc, out, defines=()):
    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", SRC, "-o", out]
    cmd += ["-D" + d for d in defines]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


def cut_kernel(text, canon, shared):
    """lines of the kernel's body and its metadata figures"""
    tag = "msp_p3_kernelILb%dELb%dEE" % (canon, shared)
    lines = text.split("\n")
    start = end = sym = None
    for i, ln in enumerate(lines):
        if start is None and tag in ln and re.match(r"^_Z\w+:", ln):
            start, sym = i + 1, ln.split(":")[0]
        elif start is not None and ln.startswith(".Lfunc_end"):
            end = i
            break
    if start is None or end is None:
        raise SystemExit("no instantiation %s in the assembly" % tag)
    meta = {}
    for b in re.split(r"\n  - \.", text[text.find("amdhsa.kernels"):]):
        if re.search(r"\.name:\s+%s\b" % re.escape(sym), b):
            for key in ("vgpr_count", "sgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
                        "vgpr_spill_count", "sgpr_spill_count"):
                m = re.search(r"\.%s:\s+(\d+)" % key, b)
                if m:
                    meta[key] = int(m.group(1))
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


def segments(body):
    """[(part, {class: instructions})] in the order of the text"""
    segs = [("before", dict.fromkeys(CLASSES, 0))]
    for ln in body:
        s = ln.strip()
        if s.startswith(";"):
            m = re.match(r"^;\s*P3_PART_(\w+)", s)
            if m:
                part = m.group(1)
                segs.append(("after" if part == "END" else part, dict.fromkeys(CLASSES, 0)))
            continue
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        c = klass(s.split()[0])
        if c:
            segs[-1][1][c] += 1
    return segs


def account(segs):
    """-> (the scan's parts with `before` and `after`, the parts `after` is made of)"""
    per, per2 = {}, {}
    for part, cnt in segs:
        if part not in PARTS:
            raise SystemExit("unknown marker P3_PART_%s" % part)
        # a part of phase 2 counts as `after` in the scan's table, and under its own name in phase 2's
        for table, name in ((per, "after" if part in PHASE2 else part),) + (((per2, part),) if part in PHASE2 else ()):
            q = table.setdefault(name, dict(segments=0, smallest=None, largest=None, **dict.fromkeys(CLASSES, 0)))
            q["segments"] += 1
            for c in CLASSES:
                q[c] += cnt[c]
            issue = cnt["vector"] + cnt["scalar"] + cnt["lds"] + cnt["global"]
            q["smallest"] = issue if q["smallest"] is None else min(q["smallest"], issue)
            q["largest"] = issue if q["largest"] is None else max(q["largest"], issue)
    return per, per2


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--canon", type=int, default=1)
    ap.add_argument("--shared", type=int, default=0)
    ap.add_argument("--asm", help="assembly of msp.hip made earlier (skips the compile)")
    ap.add_argument("--define", action="append", default=[], help="NAME=VALUE passed to the compiler as -D")
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
            compile_asm(hipcc, out, a.define)
            text = open(out).read()
    body, meta = cut_kernel(text, a.canon, a.shared)
    per, per2 = account(segments(body))
    scan_parts = [p for p in PARTS if p in per and p not in ("before", "after")]
    scan = {c: sum(per[p][c] for p in scan_parts) for c in CLASSES}
    scratch_ops = sum(1 for ln in body if ln.strip().startswith("scratch_"))
    result = dict(kernel="msp_p3_kernel<%s, %s>" % ("true" if a.canon else "false", "true" if a.shared else "false"),
                  vgprs=meta.get("vgpr_count"), sgprs=meta.get("sgpr_count"), lds_bytes=meta.get("group_segment_fixed_size"),
                  scratch_bytes=meta.get("private_segment_fixed_size"), scratch_instructions=scratch_ops,
                  vgpr_spills=meta.get("vgpr_spill_count", 0), sgpr_spills=meta.get("sgpr_spill_count", 0),
                  parts=per, scan=scan, phase2=per2)
    if a.json:
        print(json.dumps(result))
        return 0
    print(result["kernel"])
    print("%s VGPRs, %s SGPRs, %s B LDS, %s B scratch (%d scratch instructions), spills %s VGPR / %s SGPR" %
          (result["vgprs"], result["sgprs"], result["lds_bytes"], result["scratch_bytes"], scratch_ops,
           result["vgpr_spills"], result["sgpr_spills"]))
    print("%-7s %4s %7s %7s %5s %7s %9s %8s  %s" % ("part", "segs", "vector", "scalar", "LDS", "global", "smallest", "largest", ""))
    for p in PARTS:
        if p not in per:
            continue
        q = per[p]
        print("%-7s %4d %7d %7d %5d %7d %9d %8d  %s" %
              (p, q["segments"], q["vector"], q["scalar"], q["lds"], q["global"], q["smallest"], q["largest"], PART_NAMES[p]))
    print("scan (all parts but before / after): %d vector, %d scalar, %d LDS, %d global instructions of text" %
          (scan["vector"], scan["scalar"], scan["lds"], scan["global"]))
    print("`after`, part by part (phase 2: count_record_v2 is inlined at every call, so XSETUP / XWALK / XSTEP have a segment"
          " per call site)")
    for p in PHASE2:
        if p in per2:
            q = per2[p]
            print("%-7s %4d %7d %7d %5d %7d %9d %8d  %s" %
                  (p, q["segments"], q["vector"], q["scalar"], q["lds"], q["global"], q["smallest"], q["largest"], PART_NAMES[p]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
