#!/usr/bin/env python3
"""Host wall clock of the host forms of the ABI pairs (arguments in pageable host memory: staging, layout check, the
feature's kernels, the results copied down) on 10^6 synthetic reads of 150 bases against one counted k = 31 job, a FASTA
and a FASTQ text of the same reads: one warm-up, then median / min / max of N calls each in ms, one JSON line.
usage (GPU box): tools/bench_host_forms.py [--reads R] [--reps N] [--lib PATH] [--out FILE]   (--lib: another build of the
library, for a same-box A/B)"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cfrk_amd  # noqa: E402
import cfrk_amd.lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--lib", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.lib:
    cfrk_amd.lib._SO = os.path.abspath(args.lib)
R, L, K, REPS = args.reads, 150, 31, args.reps
ctx = cfrk_amd.Context(0)
nN = R * (L + 1)
d = ctx.alloc(nN + 64)
ctx.synth_reads_device(0, R, L, 3 * R, d)
ctx.sync()
data = np.empty(nN, np.int8)
ctx.d2h(data, d)
ctx.free(d)
start = np.arange(R, dtype=np.int64) * (L + 1)
length = np.full(R, L, np.int32)
g = cfrk_amd.GlobalCounter(ctx, K, cfrk_amd.CFRK_CANONICAL, 4 * R)
g.add(data, start, length)
g.finish()
spans = g.read_spans(data, start, length, 2, cfrk_amd.CFRK_COUNT_MAX)
keep = (np.arange(R) % 7 != 0).astype(np.uint8)
bases = np.frombuffer(b"ACGT", np.uint8)[np.clip(data.reshape(R, L + 1)[:, :L], 0, 3)]
head = np.frombuffer("".join(f">{i:07d}\n" for i in range(R)).encode(), np.uint8).reshape(R, 9)
nl = np.full((R, 1), 10, np.uint8)
fasta = np.ascontiguousarray(np.concatenate([head, bases, nl], axis=1)).reshape(-1)
qhead = head.copy(); qhead[:, 0] = ord("@")
plus = np.tile(np.frombuffer(b"+\n", np.uint8), (R, 1))
qual = np.full((R, L), ord("I"), np.uint8); qual[:, ::11] = ord("#")
fastq = np.ascontiguousarray(np.concatenate([qhead, bases, nl, plus, qual, nl], axis=1)).reshape(-1)

def timed(fn):
    fn()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 2), "min_ms": round(min(ts), 2), "max_ms": round(max(ts), 2)}

res = {"library": os.path.relpath(cfrk_amd.lib._SO, ROOT), "reads": R, "L": L, "k": K, "reps": REPS}
res["global_query_reads"] = timed(lambda: g.query_reads(data, start, length))
res["global_read_stats"] = timed(lambda: g.read_stats(data, start, length, 2))
res["global_read_spans"] = timed(lambda: g.read_spans(data, start, length, 2, cfrk_amd.CFRK_COUNT_MAX))
res["reads_select"] = timed(lambda: ctx.select_reads(data, start, length, spans, keep, 50))
res["per_read_sparse_k21"] = timed(lambda: ctx.per_read_sparse(data, start, length, 21, cfrk_amd.CFRK_CANONICAL))
res["distinct_sketch"] = timed(lambda: ctx.distinct_sketch(data, K, cfrk_amd.CFRK_CANONICAL, start, length))
res["fasta_parse"] = timed(lambda: ctx.parse_fasta(fasta))
res["fastq_parse_q20"] = timed(lambda: ctx.parse_fastq(fastq, 20))
def add():
    gg = cfrk_amd.GlobalCounter(ctx, K, cfrk_amd.CFRK_CANONICAL, 4 * R)
    gg.add(data, start, length)
    gg.finish()
res["global_add_finish"] = timed(add)
print(json.dumps(res), flush=True)
if args.out:
    with open(args.out, "a") as f:
        f.write(json.dumps(res) + "\n")
