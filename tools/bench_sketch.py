"""Cost of the distinct sketch next to the count it sizes: device time (HIP events on the context's stream, median of
--reps after one warm-up) of cfrk_distinct_sketch_device over R synthetic 150 bp reads, beside the device time of
counting the same reads (cfrk_global_last_add_ms, a job begun with the sketch's own hint) and of
cfrk_global_query_reads_device over them, in one process and one library, at k = 15, k = 31 canonical and k = 63, for
reads of a genome of R bases (configs[2]'s shape) and for uniform random reads (all-distinct).  One JSON line per case
on stdout (and appended to --out); the claim under test is sketch_ms < count_ms.

  python tools/bench_sketch.py [--reads R] [--reps N] [--out FILE] [--abl-lib tools/_bin/libcfrk_hip_abl.so]

--abl-lib: load the ablation build instead (make -C cfrk_amd/csrc abl) and time the other LDS layouts of the sketch
kernel as well: one word per register with a read before the atomic max (0x200000), and with the atomic max issued
for every window (0x400000).  They sketch right; only their time is of interest.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(15, 0), (31, 2), (63, 0)]                     # (k, flags): 2 = CFRK_CANONICAL
VARIANTS = [("bytes_cas", 0), ("words_read_first", 0x200000), ("words_always_atomic", 0x400000)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--L", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--abl-lib", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    import cfrk_amd
    from cfrk_amd import lib
    if a.abl_lib:
        lib._SO = os.path.abspath(a.abl_lib)
    L_ = cfrk_amd.load_library()
    stream = torch.cuda.Stream()
    ctx = cfrk_amd.Context(0, stream=stream.cuda_stream)
    R, L = a.reads, a.L
    nN = R * (L + 1)
    d, d_regs, d_out = ctx.alloc(nN + 64), ctx.alloc(cfrk_amd.CFRK_SKETCH_REGS), ctx.alloc(nN * 4 + 64)
    zeros = np.zeros(cfrk_amd.CFRK_SKETCH_REGS, np.uint8)

    def event_ms(fn):
        fn()                                            # warm-up (code objects, pool buffers)
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts), min(ts)

    lines = []
    for uniform in (False, True):
        ctx.synth_reads_device(0, R, L, R, d, uniform=uniform)
        ctx.sync()
        for k, flags in CASES:
            res = {"tool": "bench_sketch", "reads": R, "L": L, "k": k, "canonical": bool(flags), "uniform": uniform,
                   "genome": None if uniform else R, "reps": a.reps, "library": "ablation build" if a.abl_lib else "product"}
            for name, bit in (VARIANTS if a.abl_lib else VARIANTS[:1]):
                ctx.check(L_.cfrk_debug_set_flags(ctx._h, bit), "cfrk_debug_set_flags")
                ctx.h2d(d_regs, zeros)
                med, best = event_ms(lambda: ctx.distinct_sketch_device(d, nN, k, flags, d_regs, want_windows=False))
                key = "sketch" if bit == 0 else "sketch_" + name
                res[key + "_ms"], res[key + "_min_ms"] = round(med, 3), round(best, 3)
            ctx.check(L_.cfrk_debug_set_flags(ctx._h, 0), "cfrk_debug_set_flags")
            regs = np.empty(cfrk_amd.CFRK_SKETCH_REGS, np.uint8)
            ctx.d2h(regs, d_regs)
            res["windows"] = ctx.distinct_sketch_device(d, nN, k, flags, d_regs)
            res["estimate"], res["hint"] = round(cfrk_amd.sketch_estimate(regs)), cfrk_amd.sketch_hint(regs)
            res["sketch_gbases_per_s"] = round(nN / (res["sketch_ms"] * 1e-3) / 1e9, 1)
            ks = []
            for _ in range(1 + min(a.reps, 3)):
                g = cfrk_amd.GlobalCounter(ctx, k, flags, res["hint"])
                g.add_device(d, nN)
                ks.append(g.last_add_ms())
            res["count_ms"] = round(statistics.median(ks[1:]), 3)
            res["distinct"] = g.finish()
            res["estimate_rel_err"] = round(abs(res["estimate"] - res["distinct"]) / res["distinct"], 5)
            res["hint_covers_distinct"] = res["hint"] >= res["distinct"]
            med, best = event_ms(lambda: g.query_reads_device(d, nN, d_out))     # (the warm-up builds the index)
            res["query_reads_ms"] = round(med, 3)
            res["sketch_over_count"] = round(res["sketch_ms"] / res["count_ms"], 3)
            res["sketch_cheaper_than_count"] = res["sketch_ms"] < res["count_ms"]
            line = json.dumps(res)
            print(line, flush=True)
            lines.append(line)
    for p in (d, d_regs, d_out):
        ctx.free(p)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
