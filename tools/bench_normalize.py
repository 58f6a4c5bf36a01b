"""Cost of digital normalisation on the device: cfrk_global_normalize_device over a sweep of batch_reads, against the
two calls whose work it combines, on the same reads in the same process:
  read_stats   cfrk_global_read_stats_device of the reads on a finished job of them: the judge's lookups, against the
               query index instead of the live table (with the median select the judge does without)
  add_hash     cfrk_global_add_device of the reads under CFRK_FORCE_HASH: the insert's atomics if every read were kept

The reads are bench.py's C3 shape (synthetic 150 bp reads of a genome as long as there are reads: coverage 150),
synthesised on the device; k = 31 canonical, cutoff 20.  Every call is timed with device events on the context's stream
(a fresh job per normalise / add repetition, begun before the first event), after a warm-up of each shape; median, min
and max of --reps.  One JSON line per measurement to --out, and a closing line with the expectation under test: at a
large batch the call costs no more than the two comparison calls together.

  python tools/bench_normalize.py [--reads R] [--L L] [--k K] [--cutoff C] [--reps N] [--batches B,B,...] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--L", type=int, default=150)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--cutoff", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="4096,16384,65536,262144,1048576")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "bench_normalize.jsonl"))
    a = ap.parse_args()

    import torch
    import cfrk_amd
    stream = torch.cuda.Stream()                         # (a stream of its own: the events and the context share it)
    ctx = cfrk_amd.Context(0, stream=stream.cuda_stream)
    R, L, k = a.reads, a.L, a.k
    nN = R * (L + 1)
    flags = cfrk_amd.CFRK_CANONICAL
    hint = min(R, R * (L - k + 1), 4 ** min(k, 31)) + 1024
    d, d_start, d_length, d_keep = ctx.alloc(nN + 64), ctx.alloc(R * 8), ctx.alloc(R * 4), ctx.alloc(R)
    d_rows = ctx.alloc(R * 32)
    ctx.synth_reads_device(0, R, L, R, d, d_start, d_length)
    ctx.sync()
    lines = []
    base = {"tool": "bench_normalize", "reads": R, "L": L, "k": k, "cutoff": a.cutoff, "reps": a.reps, "genome": R}

    def timed(prepare, call):
        """device-event times of `call` (ms), each after its own `prepare`; the first repetition is the warm-up"""
        ts, last = [], None
        for rep in range(a.reps + 1):
            state = prepare()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            last = call(state)
            e1.record(stream)
            e1.synchronize()
            if rep:
                ts.append(e0.elapsed_time(e1))
        return ts, last

    def emit(what, ts, **more):
        row = dict(base, what=what, ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), all_ms=[round(t, 3) for t in ts], **more)
        lines.append(row)
        print(json.dumps(row), flush=True)
        return row["ms"]

    fresh = lambda: cfrk_amd.GlobalCounter(ctx, k, flags | cfrk_amd.CFRK_FORCE_HASH, hint)
    norm_ms = {}
    for B in [int(x) for x in a.batches.split(",")]:
        ts, (kept, g) = timed(fresh, lambda g, B=B: (g.normalize_device(d, d_start, d_length, nN, R, a.cutoff, d_keep, B), g))
        norm_ms[B] = emit("normalize", ts, batch=B, kept=kept, rounds=-(-R // B), distinct=g.finish())
    ts, _ = timed(fresh, lambda g: g.add_device(d, nN))
    add_ms = emit("add_hash", ts)
    g = cfrk_amd.GlobalCounter(ctx, k, flags, hint)
    g.add_device(d, nN)
    g.read_stats_device(d, d_start, d_length, nN, min(R, 1024), a.cutoff, d_rows)      # (builds the index)
    ctx.sync()
    ts, _ = timed(lambda: None, lambda _: g.read_stats_device(d, d_start, d_length, nN, R, a.cutoff, d_rows))
    stats_ms = emit("read_stats", ts)
    big = max(norm_ms)
    best = min(norm_ms, key=norm_ms.get)
    row = dict(base, what="verdict", batch=big, normalize_ms=norm_ms[big], read_stats_plus_add_hash_ms=stats_ms + add_ms,
               no_more_than_both=norm_ms[big] <= stats_ms + add_ms, fastest_batch=best, fastest_ms=norm_ms[best])
    lines.append(row)
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("".join(json.dumps(x) + "\n" for x in lines))
    for p in (d, d_start, d_length, d_keep, d_rows):
        ctx.free(p)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
