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

--paired: the cost of the pair join.  cfrk_global_normalize_pairs_device (the same reads taken as interleaved mates,
CFRK_PAIR_EITHER; CFRK_PAIR_BOTH as well, which keeps fewer reads than the unpaired rule where EITHER keeps more, so
that the join's cost can be told from the cost of inserting more or fewer reads) is timed beside the unpaired call -- whose kernels are the parent commit's, text for text -- at every
batch, alternating, in the same process; one line per call and batch, a line with the paired / unpaired ratio and the
unpaired call's own spread ((max - min) / median of its repetitions) per batch, and a verdict at 262 144: is the paired
call slower than the unpaired one by more than that spread?  The comparison calls are left out.

  python tools/bench_normalize.py [--reads R] [--L L] [--k K] [--cutoff C] [--reps N] [--batches B,B,...] [--out FILE] [--paired]
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
    ap.add_argument("--out", default=None)
    ap.add_argument("--paired", action="store_true")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "r23", "bench_normalize_pairs.jsonl") if a.paired else \
            os.path.join(ROOT, "profiles", "r21", "bench_normalize.jsonl")

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
    if a.paired:
        assert R % 2 == 0, "--paired takes an even number of reads"
        for B in [int(x) for x in a.batches.split(",")]:
            ts_u, (kept_u, _) = timed(fresh, lambda g, B=B: (g.normalize_device(d, d_start, d_length, nN, R, a.cutoff, d_keep, B), g))
            ts_p, (kept_p, _) = timed(fresh, lambda g, B=B: (g.normalize_pairs_device(d, d_start, d_length, nN, R, a.cutoff, d_keep, B,
                                                                                     cfrk_amd.CFRK_PAIR_EITHER), g))
            ts_b, (kept_b, _) = timed(fresh, lambda g, B=B: (g.normalize_pairs_device(d, d_start, d_length, nN, R, a.cutoff, d_keep, B,
                                                                                     cfrk_amd.CFRK_PAIR_BOTH), g))
            u = emit("normalize", ts_u, batch=B, kept=kept_u, rounds=-(-R // B))
            p_ = emit("normalize_pairs", ts_p, batch=B, kept=kept_p, rounds=-(-R // B), mode="either")
            emit("normalize_pairs", ts_b, batch=B, kept=kept_b, rounds=-(-R // B), mode="both")
            spread = (max(ts_u) - min(ts_u)) / u
            # the join alone: the launches a paired call adds, one per round, on the keep bytes the call left (in place)
            ts_j, _ = timed(lambda: None, lambda _, B=B: [ctx.pair_keep_device(min(B, R - off) // 2, 2, cfrk_amd.CFRK_PAIR_EITHER, 0,
                                                                                d_keep + off, d_keep + off + 1, 0, 0, 0, 0, d_keep + off,
                                                                                d_keep + off + 1, want_counts=False)
                                                          for off in range(0, R, B)])
            emit("joins_alone", ts_j, batch=B, rounds=-(-R // B))
            row = dict(base, what="ratio", batch=B, kept_ratio=kept_p / kept_u, paired_over_unpaired=p_ / u, unpaired_spread=spread, extra_ms=p_ - u,
                       extra_us_per_round=1000.0 * (p_ - u) / -(-R // B), beyond_spread=(p_ - u) / u > spread)
            lines.append(row)
            print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))
        for p in (d, d_start, d_length, d_keep, d_rows):
            ctx.free(p)
        ctx.close()
        return 0
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
