"""Cost of the read filter against one counted result: cfrk_global_read_spans_device against
cfrk_global_read_stats_device (the same lookups, with the median select instead of the run monoid), and
cfrk_reads_select_device against a plain device-to-device copy that moves the same number of bytes (in plus out), on
the same reads in the same process.

The result is configs[2]'s (10^8 synthetic 150 bp reads of a 10^8-base genome, canonical), the reads synthesised on the
device and counted once; the filtered reads are the first --query-reads of them.  The context runs on a torch stream
so that every call is timed with device events on its own stream; after a warm-up the calls of a pair alternate;
median, min and max of --reps.  select_reads_device synchronises once inside the call (the sizes): that wait is part
of its time.  --long-read times the select of --query-reads short reads with and without one read of 10^6 bases among
them (no job needed).  Appends one JSON line to --out and prints it.

  python tools/bench_filter.py [--reads R] [--query-reads Q] [--L L] [--k K] [--reps N] [--out FILE] [--long-read]
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
    ap.add_argument("--reads", type=int, default=100_000_000)
    ap.add_argument("--query-reads", type=int, default=10_000_000)
    ap.add_argument("--L", type=int, default=150)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "bench_filter.jsonl"))
    ap.add_argument("--long-read", action="store_true")
    a = ap.parse_args()

    import numpy as np
    import torch
    import cfrk_amd
    stream = torch.cuda.Stream()
    ctx = cfrk_amd.Context(0, stream.cuda_stream)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def alternate(calls):
        ts = {n: [] for n in calls}
        for fn in calls.values():                            # warm-up (code objects, pool buffers)
            fn()
            ctx.sync()
        for _ in range(a.reps):
            for n, fn in calls.items():
                ts[n].append(timed(fn))
        return {n: {"ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)} for n, t in ts.items()}

    def d2d(nbytes):
        src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        src.zero_()
        torch.cuda.synchronize()

        def fn():
            with torch.cuda.stream(stream):
                dst.copy_(src)
        return fn

    L, Q = a.L, min(a.query_reads, a.reads)
    qN = Q * (L + 1)
    res = {"tool": "bench_filter", "L": L, "query_reads": Q, "reps": a.reps}
    if a.long_read:
        # Q short reads, then the same with one read of 10^6 bases in the middle: whole reads, nothing dropped
        res["case"] = "long_read"
        rng = np.random.default_rng(1)
        for name, big in (("short_only", 0), ("with_long_read", 1_000_000)):
            length = np.full(Q + (1 if big else 0), L, np.int32)
            if big:
                length[Q // 2] = big
            start = np.concatenate([[0], np.cumsum(length.astype(np.int64) + 1)[:-1]]).astype(np.int64)
            nN = int(start[-1]) + int(length[-1]) + 1
            data = rng.integers(0, 4, nN, dtype=np.int8)
            data[start + length] = -1
            nS = len(length)
            d, ds, dl = ctx.alloc(nN + 64), ctx.alloc(nS * 8), ctx.alloc(nS * 4)
            od, os_, ol = ctx.alloc(nN + 64), ctx.alloc(nS * 8), ctx.alloc(nS * 4)
            ctx.h2d(d, data); ctx.h2d(ds, start); ctx.h2d(dl, length)
            sel = lambda: ctx.select_reads_device(d, ds, dl, nN, nS, 0, 0, 0, od, nN, os_, ol, 0, nS)
            assert sel() == (nN, nS)
            back = np.empty(nN, np.int8)
            ctx.d2h(back, od)
            r = alternate({"select": sel, "d2d": d2d(nN)})
            res[name] = {"nN": nN, "nS": nS, "same": bool((back == data).all()), **{n + "_" + f: v for n, t in r.items() for f, v in t.items()}}
            for p in (d, ds, dl, od, os_, ol):
                ctx.free(p)
    else:
        R, k = a.reads, a.k
        nN = R * (L + 1)
        d = ctx.alloc(nN + 64)
        d_start, d_length = ctx.alloc(R * 8), ctx.alloc(R * 4)
        ctx.synth_reads_device(0, R, L, R, d, d_start, d_length)
        g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, min(R, R * (L - k + 1), 4 ** min(k, 31)) + 1024)
        g.add_device(d, nN)
        ctx.sync()
        res.update({"case": "spans_and_select", "reads": R, "k": k, "distinct": g.digest()[0]})
        g.query(np.zeros(1, np.uint64), np.zeros(1, np.uint64) if k > 32 else None)          # the index build
        d_rows, d_span = ctx.alloc(Q * 32), ctx.alloc(Q * 8)
        r = alternate({"read_stats": lambda: g.read_stats_device(d, d_start, d_length, qN, Q, 2, d_rows),
                       "read_spans": lambda: g.read_spans_device(d, d_start, d_length, qN, Q, 2, cfrk_amd.CFRK_COUNT_MAX,
                                                                 cfrk_amd.CFRK_SPAN_LONGEST, d_span)})
        res["spans"] = r
        spread = r["read_stats"]["max_ms"] - r["read_stats"]["min_ms"]
        res["spans_within_spread_of_read_stats"] = r["read_spans"]["ms"] <= r["read_stats"]["ms"] + spread
        spans = np.empty(Q, cfrk_amd.READ_SPAN_DTYPE)
        ctx.d2h(spans, d_span)
        res["span_bases_mean"] = float(spans["length"].mean())
        od, os_, ol, oi = ctx.alloc(qN + 64), ctx.alloc(Q * 8), ctx.alloc(Q * 4), ctx.alloc(Q * 8)
        for name, sp, min_len in (("select_whole", 0, 0), ("select_longest", d_span, k)):
            sel = lambda: ctx.select_reads_device(d, d_start, d_length, qN, Q, sp, 0, min_len, od, qN, os_, ol, oi, Q)
            n2, s2 = sel()
            # the plain copy moves the kept bytes once in and once out; the select also reads start / length / span in its
            # two per-read passes and writes start / length / index and the kept reads' source offsets
            t = alternate({"select": sel, "d2d": d2d(n2)})
            res[name] = {"nN_out": n2, "nS_out": s2, **{n + "_" + f: v for n, tt in t.items() for f, v in tt.items()}}
            res[name]["ratio_to_d2d"] = t["select"]["ms"] / t["d2d"]["ms"]
            res[name]["select_GBps_in_plus_out"] = 2 * n2 / (t["select"]["ms"] * 1e-3) / 1e9
        for p in (d_rows, d_span, od, os_, ol, oi, d, d_start, d_length):
            ctx.free(p)
    ctx.close()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
