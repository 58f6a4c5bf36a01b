"""Cost of per-read abundance statistics against one counted result: cfrk_global_read_stats_device against the route
callers had before it, cfrk_global_query_reads_device (4 bytes per base out, reduced by the caller), on the same reads
of the same result in the same process.

The result is configs[2]'s (10^8 synthetic 150 bp reads of a 10^8-base genome, k = 31 canonical), the reads
synthesised on the device (cfrk_synth_reads_device, as bench.py does) and counted once; the query reads are the first
--query-reads of them.  The two calls alternate, each timed with a host clock around call + device synchronise after a
warm-up; median, min and max of --reps.  Kernel times come from running this under `rocprofv3 --kernel-trace --stats`.
Prints one JSON line.

  python tools/bench_read_stats.py [--reads R] [--query-reads Q] [--L L] [--k K] [--reps N] [--threshold T]

--k 63 is the two-word index, --k 12 the dense one (counted by the radix path); --L 1000 puts every read in the upper
half of the fast path (the 64-lane groups); use fewer reads with it (e.g. --reads 15000000 --query-reads 1500000).
within_bar: read_stats median <= query_reads median + (max - min) of the query_reads reps.
A sample of the rows is checked against the windows' counts that query_reads_device wrote for the same reads.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000_000)
    ap.add_argument("--query-reads", type=int, default=10_000_000)
    ap.add_argument("--L", type=int, default=150)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--threshold", type=int, default=2)
    a = ap.parse_args()

    import numpy as np
    import cfrk_amd
    ctx = cfrk_amd.Context(0)
    R, L, k, Q = a.reads, a.L, a.k, min(a.query_reads, a.reads)
    glen = R
    nN = R * (L + 1)
    qN = Q * (L + 1)
    d = ctx.alloc(nN + 64)
    d_start, d_length = ctx.alloc(R * 8), ctx.alloc(R * 4)
    ctx.synth_reads_device(0, R, L, glen, d, d_start, d_length)
    hint = min(glen, R * (L - k + 1), 4 ** min(k, 31)) + 1024
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, hint)
    g.add_device(d, nN)
    ctx.sync()
    dg = g.digest()
    res = {"tool": "bench_read_stats", "reads": R, "L": L, "k": k, "glen": glen, "reps": a.reps, "distinct": dg[0],
           "query_reads": Q, "threshold": a.threshold}
    t0 = time.perf_counter()
    g.query(np.zeros(1, np.uint64), np.zeros(1, np.uint64) if k > 32 else None)
    res["index_build_ms"] = (time.perf_counter() - t0) * 1e3

    d_rows = ctx.alloc(Q * 32)
    d_ans = ctx.alloc(qN * 4 + 64)
    calls = {"read_stats": lambda: g.read_stats_device(d, d_start, d_length, qN, Q, a.threshold, d_rows),
             "query_reads": lambda: g.query_reads_device(d, qN, d_ans)}
    ts = {n: [] for n in calls}
    for fn in calls.values():                            # warm-up (code objects)
        fn()
        ctx.sync()
    for _ in range(a.reps):                              # alternating
        for n, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            ts[n].append((time.perf_counter() - t0) * 1e3)
    for n, t in ts.items():
        res[n + "_ms"], res[n + "_min_ms"], res[n + "_max_ms"] = statistics.median(t), min(t), max(t)
    valid = Q * (L - k + 1)
    res["valid_windows"] = valid
    res["read_stats_lookups_per_s"] = valid / (res["read_stats_ms"] * 1e-3)
    res["bytes_out_read_stats"], res["bytes_out_query_reads"] = Q * 32, qN * 4
    spread = res["query_reads_max_ms"] - res["query_reads_min_ms"]
    res["bar_ms"] = res["query_reads_ms"] + spread
    res["within_bar"] = res["read_stats_ms"] <= res["bar_ms"]

    # sample check: the first rows against the windows' counts query_reads_device wrote
    m = min(Q, 20000)
    rows = np.empty(m, cfrk_amd.READ_STATS_DTYPE)
    ans = np.empty(m * (L + 1), np.uint32)
    ctx.d2h(rows, d_rows)
    ctx.d2h(ans, d_ans)
    c = np.sort(ans.reshape(m, L + 1)[:, :L - k + 1].astype(np.uint64), axis=1)      # (synthetic reads: every window valid)
    ok = bool((c != cfrk_amd.CFRK_QUERY_NONE).all())
    ok &= bool((rows["windows"] == c.shape[1]).all() and (rows["min"] == c[:, 0]).all() and (rows["max"] == c[:, -1]).all())
    ok &= bool((rows["median"] == c[:, (c.shape[1] - 1) // 2]).all() and (rows["sum"] == c.sum(axis=1)).all())
    ok &= bool((rows["present"] == (c >= 1).sum(axis=1)).all() and (rows["below"] == (c < a.threshold).sum(axis=1)).all())
    res["sample_rows"], res["sample_ok"] = m, ok
    res["sample_median_of_medians"] = float(np.median(rows["median"]))
    for p in (d_rows, d_ans, d, d_start, d_length):
        ctx.free(p)
    ctx.close()
    print(json.dumps(res))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
