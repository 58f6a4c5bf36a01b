"""Cost of point queries on one counted result: the index build, cfrk_global_query_reads_device over 10^7 of the counted
reads and cfrk_global_query_device over 10^8 keys (half present, half absent), against a CFRK_FORCE_HASH count of the
same 10^7 reads (one HBM atomic per window into a table of similar size).

The result is configs[2]'s (10^8 synthetic 150 bp reads of a 10^8-base genome, k = 31 canonical), the reads
synthesised on the device (cfrk_synth_reads_device, as bench.py does) and counted once.  Calls are timed with a host
clock around call + device synchronise, median of --reps; the index build is the first query's time (it happens once
per result).  Kernel times come from running this under `rocprofv3 --kernel-trace --stats`.  Prints one JSON line.

  python tools/bench_query.py [--reads R] [--query-reads Q] [--keys N] [--k K] [--reps N]

line_traffic_gb_est: one 128-byte index line per valid window (a probe that goes on past its first slot mostly stays
in that line: 8 slots of 16 B), plus the reads (1 B per base) and the answers (4 B per base) -- an estimate from
shapes, not a counter reading.
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
    ap.add_argument("--keys", type=int, default=100_000_000)
    ap.add_argument("--L", type=int, default=150)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()

    import numpy as np
    import cfrk_amd
    ctx = cfrk_amd.Context(0)
    R, L, k, Q = a.reads, a.L, a.k, min(a.query_reads, a.reads)
    glen = R
    nN = R * (L + 1)
    qN = Q * (L + 1)
    d = ctx.alloc(nN + 64)
    ctx.synth_reads_device(0, R, L, glen, d)
    hint = min(glen, R * (L - k + 1)) + 1024
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, hint)
    g.add_device(d, nN)
    ctx.sync()
    dg = g.digest()

    def timed(fn):
        fn()                                             # warm-up (code objects, pool buffers)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts) * 1e3, min(ts) * 1e3

    res = {"tool": "bench_query", "reads": R, "L": L, "k": k, "glen": glen, "reps": a.reps, "distinct": dg[0]}
    # index build: the first query of the result (resolve + scan + build + one lookup)
    t0 = time.perf_counter()
    g.query(np.zeros(1, np.uint64))
    res["index_build_ms"] = (time.perf_counter() - t0) * 1e3
    res["index_bytes"] = (1 << max(10, (2 * dg[0] - 1).bit_length())) * 16

    # read query over the first Q counted reads
    out = ctx.alloc(qN * 4 + 64)
    res["query_reads"] = Q
    res["query_reads_windows"] = qN
    res["query_reads_ms"], res["query_reads_min_ms"] = timed(lambda: g.query_reads_device(d, qN, out))
    valid = Q * (L - k + 1)
    res["query_reads_valid_windows"] = valid
    res["lookups_per_s"] = valid / (res["query_reads_ms"] * 1e-3)
    traffic = valid * 128 + qN * 5
    res["line_traffic_gb_est"] = traffic / 1e9
    res["line_traffic_tb_s_est"] = traffic / (res["query_reads_ms"] * 1e-3) / 1e12
    # sample check: no valid window of a counted read answers 0
    m = min(qN, 1 << 24)
    ans = np.empty(m, np.uint32)
    ctx.d2h(ans, out)
    v = ans[ans != cfrk_amd.CFRK_QUERY_NONE]
    res["sample_windows"], res["sample_valid"], res["sample_valid_zero"] = m, int(len(v)), int((v == 0).sum())
    ctx.free(out)

    # key query: half present (result keys), half absent (random 62-bit keys), shuffled
    lo, _, cnt = g.export()
    n = min(a.keys, 2 * len(lo))
    rng = np.random.default_rng(1)
    half = n // 2
    keys = np.concatenate([lo[rng.integers(0, len(lo), half)],
                           rng.integers(0, 1 << 62, n - half, dtype=np.uint64) & np.uint64((1 << (2 * k)) - 1)])
    present = np.zeros(n, bool)
    present[:half] = True
    perm = rng.permutation(n)
    keys, present = keys[perm], present[perm]
    del lo, cnt
    d_keys, d_out = ctx.alloc(n * 8), ctx.alloc(n * 4 + 64)
    ctx.h2d(d_keys, keys)
    res["query_keys"] = n
    res["query_keys_ms"], res["query_keys_min_ms"] = timed(lambda: g.query_device(d_keys, 0, n, d_out))
    res["keys_per_s"] = n / (res["query_keys_ms"] * 1e-3)
    got = np.empty(n, np.uint32)
    ctx.d2h(got, d_out)
    res["present_nonzero"] = bool((got[present] > 0).all())
    res["absent_zero_frac"] = float((got[~present] == 0).mean())
    ctx.free(d_keys)
    ctx.free(d_out)
    del keys, got, present

    # comparison: the general HBM-hash count of the same Q reads (one atomic per window, table of similar size)
    hint_q = min(glen, Q * (L - k + 1)) + 1024
    ts, ks = [], []
    for _ in range(a.reps + 1):
        h = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL | cfrk_amd.CFRK_FORCE_HASH, hint_q)
        ctx.sync()
        t0 = time.perf_counter()
        h.add_device(d, qN)
        ctx.sync()
        ts.append(time.perf_counter() - t0)
        ks.append(h.last_add_ms())
    res["force_hash_count_ms"] = statistics.median(ts[1:]) * 1e3
    res["force_hash_kernel_ms"] = statistics.median(ks[1:])
    res["query_reads_faster_than_force_hash"] = res["query_reads_ms"] < res["force_hash_count_ms"]
    ctx.free(d)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
