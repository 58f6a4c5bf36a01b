"""Cost of the read-only calls on one counted result: digest, the abundance histogram, the count-range export and the
full export, on configs[2]'s reads (10^8 synthetic 150 bp reads of a 10^8-base genome, k = 31 canonical; about 10^8
distinct keys in the one-word result list).

The reads are synthesised on the device (cfrk_synth_reads_device, as bench.py does) and counted once; every call is
then timed on that same result with a host clock around it (each call ends in a device synchronise; the host arrays are
allocated once, so first-touch page faults are not timed), median of --reps.  Kernel times come from running this under `rocprofv3 --kernel-trace --stats`.  Prints one JSON line.

  python tools/bench_spectrum.py [--reads R] [--k K] [--reps N] [--lib PATH] [--only export]

--lib loads another build of libcfrk_hip.so (a same-box A/B); --only export times digest and the full export alone,
which is all a build without the histogram has.
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
    ap.add_argument("--L", type=int, default=150)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--glen", type=int, default=0, help="genome length (default: = reads, as configs[2])")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nbins", type=int, default=16385)
    ap.add_argument("--lib", default="", help="another build of libcfrk_hip.so")
    ap.add_argument("--only", choices=["all", "export"], default="all")
    a = ap.parse_args()

    import numpy as np
    import cfrk_amd
    from cfrk_amd import lib as cl
    if a.lib:
        cl._SO = os.path.abspath(a.lib)
    ctx = cfrk_amd.Context(0)
    R, L, k = a.reads, a.L, a.k
    glen = a.glen or R
    nN = R * (L + 1)
    d = ctx.alloc(nN + 64)
    ctx.synth_reads_device(0, R, L, glen, d)
    hint = min(glen, R * (L - k + 1)) + 1024
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, hint)
    g.add_device(d, nN)
    ctx.sync()
    ctx.free(d)

    def timed(fn):
        fn()                                             # warm-up (pool buffers, sort temporaries, code objects)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = fn()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts) * 1e3, min(ts) * 1e3, out

    res = {"tool": "bench_spectrum", "reads": R, "L": L, "k": k, "glen": glen, "reps": a.reps,
           "lib": os.path.basename(cl._SO)}
    res["digest_ms"], res["digest_min_ms"], dg = timed(g.digest)
    res["distinct"], res["sum"] = dg[0], dg[1]
    if a.only == "all":
        res["histogram_ms"], res["histogram_min_ms"], h = timed(lambda: g.histogram(a.nbins))
        res["histogram_nbins"] = a.nbins
        res["histogram_sum_is_distinct"] = int(h.sum()) == dg[0]
        res["spectrum_head"] = [int(x) for x in h[:8]]
    Lib = cl.load_library()
    # host arrays allocated (and touched) once: the calls are timed, not the first-touch page faults of fresh arrays
    n = dg[0]
    lo, hi, cnt = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint32)

    def export_range(mn, mx):
        got = cl.C.c_uint64()
        rc = Lib.cfrk_global_export_range(ctx._h, mn, mx, cl._ptr(lo), cl._ptr(hi), cl._ptr(cnt), n, cl.C.byref(got))
        ctx.check(rc, "cfrk_global_export_range")
        return got.value

    if a.only == "all":
        res["export_range_2_ms"], res["export_range_2_min_ms"], m = timed(lambda: export_range(2, cfrk_amd.CFRK_COUNT_MAX))
        res["export_range_2_entries"] = m
        res["export_range_2_matches_histogram"] = m == int(h[2:].sum())
        res["export_range_gt100_ms"], res["export_range_gt100_min_ms"], m = timed(lambda: export_range(101, cfrk_amd.CFRK_COUNT_MAX))
        res["export_range_gt100_entries"] = m
        res["export_range_gt100_matches_histogram"] = m == int(h[101:].sum())

    def export_full():
        # cfrk_global_export itself (present in every build), sized by finish as GlobalCounter.export() does
        m = g.finish()
        got = cl.C.c_uint64()
        ctx.check(Lib.cfrk_global_export(ctx._h, cl._ptr(lo), cl._ptr(hi), cl._ptr(cnt), m, cl.C.byref(got)),
                  "cfrk_global_export")
        return got.value

    res["export_ms"], res["export_min_ms"], m = timed(export_full)
    res["export_entries"] = m
    res["export_sum_matches_digest"] = int(cnt[:m].astype(np.uint64).sum()) == dg[1]
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
