"""Cost and yield of the spectral correction against one counted result: cfrk_global_correct_reads_device against
cfrk_global_read_spans_device (the sibling that does the same lookups) and against the plain device-to-device copy of
`data` that the call contains, on the same reads in the same process.

The result is configs[2]'s (10^8 synthetic 150 bp reads of a 10^8-base genome, canonical), the reads synthesised on the
device and counted once; the corrected reads are the first --query-reads of them, in two forms: error-free as generated,
and with substitutions planted on the device at --error-rate per base.  The context runs on a torch stream so that every
call is timed with device events on its own stream; after a warm-up the calls alternate; median, min and max of --reps.
The yield is taken against the clean reads: of the planted errors, the fractions restored, left alone and miscorrected,
and the clean bases that were changed.  Appends one JSON line to --out and prints it.

  python tools/bench_correct.py [--reads R] [--query-reads Q] [--L L] [--k K] [--min-count T] [--error-rate E] [--reps N] [--out FILE]
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
    ap.add_argument("--min-count", type=int, default=2)
    ap.add_argument("--error-rate", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "bench_correct.jsonl"))
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

    R, L, k, Q = a.reads, a.L, a.k, min(a.query_reads, a.reads)
    nN, qN = R * (L + 1), Q * (L + 1)
    d = ctx.alloc(nN + 64)
    d_start, d_length = ctx.alloc(R * 8), ctx.alloc(R * 4)
    ctx.synth_reads_device(0, R, L, R, d, d_start, d_length)
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, min(R, R * (L - k + 1), 4 ** min(k, 31)) + 1024)
    g.add_device(d, nN)
    ctx.sync()
    res = {"tool": "bench_correct", "reads": R, "L": L, "k": k, "query_reads": Q, "min_count": a.min_count,
           "error_rate": a.error_rate, "reps": a.reps, "distinct": g.digest()[0]}
    g.query(np.zeros(1, np.uint64), np.zeros(1, np.uint64) if k > 32 else None)          # the index build

    # the query reads: the first Q of the counted reads; their clean form stays in d, the noisy form is a torch tensor
    with torch.cuda.stream(stream):
        noisy = torch.empty(qN + 64, dtype=torch.int8, device="cuda")
        out = torch.empty(qN + 64, dtype=torch.int8, device="cuda")
        t_start = torch.empty(Q, dtype=torch.int64, device="cuda")
        t_length = torch.empty(Q, dtype=torch.int32, device="cuda")
        ctx.synth_reads_device(0, Q, L, R, noisy.data_ptr(), t_start.data_ptr(), t_length.data_ptr())
        clean = noisy[:qN].clone()
        gen = torch.Generator(device="cuda")
        gen.manual_seed(22)
        planted = (torch.rand(qN, device="cuda", generator=gen) < a.error_rate) & (clean >= 0) & (clean < 4)
        shift = torch.randint(1, 4, (qN,), device="cuda", generator=gen, dtype=torch.int8)
        noisy[:qN] = torch.where(planted, (clean + shift) & 3, clean)
        del shift
        d_span = torch.empty(Q * 8, dtype=torch.uint8, device="cuda")
        d_fix = torch.empty(Q, 2, dtype=torch.int32, device="cuda")
    stream.synchronize()
    res["planted"] = int(planted.sum().item())

    def copy_of(src):
        def fn():
            with torch.cuda.stream(stream):
                out[:qN].copy_(src[:qN])
        return fn

    for name, src in (("error_free", clean), ("with_errors", noisy)):
        p = src.data_ptr()
        spans = lambda: g.read_spans_device(p, t_start.data_ptr(), t_length.data_ptr(), qN, Q, a.min_count, cfrk_amd.CFRK_COUNT_MAX,
                                            cfrk_amd.CFRK_SPAN_LONGEST, d_span.data_ptr())
        correct = lambda: g.correct_reads_device(p, t_start.data_ptr(), t_length.data_ptr(), qN, Q, a.min_count, out.data_ptr(),
                                                 d_fix.data_ptr())
        r = alternate({"read_spans": spans, "correct_reads": correct, "d2d": copy_of(src)})
        row = {n + "_" + f: v for n, t in r.items() for f, v in t.items()}
        row["ratio_to_read_spans"] = r["correct_reads"]["ms"] / r["read_spans"]["ms"]
        row["ratio_to_read_spans_plus_d2d"] = r["correct_reads"]["ms"] / (r["read_spans"]["ms"] + r["d2d"]["ms"])
        row["read_spans_spread_ms"] = r["read_spans"]["max_ms"] - r["read_spans"]["min_ms"]
        correct()                                            # (the copy that was timed last went to `out` too)
        ctx.sync()
        with torch.cuda.stream(stream):
            got = out[:qN]
            row["runs_fixed"] = int(d_fix[:, 0].to(torch.int64).sum().item())
            row["runs_left"] = int(d_fix[:, 1].to(torch.int64).sum().item())
            row["bases_changed"] = int((got != src[:qN]).sum().item())
            if name == "with_errors":
                n = max(res["planted"], 1)
                restored = int(((got == clean) & planted).sum().item())
                left = int(((got == noisy[:qN]) & planted).sum().item())
                row["errors_restored"] = restored / n
                row["errors_left_alone"] = left / n
                row["errors_miscorrected"] = (res["planted"] - restored - left) / n
                row["clean_bases_changed"] = int(((got != clean) & ~planted).sum().item())
        res[name] = row
    for ptr in (d, d_start, d_length):
        ctx.free(ptr)
    ctx.close()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
