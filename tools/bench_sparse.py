"""Cost of the per-read sparse form (cfrk_per_read_sparse_device) on synthetic reads generated on the device.

Every case is timed with HIP events on the context's stream around the call (torch.cuda.Event on a torch stream the
context launches on), one warm-up call, then the median of --reps calls, all in this one process.  Per case, one JSON
line: reads/s, windows/s, nnz, the time as a multiple of the byte floor (input bytes + 12 * nnz + 8 * nS) / 6.29 TB/s
(the copy ceiling DESIGN.md uses), and the shares of the three stages, taken from three timings of the same input:
  skeleton = a sizes-only call that is told nN = 0 (every read is then out of range and gets an empty row): the pass
             over start / length, the row-pointer scan and the read-back of nnz, without any counting;
  sizes    = the sizes-only call (count pass + scan);      full = the call with room for every entry.
  count share = (sizes - skeleton) / full, scan share = skeleton / full, compaction share = (full - sizes) / full.
At k = 8 the parent's cfrk_per_read_dense_device is timed on the first --dense-reads of the same reads (an nS whose
dense matrix fits: 16384 reads are 4 GiB at k = 8) next to the sparse call on those same reads.

  python tools/bench_sparse.py [--reps N] [--out FILE] [--quick]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_CEILING = 6.29e12      # bytes/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dense-reads", type=int, default=16384)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    ap.add_argument("--quick", action="store_true", help="10^5 reads only (a rehearsal)")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")

    import numpy as np
    import torch
    import cfrk_amd

    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    ctx = cfrk_amd.Context(0, stream.cuda_stream)

    def timed(fn):
        fn()                                                # warm-up (code objects, pool buffers)
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms)

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    cases = [(100_000, 150, (8, 21, 31))] if a.quick else \
            [(1_000_000, 150, (8, 21, 31)), (10_000_000, 150, (8, 21, 31)), (100_000, 2000, (31,))]
    for R, L, ks in cases:
        nN = R * (L + 1)
        d_data, d_start, d_length, d_row = ctx.alloc(nN + 64), ctx.alloc(R * 8), ctx.alloc(R * 4), ctx.alloc((R + 1) * 8)
        ctx.synth_reads_device(0, R, L, max(R, 10 * L), d_data, d_start, d_length)
        ctx.sync()
        for k in ks:
            room = R * (L - k + 1)                          # the window bound
            d_keys, d_counts = ctx.alloc(room * 8), ctx.alloc(room * 4)
            nnz = ctx.per_read_sparse_device(d_data, d_start, d_length, nN, R, k, 0, d_row, d_keys, d_counts, room)

            def sizes_only(nn=nN):
                try:
                    ctx.per_read_sparse_device(d_data, d_start, d_length, nn, R, k, 0, d_row, 0, 0, 0)
                except cfrk_amd.CfrkError as e:
                    if e.code != cfrk_amd.CFRK_ERR_SMALL_BUF:
                        raise

            full_ms, full_min = timed(lambda: ctx.per_read_sparse_device(d_data, d_start, d_length, nN, R, k, 0, d_row,
                                                                         d_keys, d_counts, room))
            sizes_ms, _ = timed(sizes_only)
            skel_ms, _ = timed(lambda: sizes_only(0))
            floor_ms = (nN + 12 * nnz + 8 * R) / COPY_CEILING * 1e3
            res = {"tool": "bench_sparse", "reads": R, "L": L, "k": k, "flags": 0, "reps": a.reps, "nnz": nnz,
                   "windows": room, "ms": full_ms, "min_ms": full_min, "sizes_only_ms": sizes_ms, "skeleton_ms": skel_ms,
                   "reads_per_s": R / (full_ms * 1e-3), "windows_per_s": room / (full_ms * 1e-3),
                   "byte_floor_ms": floor_ms, "time_over_byte_floor": full_ms / floor_ms,
                   "share_count": max(sizes_ms - skel_ms, 0.0) / full_ms, "share_scan": skel_ms / full_ms,
                   "share_compact": max(full_ms - sizes_ms, 0.0) / full_ms}
            ctx.sync()
            ctx.free(d_keys)
            ctx.free(d_counts)
            if k == 8:
                # the dense call on an nS whose matrix fits, and the sparse call on exactly those reads
                nd = min(a.dense_reads, R)
                ndN = nd * (L + 1)
                d_freq = ctx.alloc(nd * 4 ** k * 4)
                dense_ms, _ = timed(lambda: ctx.check(ctx._L.cfrk_per_read_dense_device(
                    ctx._h, d_data, d_start, d_length, ndN, nd, k, 0, d_freq), "cfrk_per_read_dense_device"))
                ctx.sync()
                ctx.free(d_freq)
                room_d = nd * (L - k + 1)
                dk, dc = ctx.alloc(room_d * 8), ctx.alloc(room_d * 4)
                sp_ms, _ = timed(lambda: ctx.per_read_sparse_device(d_data, d_start, d_length, ndN, nd, k, 0, d_row, dk, dc,
                                                                    room_d))
                ctx.sync()
                ctx.free(dk)
                ctx.free(dc)
                res.update({"dense_reads": nd, "dense_ms": dense_ms, "sparse_same_reads_ms": sp_ms,
                            "dense_bytes_written": nd * 4 ** k * 4, "sparse_not_slower_than_dense": sp_ms <= dense_ms})
            emit(res)
        ctx.sync()
        for b in (d_data, d_start, d_length, d_row):
            ctx.free(b)
    ctx.close()


if __name__ == "__main__":
    main()
