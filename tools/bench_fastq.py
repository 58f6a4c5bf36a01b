"""FASTQ parse on the device (cfrk_fastq_parse_device) against the host FASTQ parser and against the device FASTA parser
on the same reads, in one process.

The reads are those of tools/bench_e2e.py (10^7 synthetic reads of 150 bases by default).  Their FASTQ image is
`@rNNNNNNNNN\\n<bases>\\n+\\n<qualities>\\n` with seeded qualities, of which about one in twelve lies below 20; their FASTA
image is `>rNNNNNNNNN\\n<bases>\\n`.  Measured, each with one warm-up and the median of 5 [min, max]:
  device FASTQ parse at min_qual 0 and 20, and the device FASTA parse, ALTERNATING in the same process
  cfrk_host_parse_fastq with 16 threads at min_qual 0 and 20
Every time is HOST WALL CLOCK around the call and a stream synchronisation, as in bench_ingest.py (the FASTQ call
synchronises twice itself).  The byte floor is DESIGN 4.11's: the text twice (a reduce and a scatter pass; with
min_qual > 0 a third time, the masking pass), the codes and the tables once, at the 6.29 TB/s copy ceiling.
The device results are checked against the host parser's (nN, nS, and the codes through a k = 31 job digest).
One JSON line per measurement on stdout."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cfrk_amd  # noqa: E402

COPY_CEILING = 6.29e12


class Batch(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_int8)), ("start", C.POINTER(C.c_int64)),
                ("length", C.POINTER(C.c_int32)), ("nN", C.c_int64), ("nS", C.c_int64)]


def spread(xs):
    return {"median": round(statistics.median(xs), 6), "min": round(min(xs), 6), "max": round(max(xs), 6)}


def images(ctx, R, L, glen):
    """-> (FASTQ image, FASTA image) of reads [0, R) of the generator, as uint8 arrays"""
    nN = R * (L + 1)
    d = ctx.alloc(nN + 64)
    ctx.synth_reads_device(0, R, L, glen, d)
    codes = np.empty(nN, np.int8)
    ctx.d2h(codes, d)
    ctx.free(d)
    bases = np.frombuffer(b"ACGT", np.uint8)[codes.reshape(R, L + 1)[:, :L]]
    del codes
    name = np.empty((R, 12), np.uint8)
    name[:, 1] = ord("r"); name[:, 11] = ord("\n")
    idx = np.arange(R, dtype=np.int64)
    for j in range(9):
        name[:, 10 - j] = (idx % 10 + ord("0")).astype(np.uint8)
        idx //= 10
    fa = np.empty((R, 12 + L + 1), np.uint8)
    fa[:, :12] = name; fa[:, 0] = ord(">"); fa[:, 12:12 + L] = bases; fa[:, -1] = ord("\n")
    fq = np.empty((R, 12 + L + 1 + 2 + L + 1), np.uint8)
    fq[:, :12] = name; fq[:, 0] = ord("@"); fq[:, 12:12 + L] = bases
    fq[:, 12 + L] = ord("\n"); fq[:, 13 + L] = ord("+"); fq[:, 14 + L] = ord("\n"); fq[:, -1] = ord("\n")
    # 24 quality values, two of them below 20: one base in twelve is masked at min_qual 20
    lut = np.frombuffer(b"#+5678:;<=>?@ABCDEFGHIII", np.uint8)
    rng = np.random.default_rng(1)
    for r0 in range(0, R, 1 << 20):                       # (in pieces: the index array is the generator's largest)
        r1 = min(R, r0 + (1 << 20))
        fq[r0:r1, 15 + L:15 + 2 * L] = lut[rng.integers(0, len(lut), (r1 - r0, L), dtype=np.uint8)]
    return fq.reshape(-1), fa.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ctx = cfrk_amd.Context(0)
    L = 150
    fq, fa = images(ctx, a.reads, L, a.reads)
    H = C.CDLL(os.path.join(ROOT, "cfrk_amd", "libcfrk_host.so"))
    H.cfrk_host_parse_fastq.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(Batch), C.POINTER(C.c_uint64)]
    H.cfrk_host_free_batch.argtypes = [C.POINTER(Batch)]
    H.cfrk_host_set_parse_threads(a.threads)
    nS, nN = a.reads, a.reads * (L + 1)
    d_fq, d_fa = ctx.alloc(fq.size + 64), ctx.alloc(fa.size + 64)
    d_data, d_start, d_length = ctx.alloc(nN + 64), ctx.alloc(nS * 8), ctx.alloc(nS * 4)
    t0 = time.perf_counter(); ctx.h2d(d_fq, fq); fq_h2d = time.perf_counter() - t0
    t0 = time.perf_counter(); ctx.h2d(d_fa, fa); fa_h2d = time.perf_counter() - t0

    # host parser, and the digests the device results must reproduce
    host, want = {}, {}
    for q in (0, 20):
        times = []
        for i in range(a.reps + 1):
            b, where = Batch(), C.c_uint64()
            t0 = time.perf_counter()
            rc = H.cfrk_host_parse_fastq(fq.ctypes.data, fq.size, q, C.byref(b), C.byref(where))
            dt = time.perf_counter() - t0
            assert rc == 0 and (b.nN, b.nS) == (nN, nS), (rc, where.value, b.nN, b.nS)
            if i:
                times.append(dt)
            if i == a.reps:
                ctx.h2d(d_data, np.ctypeslib.as_array(b.data, (nN,)))
                g = cfrk_amd.GlobalCounter(ctx, 31, cfrk_amd.CFRK_CANONICAL, 1 << 26)
                g.add_device(d_data, nN)
                want[q] = g.digest()
            H.cfrk_host_free_batch(C.byref(b))
        host[q] = times

    forms = {"fastq_q0": lambda: ctx.parse_fastq_device(d_fq, fq.size, 0, d_data, nN, d_start, d_length, nS),
             "fastq_q20": lambda: ctx.parse_fastq_device(d_fq, fq.size, 20, d_data, nN, d_start, d_length, nS),
             "fasta": lambda: ctx.parse_fasta_device(d_fa, fa.size, 0, d_data, nN, d_start, d_length, nS)}
    times = {k: [] for k in forms}
    for i in range(a.reps + 1):                           # (round 0 warms up)
        for name, fn in forms.items():
            ctx.sync()
            t0 = time.perf_counter()
            got = fn()
            ctx.sync()
            dt = time.perf_counter() - t0
            assert got == (nN, nS), (name, got)
            if i:
                times[name].append(dt)
            if i == a.reps and name != "fasta":
                g = cfrk_amd.GlobalCounter(ctx, 31, cfrk_amd.CFRK_CANONICAL, 1 << 26)
                g.add_device(d_data, nN)
                q = 0 if name == "fastq_q0" else 20
                assert g.digest() == want[q], (name, "the device-parsed codes differ from the host parser's")
    base = {"reads": a.reads, "read_length": L, "nN": nN, "nS": nS, "reps": a.reps}
    for name, text, passes in (("fastq_q0", fq, 2), ("fastq_q20", fq, 3), ("fasta", fa, 2)):
        floor = (passes * text.size + nN + 12 * nS) / COPY_CEILING
        med = statistics.median(times[name])
        print(json.dumps(dict(base, what="device_parse", form=name, text_bytes=int(text.size), seconds=spread(times[name]),
                              ms=round(med * 1e3, 3), text_GBps=round(text.size / med / 1e9, 1), byte_floor_ms=round(floor * 1e3, 3),
                              times_byte_floor=round(med / floor, 2), digest_equals_host=name != "fasta" or None)), flush=True)
    for q in (0, 20):
        med = statistics.median(host[q])
        print(json.dumps(dict(base, what="host_parse", form=f"fastq_q{q}", threads=a.threads, text_bytes=int(fq.size), seconds=spread(host[q]),
                              ms=round(med * 1e3, 3), text_GBps=round(fq.size / med / 1e9, 2))), flush=True)
    print(json.dumps(dict(base, what="text_h2d", fastq_s=round(fq_h2d, 4), fasta_s=round(fa_h2d, 4))), flush=True)
    for p in (d_fq, d_fa, d_data, d_start, d_length):
        ctx.free(p)
    ctx.close()


if __name__ == "__main__":
    main()
