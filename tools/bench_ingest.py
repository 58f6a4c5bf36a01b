"""FASTA parse on the device (cfrk_fasta_parse_device) against the host parser, in process and through the CLI.

  in process   the image of tools/bench_e2e.py (10^7 reads of 150 bases, 1.63 GB) is parsed on the device (warm-up, then
               5 runs) and by cfrk_host_parse_fasta with 16 threads.  Every time is HOST WALL CLOCK around the call and a
               stream synchronisation, not HIP events: the call reads its sizes back in its middle, so the figure holds
               that read-back and the last synchronisation and is an upper bound of the kernels' time;
               the text's and the codes' H2D copies are timed the same way; the byte floor is text x 2 + codes +
               tables at the 6.29 TB/s copy ceiling of DESIGN.md
  mapped file  the same file mapped (as the CLI maps it): cfrk_memcpy_h2d straight from the mapping against
               cfrk_memcpy_h2d_staged (the pinned ring --device-parse uses), alternating
  end to end   `cfrk --global --timing` without --device-parse and with it (--text-copy staged, --text-copy plain),
               alternating, 5 runs each, k = 15 and k = 31
  at scale     --scale-reads N (3.2e7 reads: 5.2 GB of text, offsets beyond 2^32): nN, nS and the k = 31 job digest of
               the two paths must be equal (asserted)
One JSON line per measurement on stdout."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_e2e  # noqa: E402
import cfrk_amd  # noqa: E402

COPY_CEILING = 6.29e12


class Batch(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_int8)), ("start", C.POINTER(C.c_int64)),
                ("length", C.POINTER(C.c_int32)), ("nN", C.c_int64), ("nS", C.c_int64)]


def host_lib(threads):
    L = C.CDLL(os.path.join(ROOT, "cfrk_amd", "libcfrk_host.so"))
    L.cfrk_host_parse_fasta.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(Batch)]
    L.cfrk_host_free_batch.argtypes = [C.POINTER(Batch)]
    L.cfrk_host_set_parse_threads(threads)
    return L


def spread(xs):
    return {"median": round(statistics.median(xs), 6), "min": round(min(xs), 6), "max": round(max(xs), 6)}


def timed(fn, reps=5, warm=1):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def in_process(ctx, text, threads, k=None):
    n = text.size
    H = host_lib(threads)
    b = Batch()

    def host_parse():
        if b.data:
            H.cfrk_host_free_batch(C.byref(b))
        rc = H.cfrk_host_parse_fasta(text.ctypes.data, n, 0, C.byref(b))
        assert rc == 0, rc

    host_s = timed(host_parse, reps=5, warm=1)
    nN, nS = b.nN, b.nS
    codes = np.ctypeslib.as_array(b.data, (nN,))
    d_text, d_data, d_start, d_length = ctx.alloc(n + 64), ctx.alloc(nN + 64), ctx.alloc(nS * 8), ctx.alloc(nS * 4)
    text_h2d = timed(lambda: ctx.h2d(d_text, text), reps=5, warm=1)
    codes_h2d = timed(lambda: ctx.h2d(d_data, codes), reps=5, warm=1)
    got = []

    def dev_parse():
        got[:] = ctx.parse_fasta_device(d_text, n, 0, d_data, nN, d_start, d_length, nS)
        ctx.sync()

    dev_s = timed(dev_parse, reps=5, warm=1)
    assert tuple(got) == (nN, nS), (got, nN, nS)
    floor = (2 * n + nN + 12 * nS) / COPY_CEILING
    res = {"what": "in_process", "text_bytes": int(n), "nN": int(nN), "nS": int(nS), "host_threads": threads,
           "host_parse_s": spread(host_s), "device_parse_s": spread(dev_s), "text_h2d_s": spread(text_h2d),
           "codes_h2d_s": spread(codes_h2d), "byte_floor_s": round(floor, 6),
           "device_parse_GBps": round(n / statistics.median(dev_s) / 1e9, 1),
           "host_path_s": round(statistics.median(host_s) + statistics.median(codes_h2d), 4),
           "device_path_s": round(statistics.median(dev_s) + statistics.median(text_h2d), 4)}
    if k:
        # same reads, same job: the digest of the device-parsed buffer against the host-parsed one
        g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, 1 << 26)
        g.add_device(d_data, nN)
        dev_digest = g.digest()
        ctx.h2d(d_data, codes)
        g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, 1 << 26)
        g.add_device(d_data, nN)
        host_digest = g.digest()
        assert dev_digest == host_digest, (dev_digest, host_digest)
        res["digest_equal"] = True
        res["distinct"] = int(dev_digest[0])
    H.cfrk_host_free_batch(C.byref(b))
    for p in (d_text, d_data, d_start, d_length):
        ctx.free(p)
    return res


def mapped_file_h2d(ctx, path):
    mm = np.memmap(path, np.uint8, "r")
    int(mm[::4096].sum())                                  # (every page touched: the CLI maps with MAP_POPULATE)
    d = ctx.alloc(mm.size + 64)
    plain, staged = [], []
    for i in range(6):
        for name, fn, acc in (("plain", ctx.h2d, plain), ("staged", ctx.h2d_staged, staged)):
            t0 = time.perf_counter()
            fn(d, mm)
            if i:
                acc.append(time.perf_counter() - t0)
    back = np.empty(1 << 20, np.uint8)
    ctx.d2h(back, d + mm.size - back.size)
    assert (back == mm[-back.size:]).all()
    ctx.free(d)
    n = mm.size
    return {"what": "mapped_file_h2d", "bytes": int(n), "plain_s": spread(plain), "staged_s": spread(staged),
            "plain_GBps": round(n / statistics.median(plain) / 1e9, 1), "staged_GBps": round(n / statistics.median(staged) / 1e9, 1)}


def end_to_end(path, k, threads, tmp):
    walls = {"host": [], "device": [], "device_plain_copy": []}
    last = {}
    h2d = {"device": [], "device_plain_copy": []}
    for _ in range(5):
        for name, extra in (("host", ["--parse-threads", str(threads)]), ("device", ["--device-parse", "--text-copy", "staged"]),
                            ("device_plain_copy", ["--device-parse", "--text-copy", "plain"])):
            r = bench_e2e.run_cfrk([path, os.path.join(tmp, "out.bin"), str(k), "--global", "--canonical", "--binary"] + extra)
            assert "error" not in r, r
            walls[name].append(r["process_wall_s"])
            last[name] = r
            if name in h2d:
                h2d[name].append(r["text_h2d_s"])
    return {"what": "end_to_end", "k": k, "host_parse_wall_s": spread(walls["host"]), "device_parse_wall_s": spread(walls["device"]),
            "device_parse_plain_copy_wall_s": spread(walls["device_plain_copy"]),
            "host_parse_s": last["host"]["parse_s"], "text_map_s": last["device"].get("text_map_s"),
            "text_h2d_staged_s": spread(h2d["device"]), "text_h2d_plain_s": spread(h2d["device_plain_copy"]),
            "device_parse_ms": last["device"].get("device_parse_ms"), "entries_equal": last["host"]["entries"] == last["device"]["entries"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--scale-reads", type=int, default=0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    ctx = cfrk_amd.Context(0)
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR")) as tmp:
        path = os.path.join(tmp, "image.fasta")
        if a.reads:
            bench_e2e.write_fasta(path, a.reads, 150, a.reads, ctx=ctx)
            text = np.fromfile(path, np.uint8)
            print(json.dumps(in_process(ctx, text, a.threads)), flush=True)
            del text
            print(json.dumps(mapped_file_h2d(ctx, path)), flush=True)
            if not a.skip_e2e:
                for k in (15, 31):
                    print(json.dumps(end_to_end(path, k, a.threads, tmp)), flush=True)
        if a.scale_reads:
            with open(path, "wb"):
                pass
            step = 8_000_000
            parts = []
            for r0 in range(0, a.scale_reads, step):
                p = os.path.join(tmp, "part.fasta")
                bench_e2e.write_fasta(p, min(step, a.scale_reads - r0), 150, 10_000_000, ctx=ctx, r0=r0)
                parts.append(np.fromfile(p, np.uint8))
            text = np.concatenate(parts)
            del parts
            assert text.size > 1 << 32 or a.scale_reads < 26_000_000
            r = in_process(ctx, text, a.threads, k=31)
            r["what"] = "at_scale"
            print(json.dumps(r), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
