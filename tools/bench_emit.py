"""Cost of text out: cfrk_text_index_device against cfrk_fastq_parse_device on the same text, and
cfrk_reads_emit_text_device -- all reads as FASTQ and as FASTA, and the reads a real filter keeps -- against two yardsticks
measured in the same run: a plain device-to-device copy of the output's byte count, and cfrk_reads_select_device on the
same reads.  Expectation: emit costs per output byte no more than twice what the select costs per output byte.

The FASTQ image of --reads synthetic reads of --L bases (names of nine digits, Phred+33 qualities) is built on the
device; the reads come from a genome of --reads bases and are counted once at --k, canonical, so that the spans of
the "real filter" (longest run of windows counted at least twice, min_len k) trim and drop.  The context runs on a torch
stream so that every call is timed with device events on its own stream; after a warm-up the calls alternate; median, min
and max of --reps.  The emit and select calls synchronise once inside (the sizes): that wait is part of their time.
Report only: cfrk_host_format_fasta on the selected reads (--host-format), and with --cli the process wall of `cfrk
--filter-out` with and without --filter-format fastq on a file of --cli-reads reads (alternating runs).
Appends one JSON line to --out and prints it.

  python tools/bench_emit.py [--reads R] [--L L] [--k K] [--reps N] [--out FILE] [--host-format] [--cli] [--cli-reads C]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fastq_image(torch, codes, Q, L):
    """codes: Q x L uint8 in 0..3 on the device -> the text as a Q x (2 L + 16) uint8 tensor"""
    W = 2 * L + 16
    text = torch.empty((Q, W), dtype=torch.uint8, device="cuda")
    idx = torch.arange(Q, device="cuda", dtype=torch.int64)
    text[:, 0] = ord("@")
    text[:, 1] = ord("r")
    for j in range(9):
        text[:, 2 + j] = ((idx // 10 ** (8 - j)) % 10 + 48).to(torch.uint8)
    text[:, 11] = 10
    seq = text[:, 12:12 + L]
    seq.fill_(ord("A"))
    for c, ch in ((1, "C"), (2, "G"), (3, "T")):
        seq.masked_fill_(codes == c, ord(ch))
    text[:, 12 + L] = 10
    text[:, 13 + L] = ord("+")
    text[:, 14 + L] = 10
    text[:, 15 + L:15 + 2 * L] = torch.randint(35, 74, (Q, L), dtype=torch.uint8, device="cuda")
    text[:, 15 + 2 * L] = 10
    return text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--L", type=int, default=150)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "bench_emit.jsonl"))
    ap.add_argument("--host-format", action="store_true")
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--cli-reads", type=int, default=2_000_000)
    a = ap.parse_args()

    import numpy as np
    import torch
    import cfrk_amd
    stream = torch.cuda.Stream()
    ctx = cfrk_amd.Context(0, stream.cuda_stream)
    FA, FQ = cfrk_amd.CFRK_TEXT_FASTA, cfrk_amd.CFRK_TEXT_FASTQ

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

    def buf(nbytes):
        return torch.empty(nbytes + 64, dtype=torch.uint8, device="cuda")

    def reads_text(Q, L):
        """-> the FASTQ image of Q synthetic reads on the device (a flat uint8 tensor)"""
        with torch.cuda.stream(stream):
            raw, st, ln = buf(Q * (L + 1)), buf(Q * 8), buf(Q * 4)
            ctx.synth_reads_device(0, Q, L, Q, raw.data_ptr(), st.data_ptr(), ln.data_ptr())
            ctx.sync()
            codes = raw[:Q * (L + 1)].view(Q, L + 1)[:, :L] & 3
            text = fastq_image(torch, codes, Q, L).view(-1)
        torch.cuda.synchronize()
        return text

    Q, L, k = a.reads, a.L, a.k
    res = {"tool": "bench_emit", "reads": Q, "L": L, "k": k, "reps": a.reps}
    if a.cli:
        # process wall of the CLI's filter with and without the device text path, on one file as input and as QFILE
        Qc = min(a.cli_reads, Q)
        text = reads_text(Qc, L).cpu().numpy()
        cli = os.path.join(ROOT, "cfrk_amd", "cfrk")
        with tempfile.TemporaryDirectory() as tmp:
            fq = os.path.join(tmp, "reads.fastq")
            text.tofile(fq)
            base = [cli, fq, os.path.join(tmp, "none.cfrk"), str(k), "--global", "--canonical", "--query", fq, "--query-only", "--filter-out"]
            runs = {"filter_out_numbered_fasta": base + [os.path.join(tmp, "a.fa")],
                    "filter_out_format_fastq": base + [os.path.join(tmp, "b.fq"), "--filter-format", "fastq"]}
            walls = {n: [] for n in runs}
            for rep in range(a.reps + 1):                    # (the first round warms the page cache)
                for n, cmd in runs.items():
                    t0 = time.perf_counter()
                    subprocess.run(cmd, check=True, timeout=1200)
                    if rep:
                        walls[n].append(time.perf_counter() - t0)
            res.update({"case": "cli_wall", "cli_reads": Qc, "text_bytes": int(text.size),
                        "out_bytes": {n: os.path.getsize(cmd[10]) for n, cmd in runs.items()},
                        **{n + "_s": {"median": statistics.median(w), "min": min(w), "max": max(w)} for n, w in walls.items()}})
    else:
        text = reads_text(Q, L)
        nb = int(text.numel())
        assert text.data_ptr() % 16 == 0
        d_data, d_start, d_length = buf(nb // 2), buf(Q * 8), buf(Q * 4)
        d_rec, d_span = buf(Q * 24), buf(Q * 8)
        parse = lambda: ctx.parse_fastq_device(text.data_ptr(), nb, 0, d_data.data_ptr(), nb // 2, d_start.data_ptr(), d_length.data_ptr(), Q)
        index = lambda: ctx.index_text_device(text.data_ptr(), nb, FQ, d_rec.data_ptr(), Q)
        nN, nS = parse()
        assert (nN, nS) == (Q * (L + 1), Q) and index() == Q
        ctx.sync()
        rec = np.empty(3, cfrk_amd.TEXT_RECORD_DTYPE)
        ctx.d2h(rec, d_rec.data_ptr() + (Q - 3) * 24)
        W = 2 * L + 16
        assert rec["head_off"].tolist() == [(Q - 3 + j) * W for j in range(3)] and rec["qual_off"].tolist() == [(Q - 3 + j) * W + 15 + L for j in range(3)]
        assert rec["head_len"].tolist() == [11] * 3 and rec["qual_len"].tolist() == [L] * 3
        res.update({"case": "index_and_emit", "text_bytes": nb, "index_vs_parse": alternate({"fastq_parse": parse, "text_index": index})})
        g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, min(2 * Q, 4 ** min(k, 31)) + 1024)
        g.add_device(d_data.data_ptr(), nN)
        ctx.sync()
        res["distinct"] = g.digest()[0]
        g.read_spans_device(d_data.data_ptr(), d_start.data_ptr(), d_length.data_ptr(), nN, nS, 2, cfrk_amd.CFRK_COUNT_MAX,
                            cfrk_amd.CFRK_SPAN_LONGEST, d_span.data_ptr())
        ctx.sync()
        d_out = buf(nb)
        od, os_, ol, oi = buf(nN), buf(Q * 8), buf(Q * 4), buf(Q * 8)
        ptr = lambda t: t.data_ptr() if t is not None else 0
        for name, sp, min_len, fmt in (("all_fastq", None, 0, FQ), ("all_fasta", None, 0, FA), ("filtered_fastq", d_span, k, FQ)):
            emit = lambda: ctx.emit_reads_device(d_data.data_ptr(), d_start.data_ptr(), d_length.data_ptr(), nN, nS, ptr(sp), 0, min_len,
                                                 text.data_ptr(), nb, d_rec.data_ptr(), fmt, d_out.data_ptr(), nb)
            sel = lambda: ctx.select_reads_device(d_data.data_ptr(), d_start.data_ptr(), d_length.data_ptr(), nN, nS, ptr(sp), 0, min_len,
                                                  od.data_ptr(), nN, os_.data_ptr(), ol.data_ptr(), oi.data_ptr(), nS)
            ob, on = emit()
            n2, s2 = sel()
            assert on == s2
            ctx.sync()
            if name == "all_fastq":                          # whole reads, names and qualities as they came: the text itself
                with torch.cuda.stream(stream):
                    same = bool(torch.equal(d_out[:ob], text))
                res["all_fastq_is_the_input_text"] = same
            t = alternate({"emit": emit, "select": sel, "d2d": d2d(ob)})
            r = {"out_bytes": ob, "reads_out": on, "select_bytes": n2, **{n + "_" + f: v for n, tt in t.items() for f, v in tt.items()}}
            r["emit_ratio_to_d2d"] = t["emit"]["ms"] / t["d2d"]["ms"]
            r["emit_ns_per_out_byte"] = t["emit"]["ms"] * 1e6 / ob
            r["select_ns_per_out_byte"] = t["select"]["ms"] * 1e6 / n2
            r["emit_per_byte_over_select_per_byte"] = r["emit_ns_per_out_byte"] / r["select_ns_per_out_byte"]
            r["within_twice_the_select"] = r["emit_per_byte_over_select_per_byte"] <= 2.0
            res[name] = r
        if a.host_format:
            # the step the device path replaces: the selected reads come down and one host thread formats them
            n2, s2 = ctx.select_reads_device(d_data.data_ptr(), d_start.data_ptr(), d_length.data_ptr(), nN, nS, d_span.data_ptr(), 0, k,
                                             od.data_ptr(), nN, os_.data_ptr(), ol.data_ptr(), oi.data_ptr(), nS)
            t0 = time.perf_counter()
            h_d, h_s, h_l, h_i = np.empty(n2, np.int8), np.empty(s2, np.int64), np.empty(s2, np.int32), np.empty(s2, np.int64)
            for h, d in ((h_d, od), (h_s, os_), (h_l, ol), (h_i, oi)):
                ctx.d2h(h, d.data_ptr())
            t1 = time.perf_counter()
            H = C.CDLL(os.path.join(ROOT, "cfrk_amd", "libcfrk_host.so"))
            H.cfrk_host_format_fasta.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t]
            H.cfrk_host_format_fasta.restype = C.c_size_t
            vp = lambda x: x.ctypes.data_as(C.c_void_p)
            size = H.cfrk_host_format_fasta(vp(h_d), vp(h_s), vp(h_l), vp(h_i), s2, None, 0)
            out = np.empty(size, np.uint8)
            H.cfrk_host_format_fasta(vp(h_d), vp(h_s), vp(h_l), vp(h_i), s2, vp(out), size)
            res["host_format_fasta"] = {"reads": s2, "out_bytes": int(size), "copies_back_s": t1 - t0, "format_s": time.perf_counter() - t1}
    ctx.close()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
