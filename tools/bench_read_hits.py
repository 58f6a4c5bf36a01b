"""Cost of the position map and of the read hits on one counted result, k = 31 canonical by default:

  a  --reads error-free synthetic reads of a --glen-base genome: few, huge unitigs
  b  the same reads with --error-rate substitutions, min_count 1: many nodes, many short unitigs
  c  b at min_count 2

The reads are synthesised on the device (cfrk_synth_reads_device, as bench.py does; the substitutions by torch on the
same buffer) and counted once per case; the unitigs are written once by cfrk_global_unitigs_device.  Every call is timed
with device events on the context's stream, median of --reps after one warm-up, the calls alternating inside a
repetition.  Per case one JSON line, appended to --out as well:

  index          cfrk_global_unitig_index_device on the unitig list; ns_per_node = its ms / nodes
  links          cfrk_global_unitig_links_device (the whole call) on the same list
  query_device   cfrk_global_query_device on as many uniformly random keys as there are nodes
  copy_unitigs   a device copy of the unitig bytes
  hits_sizes     cfrk_global_read_hits_device, sizes only: the count pass, the scan, the synchronisation
  hits           the whole call into an array of exactly n_hits rows: count, scan, fill, finish
  spans          cfrk_global_read_spans_device (longest run, min_count as the case's) on the same reads
  hits_over_spans = hits / spans

With --paths the same three cases measure cfrk_global_read_paths_device on the hits and the links of the case (appended
to profiles/r32/bench_read_paths.jsonl):

  hits           the yardstick: the cfrk_global_read_hits_device call that produces the hits
  paths_sizes    cfrk_global_read_paths_device, sizes only, no support: checks, join, scan, path_ptr, the synchronisation
  paths          the whole call into an array of exactly n_paths rows, with support
  paths_plain    the same without support: what the atomics on support[] cost is paths - paths_plain
  copy_hits      the byte floor: a device copy of the hit array's bytes (16 B per hit in; 16 B per path and path_ptr out
                 are less)
  and paths_per_read, n_steps, n_gaps, n_unlinked, one_path_share (reads that are exactly one path) and max_support

Per-kernel times come from running this under `rocprofv3 --kernel-trace --stats`, in a run of its own.

  python tools/bench_read_hits.py [--paths] [--cases a,b,c] [--reads R] [--L L] [--glen G] [--k K] [--reps N] [--out FILE]
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
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--L", type=int, default=100)
    ap.add_argument("--glen", type=int, default=10_000_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--error-rate", type=float, default=0.01)
    ap.add_argument("--paths", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "r32", "bench_read_paths.jsonl") if a.paths else os.path.join(ROOT, "profiles", "r27", "bench_read_hits.jsonl")

    import torch
    import cfrk_amd
    stream = torch.cuda.Stream()
    ctx = cfrk_amd.Context(0, stream.cuda_stream)
    R, L, k = a.reads, a.L, a.k
    nN = R * (L + 1)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def stats(ts):
        return {"ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}

    def buf(nbytes):
        return torch.empty(nbytes + 64, dtype=torch.uint8, device="cuda")

    def small_buf(call, field):
        try:
            return call()
        except cfrk_amd.CfrkError as e:
            if e.code != cfrk_amd.CFRK_ERR_SMALL_BUF:
                raise
            return getattr(e, field) if isinstance(field, str) else tuple(getattr(e, f) for f in field)

    for case in a.cases.split(","):
        with torch.cuda.stream(stream):
            reads, r_start, r_length = buf(nN), buf(R * 8), buf(R * 4)
            ctx.synth_reads_device(0, R, L, a.glen, reads.data_ptr(), r_start.data_ptr(), r_length.data_ptr())
            ctx.sync()
            if case != "a":                                     # substitutions: another base, never a terminator
                gen = torch.Generator(device="cuda").manual_seed(25)
                codes = reads[:nN].view(R, L + 1)[:, :L]
                hit = torch.rand((R, L), device="cuda", generator=gen) < a.error_rate
                shift = torch.randint(1, 4, (R, L), device="cuda", generator=gen, dtype=torch.uint8)
                codes.copy_(torch.where(hit, (codes + shift) & 3, codes))
                del hit, shift
        torch.cuda.synchronize()
        min_count = 2 if case == "c" else 1
        hint = min(2 * a.glen + int(R * L * a.error_rate * k * (case != "a")), R * (L - k + 1)) + 1024
        g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, hint)
        g.add_device(reads.data_ptr(), nN)
        ctx.sync()
        distinct = g.digest()[0]
        oN, oS = small_buf(lambda: g.unitigs_device(min_count, 0, 0, 0, 0, 0, 0), ("nN", "nS"))
        u = [buf(oN), buf(oS * 8), buf(oS * 4), buf(oS * 16)]
        g.unitigs_device(min_count, u[0].data_ptr(), oN, u[1].data_ptr(), u[2].data_ptr(), u[3].data_ptr(), oS)
        ctx.sync()
        unitigs = (u[0].data_ptr(), u[1].data_ptr(), u[2].data_ptr(), oN, oS)
        n_kmers = u[3][:oS * 16].view(torch.int32).view(oS, 4)[:, 2].to(torch.int64)
        nodes = int(n_kmers.sum())
        rd = (reads.data_ptr(), r_start.data_ptr(), r_length.data_ptr(), nN, R)

        d_lptr = buf((oS + 1) * 8)
        n_links = small_buf(lambda: g.unitig_links_device(min_count, *unitigs, d_lptr.data_ptr(), 0, 0), "n_links")
        d_links = buf(n_links * 8)
        g.unitig_index_device(min_count, *unitigs)
        d_hptr = buf((R + 1) * 8)
        n_hits = small_buf(lambda: g.read_hits_device(*rd, d_hptr.data_ptr(), 0, 0), "n_hits")
        d_hits = buf(n_hits * 16)
        if a.paths:
            g.unitig_links_device(min_count, *unitigs, d_lptr.data_ptr(), d_links.data_ptr(), n_links)
            g.read_hits_device(*rd, d_hptr.data_ptr(), d_hits.data_ptr(), n_hits)
            ctx.sync()
            graph = (d_hptr.data_ptr(), R, d_hits.data_ptr(), n_hits, u[3].data_ptr(), oS, d_lptr.data_ptr(), d_links.data_ptr(), n_links)
            d_pptr = buf((R + 1) * 8)
            n_paths, pstats = small_buf(lambda: g.read_paths_device(*graph, d_pptr.data_ptr(), 0, 0), ("n_paths", "stats"))
            d_paths, dst = buf(n_paths * 16), buf(n_hits * 16)
            with torch.cuda.stream(stream):
                support = torch.zeros(max(n_links, 1), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()

            def copy_hits():
                with torch.cuda.stream(stream):
                    dst[:n_hits * 16].copy_(d_hits[:n_hits * 16])

            # one call into the zeroed support: what a caller gets (the timed calls below add to it again)
            g.read_paths_device(*graph, d_pptr.data_ptr(), d_paths.data_ptr(), n_paths, support.data_ptr())
            ctx.sync()
            max_support = int(support.max()) if n_links else 0
            rows = d_pptr[:(R + 1) * 8].view(torch.int64)
            one_path = int(((rows[1:] - rows[:-1]) == 1).sum())
            calls = (("hits", lambda: g.read_hits_device(*rd, d_hptr.data_ptr(), d_hits.data_ptr(), n_hits)),
                     ("paths_sizes", lambda: small_buf(lambda: g.read_paths_device(*graph, d_pptr.data_ptr(), 0, 0), "n_paths")),
                     ("paths", lambda: g.read_paths_device(*graph, d_pptr.data_ptr(), d_paths.data_ptr(), n_paths, support.data_ptr())),
                     ("paths_plain", lambda: g.read_paths_device(*graph, d_pptr.data_ptr(), d_paths.data_ptr(), n_paths)),
                     ("copy_hits", copy_hits))
            t = {name: [] for name, _ in calls}
            for rep in range(a.reps + 1):
                for name, fn in calls:
                    ms = timed(fn)
                    if rep:
                        t[name].append(ms)
            torch.cuda.synchronize()
            row = {"tool": "bench_read_hits --paths", "case": case, "reads": R, "L": L, "glen": a.glen, "k": k, "reps": a.reps,
                   "error_rate": 0.0 if case == "a" else a.error_rate, "min_count": min_count, "unitigs": oS, "n_links": n_links,
                   "n_hits": n_hits, "n_paths": n_paths, "paths_per_read": n_paths / R, "n_steps": pstats["n_steps"],
                   "n_gaps": pstats["n_gaps"], "n_unlinked": pstats["n_unlinked"], "one_path_share": one_path / R,
                   "max_support": max_support, "steps_per_link": pstats["n_steps"] / max(n_links, 1)}
            row.update({name: stats(ts) for name, ts in t.items()})
            row["paths_over_hits"] = row["paths"]["ms"] / row["hits"]["ms"]
            row["paths_over_copy"] = row["paths"]["ms"] / row["copy_hits"]["ms"]
            line = json.dumps(row)
            print(line, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
            del g, u, reads, r_start, r_length, d_lptr, d_links, d_hptr, d_hits, d_pptr, d_paths, dst, support, rows
            torch.cuda.empty_cache()
            continue
        d_spans = buf(R * 8)
        with torch.cuda.stream(stream):
            keys = torch.randint(0, 1 << (2 * k), (max(nodes, 1),), device="cuda", dtype=torch.int64)
            ans = buf(max(nodes, 1) * 4)
            dst = buf(oN)
        torch.cuda.synchronize()

        def copy():
            with torch.cuda.stream(stream):
                dst[:oN].copy_(u[0][:oN])

        calls = (("index", lambda: g.unitig_index_device(min_count, *unitigs)),
                 ("links", lambda: g.unitig_links_device(min_count, *unitigs, d_lptr.data_ptr(), d_links.data_ptr(), n_links)),
                 ("query_device", lambda: g.query_device(keys.data_ptr(), 0, len(keys), ans.data_ptr())),
                 ("copy_unitigs", copy),
                 ("hits_sizes", lambda: small_buf(lambda: g.read_hits_device(*rd, d_hptr.data_ptr(), 0, 0), "n_hits")),
                 ("hits", lambda: g.read_hits_device(*rd, d_hptr.data_ptr(), d_hits.data_ptr(), n_hits)),
                 ("spans", lambda: g.read_spans_device(*rd, min_count, 0xFFFFFFFE, cfrk_amd.CFRK_SPAN_LONGEST, d_spans.data_ptr())))
        t = {name: [] for name, _ in calls}
        for rep in range(a.reps + 1):
            for name, fn in calls:
                ms = timed(fn)
                if rep:                                         # (the first round warms up: code objects, pool buffers)
                    t[name].append(ms)
        torch.cuda.synchronize()
        row = {"tool": "bench_read_hits", "case": case, "reads": R, "L": L, "glen": a.glen, "k": k, "reps": a.reps,
               "error_rate": 0.0 if case == "a" else a.error_rate, "min_count": min_count, "distinct_keys": distinct,
               "nodes": nodes, "unitigs": oS, "unitig_bytes": oN, "longest_kmers": int(n_kmers.max()) if oS else 0,
               "n_links": n_links, "n_hits": n_hits, "windows": R * (L - k + 1)}
        row.update({name: stats(ts) for name, ts in t.items()})
        row["index_ns_per_node"] = row["index"]["ms"] * 1e6 / max(nodes, 1)
        row["index_over_links"] = row["index"]["ms"] / row["links"]["ms"]
        row["index_over_query"] = row["index"]["ms"] / row["query_device"]["ms"]
        row["hits_over_spans"] = row["hits"]["ms"] / row["spans"]["ms"]
        line = json.dumps(row)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        del g, u, keys, ans, dst, reads, r_start, r_length, d_lptr, d_links, d_hptr, d_hits, d_spans
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
