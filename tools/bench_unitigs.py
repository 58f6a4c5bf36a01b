"""Cost of cfrk_global_unitigs_device on one counted result, k = 31 canonical by default, for the splitter periods asked for:

  a  --reads error-free synthetic reads of a --glen-base genome: few, huge unitigs
  b  the same reads with --error-rate substitutions, min_count 1: many nodes, many short unitigs
  c  b at min_count 2

The reads are synthesised on the device (cfrk_synth_reads_device, as bench.py does; the substitutions by torch on the
same buffer) and counted once per case.  Every call is timed with device events on the context's stream, median of
--reps after one warm-up, the splitter periods alternating inside a repetition.  Per (case, s) one JSON line:

  graph_ms   the sizes-only call: stages 1 .. 5 and the synchronisation
  call_ms    the whole call into arrays of exactly the sizes: stages 1 .. 7
  ns_per_node = call_ms / nodes; nodes, unitigs, bytes, the longest unitig and the circular ones from the records

and per case two yardsticks in the same process: cfrk_global_query_device on 8 x nodes uniformly random keys (capped at
--max-query-keys; the lookup floor of stage 1: the same 8 probes per node, most of them ending on an empty slot as the
absent neighbours' do) and a device copy of the output bytes.  Per-kernel times come from running this under
`rocprofv3 --kernel-trace --stats`, in a run of its own.

With --links the same cases time cfrk_global_unitig_links_device instead, on the unitigs the default splitter period
wrote: per case one JSON line (tool "bench_unitig_links") with the sizes-only call (tag, count, scan: `measure`), the
whole call into an array of exactly n_links rows (`call`), the unitigs call alternating with it in the same repetitions
(`unitigs_call`), and cfrk_global_query_device on 6 x o x unitigs uniformly random keys (o = 2: the canonical job's
orientations), the number of probes the passes make: 2 x unitigs in the tag pass, o x 4 x unitigs in the count pass.

  python tools/bench_unitigs.py [--links] [--cases a,b,c] [--split 8,10,12] [--reads R] [--L L] [--glen G] [--k K] [--reps N]
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
    ap.add_argument("--split", default="8,10,12")
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--L", type=int, default=100)
    ap.add_argument("--glen", type=int, default=10_000_000)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--error-rate", type=float, default=0.01)
    ap.add_argument("--max-query-keys", type=int, default=400_000_000)
    ap.add_argument("--links", action="store_true")
    a = ap.parse_args()

    import torch
    import cfrk_amd
    stream = torch.cuda.Stream()
    ctx = cfrk_amd.Context(0, stream.cuda_stream)
    R, L, k = a.reads, a.L, a.k
    nN = R * (L + 1)
    splits = [int(s) for s in a.split.split(",")]

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

    for case in a.cases.split(","):
        with torch.cuda.stream(stream):
            reads = buf(nN)
            ctx.synth_reads_device(0, R, L, a.glen, reads.data_ptr())
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

        def sizes():
            try:
                return g.unitigs_device(min_count, 0, 0, 0, 0, 0, 0)
            except cfrk_amd.CfrkError as e:
                if e.code != cfrk_amd.CFRK_ERR_SMALL_BUF:
                    raise
                return e.nN, e.nS

        oN, oS = sizes()                                        # (builds the lookup index: not part of any timing)
        out = [buf(oN), buf(oS * 8), buf(oS * 4), buf(oS * 16)]

        def full():
            g.unitigs_device(min_count, out[0].data_ptr(), oN, out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), oS)

        if a.links:
            full()
            ctx.sync()
            d_ptr = buf((oS + 1) * 8)
            unitigs = (out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), oN, oS)

            def link_sizes():
                try:
                    return g.unitig_links_device(min_count, *unitigs, d_ptr.data_ptr(), 0, 0)
                except cfrk_amd.CfrkError as e:
                    if e.code != cfrk_amd.CFRK_ERR_SMALL_BUF:
                        raise
                    return e.n_links

            n_links = link_sizes()
            d_links = buf(n_links * 8)
            copy_of = [buf(oN), buf(oS * 8), buf(oS * 4), buf(oS * 16)]     # (the unitigs call beside it writes elsewhere)

            def link_full():
                g.unitig_links_device(min_count, *unitigs, d_ptr.data_ptr(), d_links.data_ptr(), n_links)

            def unitigs_again():
                g.unitigs_device(min_count, copy_of[0].data_ptr(), oN, copy_of[1].data_ptr(), copy_of[2].data_ptr(), copy_of[3].data_ptr(), oS)

            nq = max(1, min(12 * oS, a.max_query_keys))
            with torch.cuda.stream(stream):
                keys = torch.randint(0, 1 << (2 * k), (nq,), device="cuda", dtype=torch.int64)
                ans = buf(nq * 4)
            torch.cuda.synchronize()

            def query():
                g.query_device(keys.data_ptr(), 0, nq, ans.data_ptr())

            t = {"measure": [], "call": [], "unitigs_call": [], "query_device": []}
            for rep in range(a.reps + 1):
                for name, fn in (("measure", link_sizes), ("call", link_full), ("unitigs_call", unitigs_again), ("query_device", query)):
                    ms = timed(fn)
                    if rep:                                     # (the first round warms up: code objects, pool buffers)
                        t[name].append(ms)
            torch.cuda.synchronize()
            row = {"tool": "bench_unitig_links", "case": case, "reads": R, "L": L, "glen": a.glen, "k": k, "reps": a.reps,
                   "error_rate": 0.0 if case == "a" else a.error_rate, "min_count": min_count, "distinct_keys": distinct,
                   "unitigs": oS, "bytes": oN, "links": n_links, "query_keys": nq}
            row.update({name: stats(ts) for name, ts in t.items()})
            row["call_over_unitigs"] = row["call"]["ms"] / row["unitigs_call"]["ms"]
            row["ns_per_unitig"] = row["call"]["ms"] * 1e6 / max(oS, 1)
            print(json.dumps(row), flush=True)
            del g, out, copy_of, keys, ans, d_ptr, d_links, reads
            torch.cuda.empty_cache()
            continue
        t_graph, t_call = {s: [] for s in splits}, {s: [] for s in splits}
        for rep in range(a.reps + 1):
            for s in splits:
                g.set_debug_param(cfrk_amd.CFRK_PARAM_UNITIG_SPLIT_LOG2, s + 1)
                tg, tc = timed(sizes), timed(full)
                if rep:                                         # (the first round warms up: code objects, pool buffers)
                    t_graph[s].append(tg)
                    t_call[s].append(tc)
        g.set_debug_param(cfrk_amd.CFRK_PARAM_UNITIG_SPLIT_LOG2, 0)
        torch.cuda.synchronize()
        rec = out[3][:oS * 16].view(torch.int32).view(oS, 4)
        n_kmers = rec[:, 2].to(torch.int64)
        nodes = int(n_kmers.sum())
        common = {"tool": "bench_unitigs", "case": case, "reads": R, "L": L, "glen": a.glen, "k": k, "reps": a.reps,
                  "error_rate": 0.0 if case == "a" else a.error_rate, "min_count": min_count, "distinct_keys": distinct,
                  "nodes": nodes, "unitigs": oS, "bytes": oN, "longest_kmers": int(n_kmers.max()) if oS else 0,
                  "circular": int((rec[:, 3] & 1).sum()) if oS else 0}
        # yardsticks
        nq = min(8 * nodes, a.max_query_keys)
        with torch.cuda.stream(stream):
            keys = torch.randint(0, 1 << (2 * k), (nq,), device="cuda", dtype=torch.int64)
            ans = buf(nq * 4)
            dst = buf(oN)
        torch.cuda.synchronize()

        def query():
            g.query_device(keys.data_ptr(), 0, nq, ans.data_ptr())

        def copy():
            with torch.cuda.stream(stream):
                dst[:oN].copy_(out[0][:oN])

        yard = {}
        for name, fn in (("query_device", query), ("copy_output", copy)):
            fn()
            ctx.sync()
            yard[name] = stats([timed(fn) for _ in range(a.reps)])
        for s in splits:
            call = stats(t_call[s])
            print(json.dumps(dict(common, split_log2=s, graph=stats(t_graph[s]), call=call,
                                  ns_per_node=call["ms"] * 1e6 / max(nodes, 1), query_keys=nq,
                                  query_device=yard["query_device"], copy_output=yard["copy_output"])), flush=True)
        del g, out, keys, ans, dst, reads
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
