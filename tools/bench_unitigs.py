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

With --tips (cases b and c are the ones of interest) the tool "bench_tips" writes, per case: a line "unmasked" with the
unitigs, links and index calls without a mask, alternating in the same repetitions with the same calls of the library
given by --parent-lib on the same counted reads, and the verdict whether each median lies inside the parent's own
run-to-run spread; a line "round1" with the tips call, the mask_unitigs call, and the unitigs, links and index calls with
the mask of round 1 set, all alternating; and a line "rounds" with nodes, unitigs, tips and masked keys per clip round.

With --bubbles (cases b and c) the tool "bench_bubbles" writes, per case: a line "tips_ab" with the tips call on the
unmasked graph, alternating in the same repetitions with the tips call of the library given by --parent-lib (the check
and in-rows passes moved to a header the bubble rule shares: the call must be what it was) and the verdict whether its
median lies inside the parent's own spread; a line "bubbles" with the bubbles call (--bubble-max-diff, --bubble-ratio,
max_kmers = k) and the tips call alternating, and what both found; and a line "rounds" with nodes, unitigs, tips,
bubbles and masked keys per round of the combined loop, one mask call per round.

With --bulges (cases b and c) the tool "bench_bulges" writes, per case: a line "bulges" with the bulges call
(--bulge-max-diff, --bulge-max-visits, --bulge-ratio, max_kmers = k, max_hops = min(k + max_diff, 64); paths wanted,
sizes-only call and fill pass included) alternating with the bubbles call in the same repetitions, arms, popped and
undecided, ns per arm, and the distributions of visits (over arms) and hops (over popped arms); and a line "rounds" with
nodes, unitigs, tips, bubbles, bulges and masked keys per round of the combined loop, one mask call per round.

With --compact (cases b and c) the tool "bench_compact" writes, per case: a line "compact" with the compaction call
(cfrk_global_unitigs_compact_device on the unmasked graph and the drop bytes of round 1 of tips + bubbles + bulges, into
arrays of exactly the sizes) alternating in the same repetitions with the unitigs call under the mask of those drop bytes
-- the yardstick: the two results are asserted byte-equal first --, with the compaction's sizes-only call (everything up
to its synchronisation; the difference to the whole call is the sort, the scans, the members' list and the emit) and with
a device copy of the output bytes; and a line "loop" with the whole loop of --tip-rounds rounds, every round's graph made
by the unitigs call or by the compaction, the two alternating over --loop-reps repetitions, the rounds asserted equal.

With --weak (cases b and c) the tool "bench_weak" writes, per case: a line "weak" with the weak call (--weak-ratio,
--weak-iso-mean, max_kmers = k, iso_max_kmers = 2k) alternating in the same repetitions with the tips call, the bubbles
call and the links call that feeds all three, the candidates, connections and isolated unitigs found, and how many of the
connections the bubble rule pops as well; and two lines "rounds", for the combined loop without the rule (tips + bubbles +
bulges) and with it, each with nodes, unitigs and what every rule found per round and after the loop, and, on the graph
the loop leaves, the hits and paths (read_hits, read_paths) of the reads that were counted and of the same reads without
their substitutions: reads, reads in one path, reads in several, reads without a hit, gaps and unlinked steps.  A read
with an error breaks where the error's k-mers were dropped, as it should; an error-free read that breaks is true sequence
eaten -- the check on the rule's default ratio.  A third "rounds" line with
no rule at all gives the same numbers on the graph as counted.

With --components the tool "bench_components" writes, per case: a line "components" with the components call
(cfrk_global_unitig_components_device, the table at exact capacity) alternating in the same repetitions with its
sizes-only call, the weak call and the links call, and the census of the graph: components, the largest one's k-mers,
unitigs and share of all k-mers, the components below 2k k-mers and their k-mers, the components of one unitig; a line
"crafted_pair" with the call on two crafted link sets of the same nS and n_links over the same records -- (a) all one
component, (b) links only inside blocks of 8 unitigs -- which read the same bytes, and their ratio; and, case b, a line
"components_after_loop" with the census of the graph the four-rule loop leaves.

  python tools/bench_unitigs.py [--links | --tips [--parent-lib SO] | --bubbles [--parent-lib SO] | --bulges | --compact | --weak | --components] [--cases a,b,c] [--split 8,10,12] [--reads R] [--L L] [--glen G] [--k K] [--reps N]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Graph:
    """the unitigs, links and position map of a job through the device forms, into buffers of exactly the sizes"""

    def __init__(self, mod, g, min_count, buf):
        self.mod, self.g, self.mc, self.buf = mod, g, min_count, buf
        self.resize()

    def resize(self):
        g, mod = self.g, self.mod
        try:
            nN, nS = g.unitigs_device(self.mc, 0, 0, 0, 0, 0, 0)
        except mod.CfrkError as e:
            if e.code != mod.CFRK_ERR_SMALL_BUF:
                raise
            nN, nS = e.nN, e.nS
        self.nN, self.nS = nN, nS
        self.out = [self.buf(nN), self.buf(nS * 8), self.buf(nS * 4), self.buf(nS * 16)]
        self.unitigs()
        self.args = (self.out[0].data_ptr(), self.out[1].data_ptr(), self.out[2].data_ptr(), nN, nS)
        self.ptr = self.buf((nS + 1) * 8)
        try:
            self.n_links = g.unitig_links_device(self.mc, *self.args, self.ptr.data_ptr(), 0, 0)
        except mod.CfrkError as e:
            if e.code != mod.CFRK_ERR_SMALL_BUF:
                raise
            self.n_links = e.n_links
        self.rows = self.buf(self.n_links * 8)
        self.links()

    def unitigs(self):
        o = self.out
        self.g.unitigs_device(self.mc, o[0].data_ptr(), self.nN, o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), self.nS)

    def links(self):
        self.g.unitig_links_device(self.mc, *self.args, self.ptr.data_ptr(), self.rows.data_ptr(), self.n_links)

    def index(self):
        self.g.unitig_index_device(self.mc, *self.args)

    def nodes(self, torch):
        return int(self.out[3][:self.nS * 16].view(torch.int32).view(self.nS, 4)[:, 2].to(torch.int64).sum()) if self.nS else 0


def tips_case(a, torch, cfrk_amd, ctx, g, parent, other, min_count, common, timed, stats, buf):
    k = a.k
    ratio_q8 = int(round(a.tip_ratio * 256))
    new = _Graph(cfrk_amd, g, min_count, buf)
    ctx.sync()
    # 1 no mask set: this library and the parent's, alternating
    series = {"new": new}
    if other is not None:
        series["parent"] = _Graph(parent, other, min_count, buf)
        assert (series["parent"].nN, series["parent"].nS, series["parent"].n_links) == (new.nN, new.nS, new.n_links)
    t = {(who, call): [] for who in series for call in ("unitigs", "links", "index")}
    for rep in range(a.reps + 1):
        for call in ("unitigs", "links", "index"):
            for who in (("parent", "new") if rep % 2 else ("new", "parent")):
                if who in series:
                    ms = timed(getattr(series[who], call))
                    if rep:                                     # (the first round warms up: code objects, pool buffers)
                        t[(who, call)].append(ms)
    row = dict(common, line="unmasked", nodes=new.nodes(torch), unitigs=new.nS, links=new.n_links)
    for (who, call), ts in t.items():
        row["%s_%s" % (who, call)] = dict(stats(ts), series=ts)
    if other is not None:
        row["inside_parent_spread"] = {call: row["parent_" + call]["min_ms"] <= row["new_" + call]["ms"] <= row["parent_" + call]["max_ms"]
                                       for call in ("unitigs", "links", "index")}
        row["new_over_parent"] = {call: row["new_" + call]["ms"] / row["parent_" + call]["ms"] for call in ("unitigs", "links", "index")}
    print(json.dumps(row), flush=True)
    series.pop("parent", None)
    # 2 round 1: the tips call and the mask call, then the three calls with that mask set
    d_tip = buf(new.nS)
    tip_args = (new.out[3].data_ptr(), new.nS, new.ptr.data_ptr(), new.rows.data_ptr(), new.n_links, k, ratio_q8, d_tip.data_ptr())
    n_tips = g.unitig_tips_device(*tip_args)
    g.mask_unitigs_device(*new.args, d_tip.data_ptr())
    masked = _Graph(cfrk_amd, g, min_count, buf)
    ctx.sync()
    calls = (("tips", lambda: g.unitig_tips_device(*tip_args)), ("mask_unitigs", lambda: g.mask_unitigs_device(*new.args, d_tip.data_ptr())),
             ("unitigs_masked", masked.unitigs), ("links_masked", masked.links), ("index_masked", masked.index))
    t = {name: [] for name, _ in calls}
    for rep in range(a.reps + 1):
        for name, fn in calls:
            ms = timed(fn)
            if rep:
                t[name].append(ms)
    row = dict(common, line="round1", unitigs=new.nS, links=new.n_links, tips=n_tips, masked_keys=g.mask_count(),
               unitigs_after=masked.nS, links_after=masked.n_links, tip_ratio=a.tip_ratio, tip_max_kmers=k)
    row.update({name: stats(ts) for name, ts in t.items()})
    print(json.dumps(row), flush=True)
    # 3 the rounds
    g.mask_clear()
    rounds, cur = [], new
    for r in range(a.tip_rounds):
        if r:
            cur = _Graph(cfrk_amd, g, min_count, buf)
        d_tip = buf(cur.nS)
        n_tips = g.unitig_tips_device(cur.out[3].data_ptr(), cur.nS, cur.ptr.data_ptr(), cur.rows.data_ptr(), cur.n_links, k, ratio_q8, d_tip.data_ptr())
        if n_tips:
            g.mask_unitigs_device(*cur.args, d_tip.data_ptr())
        rounds.append({"round": r + 1, "nodes": cur.nodes(torch), "unitigs": cur.nS, "tips": n_tips, "masked_keys": g.mask_count()})
        if not n_tips:
            break
    if rounds[-1]["tips"]:
        last = _Graph(cfrk_amd, g, min_count, buf)
        rounds.append({"round": len(rounds) + 1, "nodes": last.nodes(torch), "unitigs": last.nS, "tips": None, "masked_keys": g.mask_count()})
    print(json.dumps(dict(common, line="rounds", tip_ratio=a.tip_ratio, tip_max_kmers=k, rounds=rounds)), flush=True)


def bubbles_case(a, torch, cfrk_amd, ctx, g, parent, other, min_count, common, timed, stats, buf):
    k = a.k
    tip_q8, bub_q8 = int(round(a.tip_ratio * 256)), int(round(a.bubble_ratio * 256))
    new = _Graph(cfrk_amd, g, min_count, buf)
    ctx.sync()
    d_tip, d_pop, d_partner = buf(new.nS), buf(new.nS), buf(new.nS * 4)

    def graph_args(gr):
        return (gr.out[3].data_ptr(), gr.nS, gr.ptr.data_ptr(), gr.rows.data_ptr(), gr.n_links)

    # 1 the tips call: this library and the parent's, alternating
    calls = {"new": lambda: g.unitig_tips_device(*graph_args(new), k, tip_q8, d_tip.data_ptr())}
    if other is not None:
        old = _Graph(parent, other, min_count, buf)
        assert (old.nN, old.nS, old.n_links) == (new.nN, new.nS, new.n_links)
        d_tip_old = buf(old.nS)
        calls["parent"] = lambda: other.unitig_tips_device(*graph_args(old), k, tip_q8, d_tip_old.data_ptr())
    t = {who: [] for who in calls}
    found = {}
    for rep in range(2 * a.reps + 1):
        for who in (("parent", "new") if rep % 2 else ("new", "parent")):
            if who in calls:
                box = []
                ms = timed(lambda: box.append(calls[who]()))
                found[who] = box[0]
                if rep:                                         # (the first round warms up: code objects, pool buffers)
                    t[who].append(ms)
    row = dict(common, line="tips_ab", nodes=new.nodes(torch), unitigs=new.nS, links=new.n_links, tips=found["new"], tip_ratio=a.tip_ratio)
    for who, ts in t.items():
        row[who + "_tips"] = dict(stats(ts), series=ts)
    if other is not None:
        assert found["parent"] == found["new"] and bool((d_tip[:new.nS] == d_tip_old[:new.nS]).all())
        row["inside_parent_spread"] = row["parent_tips"]["min_ms"] <= row["new_tips"]["ms"] <= row["parent_tips"]["max_ms"]
        row["new_over_parent"] = row["new_tips"]["ms"] / row["parent_tips"]["ms"]
    print(json.dumps(row), flush=True)
    # 2 the bubbles call beside the tips call
    bub = lambda: g.unitig_bubbles_device(*graph_args(new), k, a.bubble_max_diff, bub_q8, d_pop.data_ptr(), d_partner.data_ptr())
    n_pop = bub()
    t = {"bubbles": [], "tips": []}
    for rep in range(a.reps + 1):
        for name, fn in (("bubbles", bub), ("tips", calls["new"])):
            ms = timed(fn)
            if rep:
                t[name].append(ms)
    row = dict(common, line="bubbles", unitigs=new.nS, links=new.n_links, bubbles_found=n_pop, tips_found=found["new"], bubble_max_kmers=k,
               bubble_max_diff=a.bubble_max_diff, bubble_ratio=a.bubble_ratio)
    row.update({name: stats(ts) for name, ts in t.items()})
    row["ns_per_unitig"] = row["bubbles"]["ms"] * 1e6 / max(new.nS, 1)
    print(json.dumps(row), flush=True)
    # 3 the rounds of the combined loop
    rounds, cur = [], new
    for r in range(a.tip_rounds):
        if r:
            cur = _Graph(cfrk_amd, g, min_count, buf)
            d_tip, d_pop = buf(cur.nS), buf(cur.nS)
        n_tips = g.unitig_tips_device(*graph_args(cur), k, tip_q8, d_tip.data_ptr())
        n_pop = g.unitig_bubbles_device(*graph_args(cur), k, a.bubble_max_diff, bub_q8, d_pop.data_ptr(), 0)
        if n_tips or n_pop:
            d_tip[:cur.nS] |= d_pop[:cur.nS]
            g.mask_unitigs_device(*cur.args, d_tip.data_ptr())
        rounds.append({"round": r + 1, "nodes": cur.nodes(torch), "unitigs": cur.nS, "tips": n_tips, "bubbles": n_pop, "masked_keys": g.mask_count()})
        if not (n_tips or n_pop):
            break
    if rounds[-1]["tips"] or rounds[-1]["bubbles"]:
        last = _Graph(cfrk_amd, g, min_count, buf)
        rounds.append({"round": len(rounds) + 1, "nodes": last.nodes(torch), "unitigs": last.nS, "tips": None, "bubbles": None,
                       "masked_keys": g.mask_count()})
    print(json.dumps(dict(common, line="rounds", tip_ratio=a.tip_ratio, bubble_ratio=a.bubble_ratio, bubble_max_diff=a.bubble_max_diff,
                          max_kmers=k, rounds=rounds)), flush=True)


def bulges_case(a, torch, cfrk_amd, ctx, g, min_count, common, timed, stats, buf):
    k = a.k
    tip_q8, bub_q8, bulge_q8 = int(round(a.tip_ratio * 256)), int(round(a.bubble_ratio * 256)), int(round(a.bulge_ratio * 256))
    max_hops = min(k + a.bulge_max_diff, cfrk_amd.CFRK_BULGE_MAX_HOPS)
    new = _Graph(cfrk_amd, g, min_count, buf)
    ctx.sync()

    def graph_args(gr):
        return (gr.out[3].data_ptr(), gr.nS, gr.ptr.data_ptr(), gr.rows.data_ptr(), gr.n_links)

    def outputs(nS):
        return buf(nS), buf(nS), buf(nS), buf(nS * 4), buf((nS + 1) * 8)     # tip, bubble pop, bulge pop, visits, path_ptr

    def bulges(gr, d_pop, d_visits, d_ptr, d_path=None, cap=0):
        """-> (n_path, stats): the call with room for `cap` path entries; too little room reads as the sizes-only call"""
        try:
            return g.unitig_bulges_device(*graph_args(gr), k, a.bulge_max_diff, max_hops, a.bulge_max_visits, bulge_q8, d_pop.data_ptr(),
                                          d_visits.data_ptr() if d_visits is not None else 0, d_ptr.data_ptr(),
                                          d_path.data_ptr() if d_path is not None else 0, cap)
        except cfrk_amd.CfrkError as e:
            if e.code != cfrk_amd.CFRK_ERR_SMALL_BUF:
                raise
            return e.n_path, e.stats

    d_tip, d_bub, d_pop, d_visits, d_ptr = outputs(new.nS)
    n_path, st = bulges(new, d_pop, d_visits, d_ptr)
    d_path = buf(max(n_path, 1) * 4)
    calls = {"bulges": lambda: bulges(new, d_pop, d_visits, d_ptr, d_path, n_path),
             "bulges_sizes_only": lambda: bulges(new, d_pop, d_visits, d_ptr),
             "bubbles": lambda: g.unitig_bubbles_device(*graph_args(new), k, a.bubble_max_diff, bub_q8, d_bub.data_ptr(), 0)}
    n_bub = calls["bubbles"]()
    t = {name: [] for name in calls}
    for rep in range(a.reps + 1):
        for name, fn in calls.items():
            ms = timed(fn)
            if rep:                                             # (the first round warms up: code objects, pool buffers)
                t[name].append(ms)
    ctx.sync()
    visits = d_visits[:new.nS * 4].view(torch.int32)
    hops = torch.diff(d_ptr[:(new.nS + 1) * 8].view(torch.int64))
    arms_visits = visits[visits > 0]
    def quant(x):                                               # median, 90th and 99th percentile, maximum
        if not x.numel():
            return []
        x = x.sort().values
        return [int(x[min(x.numel() - 1, int(q * x.numel()))]) for q in (0.5, 0.9, 0.99)] + [int(x[-1])]

    row = dict(common, line="bulges", nodes=new.nodes(torch), unitigs=new.nS, links=new.n_links, bubbles_found=n_bub, n_path=n_path, max_kmers=k,
               max_hops=max_hops, bulge_max_diff=a.bulge_max_diff, bulge_max_visits=a.bulge_max_visits, bulge_ratio=a.bulge_ratio,
               popped_also_by_bubbles=int((d_pop[:new.nS] & d_bub[:new.nS]).sum()), **st)
    row.update({name: stats(ts) for name, ts in t.items()})
    row["ns_per_arm"] = row["bulges"]["ms"] * 1e6 / max(st["arms"], 1)
    row["visits_p50_p90_p99_max"] = quant(arms_visits)
    row["visits_sum"] = int(arms_visits.sum())
    row["hops_p50_p90_p99_max"] = quant(hops[hops > 0])
    row["hops_histogram"] = torch.bincount(hops[hops > 0], minlength=1).tolist()
    print(json.dumps(row), flush=True)
    # the rounds of the combined loop
    rounds, cur = [], new
    for r in range(a.tip_rounds):
        if r:
            cur = _Graph(cfrk_amd, g, min_count, buf)
            d_tip, d_bub, d_pop, d_visits, d_ptr = outputs(cur.nS)
        n_tips = g.unitig_tips_device(*graph_args(cur), k, tip_q8, d_tip.data_ptr())
        n_bub = g.unitig_bubbles_device(*graph_args(cur), k, a.bubble_max_diff, bub_q8, d_bub.data_ptr(), 0)
        st = g.unitig_bulges_device(*graph_args(cur), k, a.bulge_max_diff, max_hops, a.bulge_max_visits, bulge_q8, d_pop.data_ptr())[1]
        if n_tips or n_bub or st["popped"]:
            d_tip[:cur.nS] |= d_bub[:cur.nS] | d_pop[:cur.nS]
            g.mask_unitigs_device(*cur.args, d_tip.data_ptr())
        rounds.append({"round": r + 1, "nodes": cur.nodes(torch), "unitigs": cur.nS, "tips": n_tips, "bubbles": n_bub, "bulges": st["popped"],
                       "arms": st["arms"], "undecided": st["undecided"], "masked_keys": g.mask_count()})
        if not (n_tips or n_bub or st["popped"]):
            break
    if rounds[-1]["tips"] or rounds[-1]["bubbles"] or rounds[-1]["bulges"]:
        last = _Graph(cfrk_amd, g, min_count, buf)
        rounds.append({"round": len(rounds) + 1, "nodes": last.nodes(torch), "unitigs": last.nS, "tips": None, "bubbles": None, "bulges": None,
                       "masked_keys": g.mask_count()})
    print(json.dumps(dict(common, line="rounds", tip_ratio=a.tip_ratio, bubble_ratio=a.bubble_ratio, bubble_max_diff=a.bubble_max_diff,
                          bulge_ratio=a.bulge_ratio, bulge_max_diff=a.bulge_max_diff, bulge_max_visits=a.bulge_max_visits, max_kmers=k,
                          rounds=rounds)), flush=True)


def weak_case(a, torch, cfrk_amd, ctx, g, min_count, common, timed, stats, buf, rd, rd_clean):
    k = a.k
    tip_q8, bub_q8, bulge_q8 = int(round(a.tip_ratio * 256)), int(round(a.bubble_ratio * 256)), int(round(a.bulge_ratio * 256))
    weak_q8, iso_q8 = int(round(a.weak_ratio * 256)), int(round(a.weak_iso_mean * 256))
    max_hops = min(k + a.bulge_max_diff, cfrk_amd.CFRK_BULGE_MAX_HOPS)
    R = rd[4]

    def graph_args(gr):
        return (gr.out[3].data_ptr(), gr.nS, gr.ptr.data_ptr(), gr.rows.data_ptr(), gr.n_links)

    def small_buf(call, field):
        try:
            return call()
        except cfrk_amd.CfrkError as e:
            if e.code != cfrk_amd.CFRK_ERR_SMALL_BUF:
                raise
            return getattr(e, field) if isinstance(field, str) else tuple(getattr(e, f) for f in field)

    new = _Graph(cfrk_amd, g, min_count, buf)
    ctx.sync()
    d_tip, d_bub, d_weak = buf(new.nS), buf(new.nS), buf(new.nS)
    weak = lambda: g.unitig_weak_device(*graph_args(new), k, weak_q8, 2 * k, iso_q8, d_weak.data_ptr())
    calls = {"weak": weak, "tips": lambda: g.unitig_tips_device(*graph_args(new), k, tip_q8, d_tip.data_ptr()),
             "bubbles": lambda: g.unitig_bubbles_device(*graph_args(new), k, a.bubble_max_diff, bub_q8, d_bub.data_ptr(), 0), "links_call": new.links}
    st, n_tips, n_bub = weak(), calls["tips"](), calls["bubbles"]()
    t = {name: [] for name in calls}
    for rep in range(a.reps + 1):
        for name, fn in calls.items():                          # alternating in one process
            ms = timed(fn)
            if rep:                                             # (the first round warms up: code objects, pool buffers)
                t[name].append(ms)
    ctx.sync()
    torch.cuda.synchronize()
    row = dict(common, line="weak", nodes=new.nodes(torch), unitigs=new.nS, links=new.n_links, tips_found=n_tips, bubbles_found=n_bub,
               max_kmers=k, weak_ratio=a.weak_ratio, iso_max_kmers=2 * k, weak_iso_mean=a.weak_iso_mean,
               connections_also_popped_by_bubbles=int(((d_weak[:new.nS] == 1) & (d_bub[:new.nS] != 0)).sum()), **st)
    row.update({name: dict(stats(ts), series=ts) for name, ts in t.items()})
    row["weak_over_tips"] = row["weak"]["ms"] / row["tips"]["ms"]
    row["weak_over_links"] = row["weak"]["ms"] / row["links_call"]["ms"]
    row["ns_per_unitig"] = row["weak"]["ms"] * 1e6 / max(new.nS, 1)
    print(json.dumps(row), flush=True)
    del new, d_tip, d_bub, d_weak

    def paths_on(gr, rd):
        """the hits and paths of the reads `rd` on the graph the mask leaves"""
        g.unitig_index_device(min_count, *gr.args)
        d_hptr = buf((R + 1) * 8)
        n_hits = small_buf(lambda: g.read_hits_device(*rd, d_hptr.data_ptr(), 0, 0), "n_hits")
        d_hits = buf(max(n_hits, 1) * 16)
        if n_hits:
            g.read_hits_device(*rd, d_hptr.data_ptr(), d_hits.data_ptr(), n_hits)
        ctx.sync()
        d_pptr = buf((R + 1) * 8)
        n_paths, pst = small_buf(lambda: g.read_paths_device(d_hptr.data_ptr(), R, d_hits.data_ptr(), n_hits, *graph_args(gr), d_pptr.data_ptr(), 0, 0),
                                 ("n_paths", "stats"))
        ctx.sync()
        torch.cuda.synchronize()
        per_read = torch.diff(d_pptr[:(R + 1) * 8].view(torch.int64))
        return {"reads": R, "hits": n_hits, "paths": n_paths, "reads_in_one_path": int((per_read == 1).sum()),
                "reads_in_several_paths": int((per_read > 1).sum()), "reads_without_a_hit": int((per_read == 0).sum()),
                "gaps": pst["n_gaps"], "unlinked": pst["n_unlinked"], "steps": pst["n_steps"]}

    for rules in ("none", "tips+bubbles+bulges", "tips+bubbles+bulges+weak"):
        g.mask_clear()
        rounds, cur = [], _Graph(cfrk_amd, g, min_count, buf)
        for r in range(a.tip_rounds if rules != "none" else 0):
            if r:
                cur = _Graph(cfrk_amd, g, min_count, buf)
            d_tip, d_bub, d_pop, d_weak = buf(cur.nS), buf(cur.nS), buf(cur.nS), buf(cur.nS)
            n_tips = g.unitig_tips_device(*graph_args(cur), k, tip_q8, d_tip.data_ptr())
            n_bub = g.unitig_bubbles_device(*graph_args(cur), k, a.bubble_max_diff, bub_q8, d_bub.data_ptr(), 0)
            bst = g.unitig_bulges_device(*graph_args(cur), k, a.bulge_max_diff, max_hops, a.bulge_max_visits, bulge_q8, d_pop.data_ptr())[1]
            wst = {"connections": 0, "isolated": 0, "candidates": 0}
            if rules.endswith("weak"):
                wst = g.unitig_weak_device(*graph_args(cur), k, weak_q8, 2 * k, iso_q8, d_weak.data_ptr())
            found = n_tips or n_bub or bst["popped"] or wst["connections"] or wst["isolated"]
            if found:
                ctx.sync()
                d_tip[:cur.nS] |= d_bub[:cur.nS] | d_pop[:cur.nS]
                if rules.endswith("weak"):
                    d_tip[:cur.nS] |= d_weak[:cur.nS].ne(0).to(torch.uint8)
                torch.cuda.synchronize()
                g.mask_unitigs_device(*cur.args, d_tip.data_ptr())
            rounds.append({"round": r + 1, "nodes": cur.nodes(torch), "unitigs": cur.nS, "tips": n_tips, "bubbles": n_bub, "bulges": bst["popped"],
                           "undecided": bst["undecided"], "connections": wst["connections"], "isolated": wst["isolated"],
                           "weak_candidates": wst["candidates"], "masked_keys": g.mask_count()})
            del d_tip, d_bub, d_pop, d_weak
            if not found:
                break
        if rounds and any(rounds[-1][f] for f in ("tips", "bubbles", "bulges", "connections", "isolated")):
            cur = _Graph(cfrk_amd, g, min_count, buf)
        ctx.sync()
        after = {"nodes": cur.nodes(torch), "unitigs": cur.nS, "links": cur.n_links, "masked_keys": g.mask_count()}
        print(json.dumps(dict(common, line="rounds", rules=rules, tip_ratio=a.tip_ratio, bubble_ratio=a.bubble_ratio, bubble_max_diff=a.bubble_max_diff,
                              bulge_ratio=a.bulge_ratio, bulge_max_diff=a.bulge_max_diff, bulge_max_visits=a.bulge_max_visits, weak_ratio=a.weak_ratio,
                              weak_iso_mean=a.weak_iso_mean, max_kmers=k, rounds=rounds, after=after, read_paths=paths_on(cur, rd),
                              error_free_read_paths=paths_on(cur, rd_clean))), flush=True)
        del cur
        torch.cuda.empty_cache()
    g.mask_clear()


def components_case(a, torch, cfrk_amd, ctx, g, min_count, common, timed, stats, buf, case):
    """--components: the components call beside the weak and the links call; the census of the graph (and, case b, of the
    graph the four-rule loop leaves); a crafted pair at the same nS and n_links: one component against blocks of 8"""
    k = a.k
    tip_q8, bub_q8, bulge_q8 = int(round(a.tip_ratio * 256)), int(round(a.bubble_ratio * 256)), int(round(a.bulge_ratio * 256))
    weak_q8, iso_q8 = int(round(a.weak_ratio * 256)), int(round(a.weak_iso_mean * 256))
    max_hops = min(k + a.bulge_max_diff, cfrk_amd.CFRK_BULGE_MAX_HOPS)

    def graph_args(gr):
        return (gr.out[3].data_ptr(), gr.nS, gr.ptr.data_ptr(), gr.rows.data_ptr(), gr.n_links)

    def sizes_only(args, d_comp):
        try:
            return g.unitig_components_device(*args, 0, d_comp.data_ptr())
        except cfrk_amd.CfrkError as e:
            if e.code != cfrk_amd.CFRK_ERR_SMALL_BUF:
                raise
            return e.n_comps, e.stats

    def census(args):
        """the components of a graph -> (figures, d_comp, d_tab, n)"""
        nS = args[1]
        d_comp = buf(nS * 4)
        n, st = sizes_only(args, d_comp)
        d_tab = buf(max(n, 1) * 32)
        g.unitig_components_device(*args, 0, d_comp.data_ptr(), d_tab.data_ptr(), n)
        ctx.sync()
        torch.cuda.synchronize()
        tab = d_tab[:n * 32].view(torch.int64).view(n, 4)
        nk = tab[:, 1]
        members = tab[:, 3] >> 32                                # (first in the low word, n_unitigs in the high one)
        big = int(nk.argmax()) if n else 0
        fig = {"components": n, "kept_unitigs": st["n_unitigs"], "kmers": st["n_kmers"], "kept_links": st["n_links"],
               "largest_kmers": int(nk[big]) if n else 0, "largest_unitigs": int(members[big]) if n else 0,
               "largest_share_of_kmers": (int(nk[big]) / max(st["n_kmers"], 1)) if n else 0.0,
               "components_below_2k_kmers": int((nk < 2 * k).sum()), "kmers_in_components_below_2k": int(nk[nk < 2 * k].sum()),
               "components_of_one_unitig": int((members == 1).sum())}
        return fig, d_comp, d_tab, n

    new = _Graph(cfrk_amd, g, min_count, buf)
    ctx.sync()
    fig, d_comp, d_tab, n = census(graph_args(new))
    d_weak = buf(new.nS)
    calls = {"components": lambda: g.unitig_components_device(*graph_args(new), 0, d_comp.data_ptr(), d_tab.data_ptr(), n),
             "components_sizes_only": lambda: sizes_only(graph_args(new), d_comp),
             "weak": lambda: g.unitig_weak_device(*graph_args(new), k, weak_q8, 2 * k, iso_q8, d_weak.data_ptr()), "links_call": new.links}
    t = {name: [] for name in calls}
    for rep in range(a.reps + 1):
        for name, fn in calls.items():                          # alternating in one process
            ms = timed(fn)
            if rep:                                             # (the first round warms up: code objects, pool buffers)
                t[name].append(ms)
    ctx.sync()
    torch.cuda.synchronize()
    row = dict(common, line="components", nodes=new.nodes(torch), unitigs=new.nS, links=new.n_links, census=fig)
    row.update({name: dict(stats(ts), series=ts) for name, ts in t.items()})
    row["components_over_links"] = row["components"]["ms"] / row["links_call"]["ms"]
    row["components_over_weak"] = row["components"]["ms"] / row["weak"]["ms"]
    row["ns_per_unitig"] = row["components"]["ms"] * 1e6 / max(new.nS, 1)
    print(json.dumps(row), flush=True)

    # the crafted pair: the real records, rows of n_links / nS links each (the remainder spread over the first rows), link p
    # of row j to (a) j + 1 + p, all one component, (b) the same inside j's block of 8.  The two read the same bytes.
    nS, deg, rem = new.nS, new.n_links // max(new.nS, 1), new.n_links % max(new.nS, 1)
    if nS >= 16 and 1 <= deg < 16:
        j = torch.arange(nS, device="cuda", dtype=torch.int64)
        d = deg + (j < rem).to(torch.int64)
        ptr = buf((nS + 1) * 8)
        p64 = ptr[:(nS + 1) * 8].view(torch.int64)
        p64[0] = 0
        p64[1:] = torch.cumsum(d, 0)
        src = torch.repeat_interleave(j, d)
        pos = torch.arange(new.n_links, device="cuda", dtype=torch.int64) - p64[:-1][src]
        pair = {}
        for name, to in (("one_component", (src + 1 + pos) % nS), ("blocks_of_8", torch.minimum((src & ~7) + ((src + 1 + pos) & 7), j[-1]))):
            rows = buf(new.n_links * 8)
            r32 = rows[:new.n_links * 8].view(torch.int32).view(new.n_links, 2)
            r32[:, 0] = to.to(torch.int32)
            r32[:, 1] = 0
            torch.cuda.synchronize()
            args = (new.out[3].data_ptr(), nS, ptr.data_ptr(), rows.data_ptr(), new.n_links)
            cfig, c_comp, c_tab, cn = census(args)
            ts = []
            for rep in range(a.reps + 1):
                ms = timed(lambda: g.unitig_components_device(*args, 0, c_comp.data_ptr(), c_tab.data_ptr(), cn))
                if rep:
                    ts.append(ms)
            pair[name] = dict(stats(ts), series=ts, components=cn, largest_unitigs=cfig["largest_unitigs"])
            del rows, c_comp, c_tab
        print(json.dumps(dict(common, line="crafted_pair", unitigs=nS, links=new.n_links, links_per_row=deg, **pair,
                              one_over_blocks=pair["one_component"]["ms"] / pair["blocks_of_8"]["ms"])), flush=True)
        del ptr, src, pos, j, d
    del new, d_comp, d_tab, d_weak
    torch.cuda.empty_cache()
    if case != "b":
        return
    # the 1 % case: the census again on the graph the four-rule loop leaves
    rounds, cur = 0, _Graph(cfrk_amd, g, min_count, buf)
    for r in range(a.tip_rounds):
        if r:
            cur = _Graph(cfrk_amd, g, min_count, buf)
        d_tip, d_bub, d_pop, d_weak = buf(cur.nS), buf(cur.nS), buf(cur.nS), buf(cur.nS)
        n_tips = g.unitig_tips_device(*graph_args(cur), k, tip_q8, d_tip.data_ptr())
        n_bub = g.unitig_bubbles_device(*graph_args(cur), k, a.bubble_max_diff, bub_q8, d_bub.data_ptr(), 0)
        bst = g.unitig_bulges_device(*graph_args(cur), k, a.bulge_max_diff, max_hops, a.bulge_max_visits, bulge_q8, d_pop.data_ptr())[1]
        wst = g.unitig_weak_device(*graph_args(cur), k, weak_q8, 2 * k, iso_q8, d_weak.data_ptr())
        found = n_tips or n_bub or bst["popped"] or wst["connections"] or wst["isolated"]
        rounds += 1
        if found:
            ctx.sync()
            d_tip[:cur.nS] |= d_bub[:cur.nS] | d_pop[:cur.nS] | d_weak[:cur.nS].ne(0).to(torch.uint8)
            torch.cuda.synchronize()
            g.mask_unitigs_device(*cur.args, d_tip.data_ptr())
        del d_tip, d_bub, d_pop, d_weak
        if not found:
            break
    if found:
        cur = _Graph(cfrk_amd, g, min_count, buf)
    ctx.sync()
    fig, d_comp, d_tab, n = census(graph_args(cur))
    print(json.dumps(dict(common, line="components_after_loop", rules="tips+bubbles+bulges+weak", rounds=rounds, nodes=cur.nodes(torch),
                          unitigs=cur.nS, links=cur.n_links, masked_keys=g.mask_count(), census=fig)), flush=True)
    del cur, d_comp, d_tab
    g.mask_clear()


def compact_case(a, torch, cfrk_amd, ctx, g, min_count, common, timed, stats, buf, stream):
    k = a.k
    tip_q8, bub_q8, bulge_q8 = int(round(a.tip_ratio * 256)), int(round(a.bubble_ratio * 256)), int(round(a.bulge_ratio * 256))
    max_hops = min(k + a.bulge_max_diff, cfrk_amd.CFRK_BULGE_MAX_HOPS)

    def graph_args(gr):
        return (gr.out[3].data_ptr(), gr.nS, gr.ptr.data_ptr(), gr.rows.data_ptr(), gr.n_links)

    def drop_of(gr):
        """round 1 of tips + bubbles + bulges on this graph -> (drop bytes, what each rule found)"""
        d_tip, d_bub, d_pop = buf(gr.nS), buf(gr.nS), buf(gr.nS)
        n_tips = g.unitig_tips_device(*graph_args(gr), k, tip_q8, d_tip.data_ptr())
        n_bub = g.unitig_bubbles_device(*graph_args(gr), k, a.bubble_max_diff, bub_q8, d_bub.data_ptr(), 0)
        st = g.unitig_bulges_device(*graph_args(gr), k, a.bulge_max_diff, max_hops, a.bulge_max_visits, bulge_q8, d_pop.data_ptr())[1]
        ctx.sync()
        d_tip[:gr.nS] |= d_bub[:gr.nS] | d_pop[:gr.nS]
        torch.cuda.synchronize()
        return d_tip, (n_tips, n_bub, st["popped"])

    def compact(gr, d_drop, out=None, sizes=(0, 0)):
        """-> (nN, nS) of the compaction of gr; without `out` the sizes-only call"""
        o = [x.data_ptr() for x in out] if out else [0, 0, 0, 0]
        try:
            return g.compact_unitigs_device(gr.out[0].data_ptr(), gr.out[1].data_ptr(), gr.out[2].data_ptr(), gr.out[3].data_ptr(), gr.nN, gr.nS,
                                            gr.ptr.data_ptr(), gr.rows.data_ptr(), gr.n_links, d_drop.data_ptr(), o[0], sizes[0], o[1], o[2], o[3], sizes[1])
        except cfrk_amd.CfrkError as e:
            if e.code != cfrk_amd.CFRK_ERR_SMALL_BUF:
                raise
            return e.nN, e.nS

    new = _Graph(cfrk_amd, g, min_count, buf)
    d_drop, found = drop_of(new)
    cN, cS = compact(new, d_drop)
    cout = [buf(cN), buf(cS * 8), buf(cS * 4), buf(cS * 16)]
    assert compact(new, d_drop, cout, (cN, cS)) == (cN, cS)
    g.mask_unitigs_device(*new.args, d_drop.data_ptr())
    masked = _Graph(cfrk_amd, g, min_count, buf)                 # the yardstick: the unitigs call under the mask of round 1
    ctx.sync()
    assert (masked.nN, masked.nS) == (cN, cS), ((masked.nN, masked.nS), (cN, cS))
    for got, want, n in zip(cout, masked.out, (cN, cS * 8, cS * 4, cS * 16)):
        assert bool((got[:n] == want[:n]).all()), "the compaction is not the masked unitigs call byte for byte"
    dst = buf(cN)

    def copy():
        with torch.cuda.stream(stream):
            dst[:cN].copy_(cout[0][:cN])

    calls = {"compact": lambda: compact(new, d_drop, cout, (cN, cS)), "unitigs_masked": masked.unitigs,
             "compact_sizes_only": lambda: compact(new, d_drop), "copy_output": copy}
    t = {name: [] for name in calls}
    for rep in range(a.reps + 1):
        for name, fn in calls.items():                          # alternating in one process
            ms = timed(fn)
            if rep:                                             # (the first round warms up: code objects, pool buffers)
                t[name].append(ms)
    row = dict(common, line="compact", nodes=new.nodes(torch), unitigs=new.nS, links=new.n_links, tips=found[0], bubbles=found[1], bulges=found[2],
               dropped=int(d_drop[:new.nS].ne(0).sum()), unitigs_after=cS, bytes_after=cN, byte_equal=True)
    row.update({name: dict(stats(ts), series=ts) for name, ts in t.items()})
    row["order_and_emit_ms"] = row["compact"]["ms"] - row["compact_sizes_only"]["ms"]
    row["unitigs_over_compact"] = row["unitigs_masked"]["ms"] / row["compact"]["ms"]
    row["outside_yardstick_spread"] = row["compact"]["max_ms"] < row["unitigs_masked"]["min_ms"]
    print(json.dumps(row), flush=True)
    # the whole loop, with and without recompaction, from an unmasked graph each time; the two alternate
    def loop(recompact):
        g.mask_clear()
        cur, rounds = _Graph(cfrk_amd, g, min_count, buf), []
        for r in range(a.tip_rounds):
            d, found = drop_of(cur)
            if any(found):
                g.mask_unitigs_device(*cur.args, d.data_ptr())
            rounds.append((cur.nS,) + found)
            if not any(found):
                break                                           # (else: the next graph, after the last round the loop's result)
            if recompact:
                nN, nS = compact(cur, d)
                nxt = _Graph.__new__(_Graph)
                nxt.mod, nxt.g, nxt.mc, nxt.buf, nxt.nN, nxt.nS = cfrk_amd, g, min_count, buf, nN, nS
                nxt.out = [buf(nN), buf(nS * 8), buf(nS * 4), buf(nS * 16)]
                assert compact(cur, d, nxt.out, (nN, nS)) == (nN, nS)
                nxt.args = (nxt.out[0].data_ptr(), nxt.out[1].data_ptr(), nxt.out[2].data_ptr(), nN, nS)
                nxt.ptr = buf((nS + 1) * 8)
                try:
                    nxt.n_links = g.unitig_links_device(min_count, *nxt.args, nxt.ptr.data_ptr(), 0, 0)
                except cfrk_amd.CfrkError as e:
                    if e.code != cfrk_amd.CFRK_ERR_SMALL_BUF:
                        raise
                    nxt.n_links = e.n_links
                nxt.rows = buf(nxt.n_links * 8)
                nxt.links()
                cur = nxt
            else:
                cur = _Graph(cfrk_amd, g, min_count, buf)
        return rounds

    t, seen = {False: [], True: []}, {}
    for rep in range(a.loop_reps + 1):
        for recompact in ((False, True) if rep % 2 else (True, False)):
            box = []
            ms = timed(lambda: box.append(loop(recompact)))
            seen[recompact] = box[0]
            if rep:
                t[recompact].append(ms)
    assert seen[False] == seen[True], (seen[False], seen[True])
    row = dict(common, line="loop", rounds=[dict(zip(("unitigs", "tips", "bubbles", "bulges"), r)) for r in seen[True]],
               loop=dict(stats(t[False]), series=t[False]), loop_recompact=dict(stats(t[True]), series=t[True]))
    row["loop_over_recompact"] = row["loop"]["ms"] / row["loop_recompact"]["ms"]
    print(json.dumps(row), flush=True)


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
    ap.add_argument("--tips", action="store_true")
    ap.add_argument("--tip-ratio", type=float, default=2.0)
    ap.add_argument("--tip-rounds", type=int, default=4)
    ap.add_argument("--bubbles", action="store_true")
    ap.add_argument("--bubble-ratio", type=float, default=0.0)
    ap.add_argument("--bubble-max-diff", type=int, default=0)
    ap.add_argument("--bulges", action="store_true")
    ap.add_argument("--bulge-ratio", type=float, default=0.0)
    ap.add_argument("--bulge-max-diff", type=int, default=0)
    ap.add_argument("--bulge-max-visits", type=int, default=1024)
    ap.add_argument("--compact", action="store_true")
    ap.add_argument("--weak", action="store_true")
    ap.add_argument("--components", action="store_true")
    ap.add_argument("--weak-ratio", type=float, default=4.0)
    ap.add_argument("--weak-iso-mean", type=float, default=2.0)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--parent-lib", help="libcfrk_hip.so of the parent commit: with --tips the unmasked calls, with --bubbles the tips call alternate with it")
    a = ap.parse_args()

    import torch
    import cfrk_amd
    stream = torch.cuda.Stream()
    ctx = cfrk_amd.Context(0, stream.cuda_stream)
    parent = pctx = None
    if (a.tips or a.bubbles) and a.parent_lib:                                 # a second copy of the Python mirror bound to the other library
        import importlib.util
        spec = importlib.util.spec_from_file_location("cfrk_parent_lib", cfrk_amd.lib.__file__)
        parent = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(parent)
        parent._SO = os.path.abspath(a.parent_lib)
        pctx = parent.Context(0, stream.cuda_stream)
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
            r_start, r_length = (buf(R * 8), buf(R * 4)) if a.weak else (None, None)   # (the reads as a list: --weak maps them back)
            ctx.synth_reads_device(0, R, L, a.glen, reads.data_ptr(), r_start.data_ptr() if a.weak else None, r_length.data_ptr() if a.weak else None)
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

        if a.weak:
            common = {"tool": "bench_weak", "case": case, "reads": R, "L": L, "glen": a.glen, "k": k, "reps": a.reps,
                      "error_rate": 0.0 if case == "a" else a.error_rate, "min_count": min_count, "distinct_keys": distinct}
            with torch.cuda.stream(stream):
                clean = buf(nN)                                 # the same reads without the substitutions
                ctx.synth_reads_device(0, R, L, a.glen, clean.data_ptr())
                ctx.sync()
            torch.cuda.synchronize()
            weak_case(a, torch, cfrk_amd, ctx, g, min_count, common, timed, stats, buf, (reads.data_ptr(), r_start.data_ptr(), r_length.data_ptr(), nN, R),
                      (clean.data_ptr(), r_start.data_ptr(), r_length.data_ptr(), nN, R))
            del g, out, reads, clean, r_start, r_length
            torch.cuda.empty_cache()
            continue
        if a.components:
            common = {"tool": "bench_components", "case": case, "reads": R, "L": L, "glen": a.glen, "k": k, "reps": a.reps,
                      "error_rate": 0.0 if case == "a" else a.error_rate, "min_count": min_count, "distinct_keys": distinct}
            components_case(a, torch, cfrk_amd, ctx, g, min_count, common, timed, stats, buf, case)
            del g, out, reads
            torch.cuda.empty_cache()
            continue
        if a.compact:
            common = {"tool": "bench_compact", "case": case, "reads": R, "L": L, "glen": a.glen, "k": k, "reps": a.reps,
                      "error_rate": 0.0 if case == "a" else a.error_rate, "min_count": min_count, "distinct_keys": distinct}
            compact_case(a, torch, cfrk_amd, ctx, g, min_count, common, timed, stats, buf, stream)
            del g, out, reads
            torch.cuda.empty_cache()
            continue
        if a.bulges:
            common = {"tool": "bench_bulges", "case": case, "reads": R, "L": L, "glen": a.glen, "k": k, "reps": a.reps,
                      "error_rate": 0.0 if case == "a" else a.error_rate, "min_count": min_count, "distinct_keys": distinct}
            bulges_case(a, torch, cfrk_amd, ctx, g, min_count, common, timed, stats, buf)
            del g, out, reads
            torch.cuda.empty_cache()
            continue
        if a.tips or a.bubbles:
            other = None
            if parent is not None:                              # the same reads counted by the parent's library as well
                other = parent.GlobalCounter(pctx, k, cfrk_amd.CFRK_CANONICAL, hint)
                other.add_device(reads.data_ptr(), nN)
                pctx.sync()
                assert other.digest()[0] == distinct
            common = {"tool": "bench_bubbles" if a.bubbles else "bench_tips", "case": case, "reads": R, "L": L, "glen": a.glen, "k": k, "reps": a.reps,
                      "error_rate": 0.0 if case == "a" else a.error_rate, "min_count": min_count, "distinct_keys": distinct}
            (bubbles_case if a.bubbles else tips_case)(a, torch, cfrk_amd, ctx, g, parent, other, min_count, common, timed, stats, buf)
            del g, other, out, reads
            torch.cuda.empty_cache()
            continue
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
