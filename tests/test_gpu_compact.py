"""GPU: the unitig compaction (cfrk_global_unitigs_compact) in its device form and its host form against
tests/compact_ref.py and against the product's own unitigs() under the mask: the hand-made and random cases of
tests/test_compact_cpu.py, real graphs with the rules' drops and random ones, one long chain, one long member among short
ones and outputs around the emit's tile size, the capacity protocol, the refusals, rows that pass the check without being
link sets, starts past 2^32, the loops with recompaction and the CLI option.  All comparisons are equality."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from . import bubbles_ref as br
from . import bulges_ref as gr
from . import compact_ref as cr
from . import tips_ref as tr
from . import unitig_links_ref as lr
from . import unitig_ref as ur
from .test_compact_cpu import N_RANDOM, hand_cases, random_case
from .test_gpu_bulges import error_reads, fuzz_case, real_graph, real_input, rows_of
from .test_gpu_filter import _Guarded, _upload
from .test_gpu_unitigs import _job, _same

pytestmark = pytest.mark.gpu

CFRK_ERR_ARG, CFRK_ERR_STATE, CFRK_ERR_LAYOUT, CFRK_ERR_SMALL_BUF = -1, -4, -5, -9
TILE = 4096                                             # CFRK_COMPACT_TILE_BYTES
NONE = cr.POS_NONE


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


def _counter(ctx, k, canonical):
    """a job that only supplies k and the strand rule (a context holds one job: a new one replaces the last)"""
    import cfrk_amd
    return cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL if canonical else 0, 1000)


def _device(ctx, g, lay, ptr, links, drop, skew_in=3, skew_out=5, cap=None, want_into=True, starts=None):
    """the device form on unaligned data pointers into guarded arrays: a sizes-only call, then the call with room for
    exactly the result (or cap = (cap_data, cap_unitigs)) -> (data, start, length, rec, into)"""
    import cfrk_amd
    data, start, length, rec = lay
    nN, nS = len(data), len(rec)
    ins = [_upload(ctx, data, skew_in), _upload(ctx, start), _upload(ctx, length), _upload(ctx, rec), _upload(ctx, ptr), _upload(ctx, links),
           _upload(ctx, np.ascontiguousarray(drop, np.uint8)) if drop is not None else 0]
    d_into = _Guarded(ctx, nS * 8)
    bufs = []
    call = lambda o, cd, cu: g.compact_unitigs_device(ins[0] + skew_in, ins[1], ins[2], ins[3], nN, nS, ins[4], ins[5], len(links), ins[6],
                                                      o[0], cd, o[1], o[2], o[3], cu, d_into.ptr if want_into else 0)
    try:
        try:
            n_data, n_units = call((0, 0, 0, 0), 0, 0)
            assert (n_data, n_units) == (0, 0)                      # everything dropped
        except cfrk_amd.CfrkError as e:
            if e.code != CFRK_ERR_SMALL_BUF:
                raise
            n_data, n_units = e.nN, e.nS
            assert n_units > 0 and n_data > n_units
            ctx.sync()
            d_into.fetch(0)                                         # sizes only: nothing written
            cd, cu = (n_data, n_units) if cap is None else cap
            bufs = [_Guarded(ctx, cd, skew_out), _Guarded(ctx, cu * 8), _Guarded(ctx, cu * 4), _Guarded(ctx, cu * 16)]
            assert call([b.ptr for b in bufs], cd, cu) == (n_data, n_units)
        ctx.sync()
        into = d_into.fetch(nS * 8 if want_into else 0, cr.POS_DTYPE)
        if not bufs:
            return np.zeros(0, np.int8), np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, ur.UNITIG_DTYPE), into
        return (bufs[0].fetch(n_data, np.int8), bufs[1].fetch(n_units * 8, np.int64), bufs[2].fetch(n_units * 4, np.int32),
                bufs[3].fetch(n_units * 16, ur.UNITIG_DTYPE), into)
    finally:
        ctx.sync()
        for b in bufs + [d_into]:
            b.free()
        for p in ins:
            if p:
                ctx.free(p)


def _equal(got, want_units, want_into, what=""):
    want = ur.layout(want_units)
    for name, a, b in zip(("data", "start", "length", "rec"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all(), (what, name)
    if want_into is not None:
        assert got[4].tolist() == want_into.tolist(), (what, "into")


def _both_forms(ctx, g, units, ptr, links, drop, want_units, want_into, what="", skews=(3, 5)):
    lay = ur.layout(units)
    _equal(g.compact_unitigs(*lay, ptr, links, drop), want_units, want_into, (what, "host"))
    _equal(_device(ctx, g, lay, ptr, links, drop, *skews), want_units, want_into, (what, "device"))


# ------------------------------------------------------------------ the rule against the reference

@pytest.mark.parametrize("canonical", [False, True])
def test_hand_made_cases(ctx, canonical):
    for name, k, (table, units, ptr, links, drop) in hand_cases(canonical):
        want, into, _ = cr.compact(units, ptr, links, drop, k, canonical)
        _both_forms(ctx, _counter(ctx, k, canonical), units, ptr, links, drop, want, into, name)
    name, k, (table, units, ptr, links, drop) = hand_cases(canonical)[-1]
    want, into, _ = cr.compact(units, ptr, links, None, k, canonical)        # a NULL drop drops nothing
    assert want == units
    _both_forms(ctx, _counter(ctx, k, canonical), units, ptr, links, None, want, into, "NULL drop")


def test_random_dictionaries(ctx):
    merged = closed = 0
    cases = {}
    for seed in range(0, N_RANDOM, N_RANDOM // 300)[:300]:
        k, canonical, case = random_case(seed)
        cases.setdefault((k, canonical), []).append((seed, case))
    assert len(cases) == 12 and sum(len(c) for c in cases.values()) == 300
    for (k, canonical), group in sorted(cases.items()):             # one job per (k, strand rule)
        g = _counter(ctx, k, canonical)
        for seed, (table, units, ptr, links, drop) in group:
            want, into, stats = cr.compact(units, ptr, links, drop, k, canonical)
            merged, closed = merged + (stats["merged"] > 0), closed + (stats["closed"] > 0)
            _both_forms(ctx, g, units, ptr, links, drop, want, into, seed, (seed % 16, (seed // 16) % 16))
    assert merged >= 20 and closed >= 2                             # (the reference says so: the comparison is not vacuous)


# ------------------------------------------------------------------ real graphs

def _rule_drop(units, ptr, links, k, canonical):
    tip = tr.tips(units, ptr, links, canonical, k, 512)
    pop = br.bubbles(units, ptr, links, canonical, k, 1, 0)[0]
    bulge = gr.bulges(units, ptr, links, canonical, k, 1)[0]
    return tip | pop | bulge


@pytest.mark.parametrize("min_count", [1, 2])
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [5, 15, 21, 31, 33, 63])
def test_real_graphs(ctx, k, canonical, min_count):
    table, units, ptr, links = real_graph(k, canonical, min_count)
    job = _job(ctx, [(r, 1) for r in error_reads(*real_input(k, canonical, min_count))], k, canonical)
    lay = job.unitigs(min_count)
    _same(lay, ur.layout(units))
    rng = np.random.default_rng(3100 + k)
    g = job                                                         # (the call only reads k and the strand rule off it)
    merged = 0
    for what, drop in (("rules", _rule_drop(units, ptr, links, k, canonical)), ("10 %", (rng.random(len(units)) < 0.1).astype(np.uint8)),
                       ("50 %", (rng.random(len(units)) < 0.5).astype(np.uint8))):
        assert drop.any()
        want, into, stats = cr.compact(units, ptr, links, drop, k, canonical)
        merged += stats["merged"]
        cr.check_into(units, want, into, drop, k)                   # into is consistent with the sequences
        _both_forms(ctx, g, units, ptr, links, drop, want, into, what)
        job.mask_clear()                                            # the product's own unitigs under the mask
        job.mask_unitigs(*lay[:3], drop)
        masked = job.unitigs(min_count)
        got = job.compact_unitigs(*lay, ptr, links, drop)
        _same(got[:4], masked)
        job.unitig_index(*got[:3], min_count)                       # the sufficient check accepts the result
    assert merged >= 1


# ------------------------------------------------------------------ one long chain

_CHAIN = {}


def _repeat_free(seed, n, k):
    """a random genome in which no (k - 1)-mer occurs twice on either strand: its graph has no branch of its own"""
    rng = np.random.default_rng(seed)
    g, seen = [], set()
    while len(g) < n:
        g.append(ur.BASES[int(rng.integers(4))])
        if len(g) < k - 1:
            continue
        w = "".join(g[-(k - 1):])
        if w in seen or ur.rc(w) in seen or w == ur.rc(w):
            g.pop()                                                 # (another draw)
            continue
        seen.add(w)
    return "".join(g)


def _long_chain(canonical):
    if canonical not in _CHAIN:
        k = 15
        g = _repeat_free(41, 40000, k)
        tips = []
        for p in range(k + 3, len(g) - 1, 8):                       # a read that leaves the genome with its last base
            tips.append(g[p - k + 1:p] + ur.BASES[(ur.BASES.index(g[p]) + 1 + p % 3) % 4])
        table = ur.count_kmers([g, g], k, canonical)
        ur.count_kmers(tips, k, canonical, 1, table)
        units, ptr, links = tr.graph(table, k, canonical)
        drop = np.array([1 if u[1] == u[2] == 1 else 0 for u in units], np.uint8)     # the tips: one k-mer, seen once
        _CHAIN[canonical] = (k, g, units, ptr, links, drop)
    return _CHAIN[canonical]


@pytest.mark.parametrize("canonical", [False, True])
def test_one_long_chain(ctx, canonical):
    k, genome, units, ptr, links, drop = _long_chain(canonical)
    want, into, _ = cr.compact(units, ptr, links, drop, k, canonical)
    members = into[drop == 0]
    assert len(want) == 1 and want[0][0] in (genome, ur.rc(genome)) and len(members) >= 4096
    assert not canonical or 0 < int((members["at"] & 1).sum()) < len(members)      # members of both orientations
    _both_forms(ctx, _counter(ctx, k, canonical), units, ptr, links, drop, want, into)


# ------------------------------------------------------------------ balance and tile seams

def chain_graph(genome, cuts, k, canonical, seed):
    """the genome cut into pieces at the k-mer offsets `cuts`, a one-k-mer tip at every cut, the unitigs shuffled and, in a
    canonical job, flipped at random -> (units, link_ptr, links, drop): dropping the tips joins the pieces again"""
    rng = np.random.default_rng(seed)
    bounds = [0] + list(cuts) + [len(genome) - k + 1]
    assert all(a < b for a, b in zip(bounds, bounds[1:]))
    seqs = [genome[a:b + k - 1] for a, b in zip(bounds, bounds[1:])]
    n_pieces = len(seqs)
    for c in cuts:
        seqs.append(genome[c:c + k - 1] + ur.BASES[(ur.BASES.index(genome[c + k - 1]) + 1) % 4])
    order = rng.permutation(len(seqs))
    place = np.argsort(order)                                       # unit `i` of the list above is unitig place[i]
    flip = (rng.random(len(seqs)) < 0.5) if canonical else np.zeros(len(seqs), bool)
    units = [None] * len(seqs)
    for i, s in enumerate(seqs):
        n = len(s) - k + 1
        units[place[i]] = (ur.rc(s) if flip[i] else s, int(rng.integers(1, 50)) * n, n, False)
    edges = []
    for i in range(n_pieces - 1):
        for t in (i + 1, n_pieces + i):                             # the next piece, and the tip at that cut
            edges.append((int(place[i]), int(flip[i]), int(place[t]), int(flip[t])))
    link_ptr, links = rows_of(len(seqs), edges, canonical)
    drop = np.zeros(len(seqs), np.uint8)
    drop[place[n_pieces:]] = 1
    return units, link_ptr, links, drop


def _rand_genome(seed, n):
    return "".join(ur.BASES[i] for i in np.random.default_rng(seed).integers(0, 4, n))


@pytest.mark.parametrize("canonical", [False, True])
def test_one_long_member_among_short_ones(ctx, canonical):
    k = 21
    genome = _rand_genome(51, 40000 + 100000 + 10000 * 9 + 2000)
    cuts = [40000 + 9 * i for i in range(5000)] + [40000 + 9 * 5000 + 100000 + 9 * i for i in range(5000)]
    units, ptr, links, drop = chain_graph(genome, cuts, k, canonical, 52)
    assert max(u[2] for u in units) >= 100000 and len(units) > 20000
    want, into, _ = cr.compact(units, ptr, links, drop, k, canonical)
    assert len(want) == 1 and want[0][0] in (genome, ur.rc(genome))
    _equal(_device(ctx, _counter(ctx, k, canonical), ur.layout(units), ptr, links, drop), want, into)


@pytest.mark.parametrize("canonical", [False, True])
def test_outputs_around_the_tile_size(ctx, canonical):
    k = 21
    g = _counter(ctx, k, canonical)
    for total in (TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1):        # bytes of data_out: one unitig and its terminator
        for skew in (0, 5):
            genome = _rand_genome(60 + total, total - 1)
            # member boundaries on the tile boundary (as the emit lays its tiles for this skew), one base before and after
            seam = TILE - skew - (k - 1)
            cuts = sorted({100, seam - 1, seam, seam + 1} & set(range(1, len(genome) - k + 1)))
            units, ptr, links, drop = chain_graph(genome, cuts, k, canonical, total + skew)
            want, into, _ = cr.compact(units, ptr, links, drop, k, canonical)
            assert len(want) == 1 and len(want[0][0]) + 1 == total
            _equal(_device(ctx, g, ur.layout(units), ptr, links, drop, 1, skew), want, into, (total, skew))
    # several unitigs whose bytes end on, before and behind a tile boundary
    units, ptr, links, drop = [], [np.zeros(1, np.int64)], [], []
    sizes = (TILE - 1, k, TILE - k - 1, 2 * TILE)                   # bases: with its terminator the first ends a tile, the third the next
    for j, n in enumerate(sizes):
        u, p, rows, d = chain_graph(_rand_genome(70 + j, n), [n // 2 - k] if n > 3 * k else [], k, canonical, 70 + j)
        rows = rows.copy()
        rows["to"] += len(units)
        units, drop = units + u, drop + d.tolist()
        ptr.append(p[1:] + ptr[-1][-1])
        links.append(rows)
    ptr, links, drop = np.concatenate(ptr), np.concatenate(links), np.array(drop, np.uint8)
    want, into, _ = cr.compact(units, ptr, links, drop, k, canonical)
    assert sorted(len(w[0]) for w in want) == sorted(sizes)
    _both_forms(ctx, g, units, ptr, links, drop, want, into, "four unitigs")


# ------------------------------------------------------------------ the protocol

@pytest.mark.parametrize("canonical", [False, True])
def test_capacity_protocol_and_arguments(ctx, canonical):
    import cfrk_amd
    k = 15
    _, units, ptr, links = real_graph(k, canonical, 1)
    g = _job(ctx, [("ACGTTGCATGCCGATAGCTAGCTAGGATCGAT", 2)], k, canonical)          # a job with counts: its digest must not move
    digest = g.digest()
    drop = _rule_drop(units, ptr, links, k, canonical)
    want, into, _ = cr.compact(units, ptr, links, drop, k, canonical)
    lay = ur.layout(units)
    w = ur.layout(want)
    nN, nS = len(w[0]), len(want)
    _equal(_device(ctx, g, lay, ptr, links, drop), want, into)                      # sizes-only, then exact
    for cap in ((nN - 1, nS), (nN, nS - 1)):                                        # one short in each capacity: nothing written
        with pytest.raises(cfrk_amd.CfrkError) as e:
            _device(ctx, g, lay, ptr, links, drop, cap=cap)
        assert e.value.code == CFRK_ERR_SMALL_BUF and (e.value.nN, e.value.nS) == (nN, nS)
    got = _device(ctx, g, lay, ptr, links, drop, cap=(nN + 7, nS + 3), want_into=False)   # more room: the rest untouched; into may be NULL
    _equal(got, want, None)
    assert len(got[4]) == 0
    # the host form: sizes only, one short in each, exact
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    L, h = ctx._L, ctx._h
    head = (vp(lay[0]), vp(lay[1]), vp(lay[2]), vp(lay[3]), len(lay[0]), len(units), vp(ptr), vp(links), len(links), vp(drop))
    a, b = C.c_int64(), C.c_int64()
    for cd, cu in ((0, 0), (nN - 1, nS), (nN, nS - 1)):
        out = [np.full(cd + 1, 0x5A, np.int8), np.full(cu + 1, 0x5A, np.int64), np.full(cu + 1, 0x5A, np.int32), np.zeros(cu + 1, ur.UNITIG_DTYPE)]
        pos = np.full(len(units), 7, cr.POS_DTYPE)
        rc = L.cfrk_global_unitigs_compact(h, *head, vp(out[0]) if cd else None, cd, vp(out[1]) if cu else None, vp(out[2]) if cu else None,
                                           vp(out[3]) if cu else None, cu, vp(pos), C.byref(a), C.byref(b))
        assert rc == CFRK_ERR_SMALL_BUF and (a.value, b.value) == (nN, nS)
        assert (out[0] == 0x5A).all() and (out[1] == 0x5A).all() and (out[2] == 0x5A).all() and not out[3]["kc"].any() and (pos["unitig"] == 7).all()
    # CFRK_ERR_ARG
    out = [np.zeros(nN, np.int8), np.zeros(nS, np.int64), np.zeros(nS, np.int32), np.zeros(nS, ur.UNITIG_DTYPE)]
    pos = np.zeros(len(units), cr.POS_DTYPE)
    ok = head + (vp(out[0]), nN, vp(out[1]), vp(out[2]), vp(out[3]), nS, vp(pos), C.byref(a), C.byref(b))
    assert L.cfrk_global_unitigs_compact(h, *ok) == 0
    _equal(tuple(out) + (pos,), want, into)
    for fn in (L.cfrk_global_unitigs_compact, L.cfrk_global_unitigs_compact_device):
        for at, value in ((0, None), (1, None), (2, None), (3, None), (6, None), (7, None), (10, None), (12, None), (13, None), (14, None),
                          (17, None), (18, None), (4, -1), (5, -1), (8, -1), (5, 1 << 31)):
            args = list(ok)
            args[at] = value
            assert fn(h, *args) == CFRK_ERR_ARG, (at, value)
        a.value = b.value = 9                                                       # nS = 0 is fine
        assert fn(h, None, None, None, None, 0, 0, None, None, 0, None, None, 0, None, None, None, 0, None, C.byref(a), C.byref(b)) == 0
        assert (a.value, b.value) == (0, 0)
    with cfrk_amd.Context(0) as c:                                                  # no job
        for fn in (c._L.cfrk_global_unitigs_compact, c._L.cfrk_global_unitigs_compact_device):
            assert fn(c._h, None, None, None, None, 0, 0, None, None, 0, None, None, 0, None, None, None, 0, None, C.byref(a), C.byref(b)) == CFRK_ERR_STATE
    assert g.digest() == digest


# ------------------------------------------------------------------ refusals

@pytest.mark.parametrize("canonical", [False, True])
def test_refuses_what_is_no_unitig_list(ctx, canonical):
    """every CFRK_ERR_LAYOUT reason of the section but the component of 2^31 bases, with the unitig it names"""
    k = 15
    _, units, ptr, links = real_graph(k, canonical, 1)
    g = _counter(ctx, k, canonical)
    drop = _rule_drop(units, ptr, links, k, canonical)
    data, start, length, rec = ur.layout(units)
    nS = len(units)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def refused(unitig, data=data, start=start, length=length, rec=rec, ptr=ptr, links=links, host=False):
        lay = (data, start, length, rec)
        ins = [_upload(ctx, x) for x in lay + (ptr, links, drop)]
        outs = [_Guarded(ctx, len(data) + nS), _Guarded(ctx, nS * 8), _Guarded(ctx, nS * 4), _Guarded(ctx, nS * 16), _Guarded(ctx, nS * 8)]
        a, b = C.c_int64(-1), C.c_int64(-1)
        rc = ctx._L.cfrk_global_unitigs_compact_device(ctx._h, *(C.c_void_p(p) for p in ins[:4]), len(data), nS, C.c_void_p(ins[4]), C.c_void_p(ins[5]),
                                                       len(links), C.c_void_p(ins[6]), C.c_void_p(outs[0].ptr), len(data) + nS, C.c_void_p(outs[1].ptr),
                                                       C.c_void_p(outs[2].ptr), C.c_void_p(outs[3].ptr), nS, C.c_void_p(outs[4].ptr), C.byref(a), C.byref(b))
        assert rc == CFRK_ERR_LAYOUT and ("unitig %d " % unitig) in ctx._L.cfrk_last_error(ctx._h).decode(), ctx._L.cfrk_last_error(ctx._h)
        assert (a.value, b.value) == (0, 0)
        ctx.sync()
        for o in outs:
            o.fetch(0)                                              # nothing was written at all
            o.free()
        for p in ins:
            ctx.free(p)
        if host:
            out = [np.zeros(len(data) + nS, np.int8), np.zeros(nS, np.int64), np.zeros(nS, np.int32), np.zeros(nS, ur.UNITIG_DTYPE)]
            rc = ctx._L.cfrk_global_unitigs_compact(ctx._h, vp(data), vp(start), vp(length), vp(rec), len(data), nS, vp(ptr), vp(links), len(links),
                                                    vp(drop), vp(out[0]), len(out[0]), vp(out[1]), vp(out[2]), vp(out[3]), nS, None, C.byref(a), C.byref(b))
            assert rc == CFRK_ERR_LAYOUT and ("unitig %d " % unitig) in ctx._L.cfrk_last_error(ctx._h).decode()

    j = nS // 2
    bad = length.copy()                                             # shorter than k
    bad[j] = k - 1
    refused(j, length=bad)
    bad = rec.copy()                                                # length != n_kmers + k - 1
    bad["n_kmers"][j] += 1
    refused(j, rec=bad, host=True)
    bad = start.copy()                                              # a range outside [0, nN)
    bad[nS - 1] = len(data) - int(length[nS - 1]) + 1
    refused(nS - 1, start=bad)
    bad = start.copy()
    bad[j] = -5
    refused(j, start=bad)
    bad = start.copy()                                              # starts that do not ascend
    bad[j] = start[j - 1] + int(length[j - 1]) - 1
    refused(j, start=bad)
    nxt = cr.merges(units, ptr, links, drop.astype(bool).tolist(), k, canonical)      # a merge whose overlap does not match
    (u, ou), (v, ov) = next((x, y) for x, y in sorted(nxt.items()) if x[0] != y[0])
    bad = data.copy()
    at = int(start[v]) + (int(length[v]) - 1 if ov else 0)          # the first base of (v,ov): in this overlap and in no other (length >= k)
    bad[at] = (bad[at] + 1) % 4
    refused(min(u, v), data=bad, host=True)
    rows = links.copy()                                             # the rows' own check still runs in front
    first = next(i for i in range(nS) if ptr[i + 1] > ptr[i])
    rows[ptr[first]]["to"] = nS
    refused(first, links=rows, host=True)


@pytest.mark.parametrize("canonical", [False, True])
def test_hostile_rows_that_pass_the_check(ctx, canonical):
    """rows that are no link set, sequences that are no unitigs: the call returns; without an error every survivor lies in
    exactly one written unitig and the sizes keep their bounds"""
    import cfrk_amd
    rng = np.random.default_rng(3131 + canonical)
    fine = refused = 0
    for i in range(99):
        k = (1, 3, 4)[i // 33]
        if i % 33 == 0:
            g = _counter(ctx, k, canonical)
        rec, ptr, rows, _ = fuzz_case(rng, canonical)
        nS = len(rec)
        length = (rec["n_kmers"] + k - 1).astype(np.int32)
        start = np.zeros(nS, np.int64)
        np.cumsum(length[:-1] + 1, out=start[1:])
        data = rng.integers(0, 4 if i % 2 else 1, int(length.sum()) + nS).astype(np.int8)     # random bases, or all A
        data[start + length] = -1
        drop = (rng.random(nS) < (0.0, 0.2, 0.6)[i % 3]).astype(np.uint8)
        try:
            if i % 2:
                got = _device(ctx, g, (data, start, length, rec), ptr, rows, drop, i % 16, (i // 2) % 16)
            else:
                got = g.compact_unitigs(data, start, length, rec, ptr, rows, drop)
        except cfrk_amd.CfrkError as e:
            assert e.code == CFRK_ERR_LAYOUT and "does not overlap" in str(e), e
            refused += 1
            continue
        fine += 1
        alive = drop == 0
        out, ostart, olength, orec, into = got
        assert len(orec) <= alive.sum() and len(out) <= int(length[alive].sum()) + int(alive.sum())
        assert int(orec["n_kmers"].sum()) == int(rec["n_kmers"][alive].sum()) and int(orec["kc"].sum()) == int(rec["kc"][alive].sum())
        assert (into["unitig"][alive] < len(orec)).all() and (into["unitig"][~alive] == NONE).all() and (into["at"][~alive] == NONE).all()
        assert (olength == orec["n_kmers"] + k - 1).all() and (out[ostart + olength] == -1).all()
        assert np.bincount(into["unitig"][alive], minlength=len(orec)).min(initial=1) >= 1
    assert fine >= 30 and refused >= 5, (fine, refused)


# ------------------------------------------------------------------ starts past 2^32

def test_starts_past_4gib(ctx):
    """the unitigs lie at both ends of a buffer of more than 2^32 bytes, of which only they are ever written or read"""
    k, canonical = 21, True
    genome = _rand_genome(81, 3000)
    units, ptr, links, drop = chain_graph(genome, [400, 900, 1500, 2200], k, canonical, 82)
    want, into, _ = cr.compact(units, ptr, links, drop, k, canonical)
    assert len(want) == 1
    data, start, length, rec = ur.layout(units)
    N = (1 << 32) + (1 << 20)
    far = start.copy()
    half = len(units) // 2
    far[half:] += N - len(data) - 64                                # the second half ends shortly before N
    assert far[half] > 1 << 32
    g = _counter(ctx, k, canonical)
    d_data = ctx.alloc(N)
    ins = [_upload(ctx, x) for x in (far, length, rec, ptr, links, drop)]
    outs = [_Guarded(ctx, len(genome) + 1, 7), _Guarded(ctx, 8), _Guarded(ctx, 4), _Guarded(ctx, 16), _Guarded(ctx, len(units) * 8)]
    try:
        for j in range(len(units)):
            ctx.h2d(d_data + int(far[j]), data[start[j]:start[j] + length[j] + 1].copy())
        assert g.compact_unitigs_device(d_data, ins[0], ins[1], ins[2], N, len(units), ins[3], ins[4], len(links), ins[5], outs[0].ptr,
                                        len(genome) + 1, outs[1].ptr, outs[2].ptr, outs[3].ptr, 1, outs[4].ptr) == (len(genome) + 1, 1)
        ctx.sync()
        got = (outs[0].fetch(len(genome) + 1, np.int8), outs[1].fetch(8, np.int64), outs[2].fetch(4, np.int32), outs[3].fetch(16, ur.UNITIG_DTYPE),
               outs[4].fetch(len(units) * 8, cr.POS_DTYPE))
        _equal(got, want, into)
    finally:
        ctx.sync()
        for o in outs:
            o.free()
        for p in ins + [d_data]:
            ctx.free(p)


# ------------------------------------------------------------------ the loops

@pytest.mark.parametrize("k,canonical,min_count", [(15, False, 1), (15, True, 1), (21, True, 2), (33, False, 1)])
def test_loops_with_recompaction(ctx, k, canonical, min_count):
    from .test_gpu_bubbles import _rows as _bubble_rows
    from .test_gpu_bulges import _rows as _bulge_rows
    table = real_graph(k, canonical, min_count)[0]
    reads = [(r, 1) for r in error_reads(*real_input(k, canonical, min_count))]
    want_units, want_report, reduced, want_rows, want_bulges = gr.simplify(table, k, canonical, min_count, rounds=3, bubble_max_diff=1, bulge_max_diff=1)
    assert len(want_report) >= 2
    runs = []
    for recompact in (False, True):
        g = _job(ctx, reads, k, canonical)
        digest = g.digest()
        got, report, rows, bulges = g.simplify(min_count, rounds=3, bubble_max_diff=1, bulges=True, bulge_max_diff=1, recompact=recompact)
        assert report == want_report and rows == _bubble_rows(want_rows) and bulges == _bulge_rows(want_bulges)    # round for round
        _same(got, ur.layout(want_units))
        assert g.mask_count() == len(table) - len(reduced) and g.digest() == digest
        runs.append((got, report, rows, bulges))
    assert all((a == b).all() for a, b in zip(runs[0][0], runs[1][0])) and runs[0][1:] == runs[1][1:]
    want_units, want_report, _ = tr.clip(table, k, canonical, min_count, None, 512, rounds=4)
    for recompact in (False, True):
        g = _job(ctx, reads, k, canonical)
        got, report = g.clip_tips(min_count, rounds=4, recompact=recompact)
        assert report == want_report
        _same(got, ur.layout(want_units))


@pytest.mark.parametrize("k,canonical,min_count", [(15, True, 1), (33, False, 1)])
def test_cli_simplify_recompact(tmp_path, k, canonical, min_count):
    from .test_gpu_query import _cli
    reads = error_reads(*real_input(k, canonical, min_count))
    fasta = tmp_path / "in.fa"
    with open(fasta, "w") as f:
        for i, r in enumerate(reads):
            f.write(">r%d\n%s\n" % (i, r))
    tail = [str(k), "--global"] + (["--canonical"] if canonical else [])
    Q = lambda name: str(tmp_path / name)
    names = ("u.fa", "g.gfa", "m.gaf", "r.tsv", "b.tsv", "p.tsv")
    outs = lambda t: ["--unitigs-out", Q(t + "u.fa"), "--unitigs-links", "--unitigs-gfa", Q(t + "g.gfa"), "--unitigs-map", str(fasta),
                      "--unitigs-map-out", Q(t + "m.gaf"), "--unitigs-min-count", str(min_count), "--tip-report", Q(t + "r.tsv")]
    read = lambda name: open(tmp_path / name, "rb").read()
    full = lambda t: ["--unitigs-clip-tips", "--unitigs-pop-bubbles", "--bubble-max-diff", "1", "--bubble-report", Q(t + "b.tsv"),
                      "--unitigs-pop-bulges", "--bulge-max-diff", "1", "--bulge-report", Q(t + "p.tsv"), "--simplify-rounds", "3"]
    subprocess.run([_cli(), str(fasta), Q("a.out")] + tail + outs("a") + full("a"), check=True, timeout=300)
    subprocess.run([_cli(), str(fasta), Q("b.out")] + tail + outs("b") + full("b") + ["--simplify-recompact"], check=True, timeout=300)
    assert read("ar.tsv").count(b"\n") >= 2                         # a second round ran: its unitigs came from the compaction
    for n in names + (".out",):
        assert read("a" + n) == read("b" + n), n
    subprocess.run([_cli(), str(fasta), Q("c.out")] + tail + outs("c") + ["--unitigs-clip-tips"], check=True, timeout=300)
    subprocess.run([_cli(), str(fasta), Q("d.out")] + tail + outs("d") + ["--unitigs-clip-tips", "--simplify-recompact"], check=True, timeout=300)
    for n in names[:4]:
        assert read("c" + n) == read("d" + n), n
    r = subprocess.run([_cli(), str(fasta), Q("e.out")] + tail + ["--unitigs-out", Q("eu.fa"), "--simplify-recompact"], capture_output=True, timeout=60)
    assert r.returncode != 0 and b"--simplify-recompact needs" in r.stderr
