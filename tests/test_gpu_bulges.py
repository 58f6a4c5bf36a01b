"""GPU: the bulge rule (cfrk_global_unitig_bulges) in its device form and its host form against tests/bulges_ref.py:
hand-made records and rows, the budget on a ladder of diamonds, real graphs of reads with errors on the reference's
unitigs and links, random rows that pass the check without being link sets, the five refusals, the capacity protocol and
the argument checks; the simplify loop round for round; the CLI.  Equality of `visits` is what shows that the search runs in the
specified order."""
import ctypes as C

import numpy as np
import pytest

from . import bulges_ref as gr
from . import tips_ref as tr
from . import unitig_links_ref as lr
from . import unitig_ref as ur
from .test_gpu_filter import _Guarded, _upload
from .test_gpu_unitig_links import _same_links
from .test_gpu_unitigs import _job, _same

pytestmark = pytest.mark.gpu

CFRK_ERR_ARG, CFRK_ERR_STATE, CFRK_ERR_LAYOUT, CFRK_ERR_SMALL_BUF = -1, -4, -5, -9
REC = np.dtype([("kc", "<u8"), ("n_kmers", "<u4"), ("flags", "<u4")])
STATS = ("arms", "popped", "undecided")


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


def _counter(ctx, canonical):
    """a job that only supplies the strand rule"""
    import cfrk_amd
    return cfrk_amd.GlobalCounter(ctx, 21, cfrk_amd.CFRK_CANONICAL if canonical else 0, 1000)


# ------------------------------------------------------------------ hand-made graphs

def rows_of(nS, edges, canonical):
    """edges (u, ou, v, ov) in the order given -> (link_ptr, links); a canonical job gets every link's mirror behind them"""
    frm, to, flags = [], [], []
    for u, ou, v, ov in edges:
        frm.append(u), to.append(v), flags.append((lr.FROM_MINUS if ou else 0) | (lr.TO_MINUS if ov else 0))
    if canonical:
        for u, ou, v, ov in edges:
            frm.append(v), to.append(u), flags.append((0 if ov else lr.FROM_MINUS) | (0 if ou else lr.TO_MINUS))
    order = np.argsort(np.array(frm, np.int64), kind="stable")
    rows = np.zeros(len(frm), lr.UNITIG_LINK_DTYPE)
    rows["to"], rows["flags"] = np.array(to, np.uint32)[order], np.array(flags, np.uint32)[order]
    ptr = np.zeros(nS + 1, np.int64)
    np.cumsum(np.bincount(np.array(frm, np.int64), minlength=nS), out=ptr[1:])
    return ptr, rows


def units_of(n, kc):
    return [("", c, m, False) for m, c in zip(n, kc)]


def records(units):
    rec = np.zeros(len(units), REC)
    rec["kc"], rec["n_kmers"], rec["flags"] = [u[1] for u in units], [u[2] for u in units], [1 if u[3] else 0 for u in units]
    return rec


P = lambda *e: [(u, 0, v, 0) for u, v in e]
# S = 0, T = 1, the arm is 2 (and 3 where there are two); the chain follows.  (max_kmers, max_diff, max_hops, max_visits,
# ratio_q8); the popped unitigs were worked out by hand.  name, edges, n, kc, canonical only, [(params, popped)]
TWO = P((0, 2), (2, 1), (0, 3), (3, 4), (4, 1))
THREE = P((0, 2), (2, 1), (0, 3), (3, 4), (4, 5), (5, 1))
HAND = [
    ("a two-hop chain beside the arm", TWO, [5, 5, 4, 2, 2], [50, 50, 4, 6, 6], False,
     [((4, 0, 4, 1024, 0), {2}), ((3, 0, 4, 1024, 0), set()), ((4, 0, 0, 1024, 0), set()), ((0, 0, 4, 1024, 0), set()),
      ((4, 0, 2, 1024, 0), {2}), ((4, 0, 1, 1024, 0), set()),                  # max_hops one short
      ((4, 0, 4, 4, 0), {2}), ((4, 0, 4, 3, 0), set())]),                      # the fourth link looked at is the one into T
    ("a three-hop chain beside the arm", THREE, [5, 5, 4, 2, 1, 1], [50, 50, 4, 6, 3, 3], False,
     [((4, 0, 4, 1024, 0), {2}), ((4, 0, 3, 1024, 0), {2}), ((4, 0, 2, 1024, 0), set())]),
    ("one interior unitig ranks below the arm: two hops", TWO, [5, 5, 4, 2, 2], [50, 50, 4, 6, 1], False, [((4, 0, 4, 1024, 0), set())]),
    ("one interior unitig ranks below the arm: three hops", THREE, [5, 5, 4, 2, 1, 1], [50, 50, 8, 6, 3, 1], False,
     [((4, 0, 4, 1024, 0), set())]),
    ("the length sum one above the window", TWO, [5, 5, 4, 2, 3], [50, 50, 4, 6, 9], False,
     [((4, 0, 4, 1024, 0), set()), ((4, 1, 4, 1024, 0), {2})]),
    ("the length sum one below the window", TWO, [5, 5, 4, 2, 1], [50, 50, 4, 6, 3], False,
     [((4, 0, 4, 1024, 0), set()), ((4, 1, 4, 1024, 0), {2})]),
    # only a walk that comes back to unitig(s), passes unitig(t) or repeats a unitig has the arm's length
    ("an interior unitig would be unitig(s)", P((0, 2), (2, 1), (0, 3), (3, 0), (0, 4), (4, 1)), [2, 5, 5, 2, 1], [20, 50, 5, 6, 3], False,
     [((5, 0, 8, 1024, 0), set())]),
    ("an interior unitig would be unitig(t)", P((0, 2), (2, 1), (0, 3), (3, 1), (1, 4), (4, 1)), [5, 2, 5, 2, 1], [50, 20, 5, 6, 3], False,
     [((5, 0, 8, 1024, 0), set())]),
    ("an interior unitig would be repeated", P((0, 2), (2, 1), (0, 3), (3, 4), (4, 3), (4, 1)), [5, 5, 6, 2, 1], [50, 50, 6, 6, 3], False,
     [((6, 0, 8, 1024, 0), set()), ((6, 3, 8, 1024, 0), {2})]),
    ("unitig(s) and unitig(t) in the other orientation", [(0, 0, 2, 0), (2, 0, 1, 0), (0, 0, 3, 0), (3, 0, 0, 1), (0, 1, 4, 0), (4, 0, 1, 0)],
     [2, 5, 5, 2, 1], [20, 50, 5, 6, 3], True, [((5, 0, 8, 1024, 0), set())]),
    ("s == t as unitigs", P((0, 2), (2, 0), (0, 3), (3, 4), (4, 0)), [5, 4, 4, 2, 2], [50, 40, 4, 6, 6], False, [((4, 0, 4, 1024, 0), {2})]),
    ("two arms whose only paths run through each other; a single-unitig bubble", P((0, 2), (2, 1), (0, 3), (3, 1)), [5, 5, 4, 4],
     [50, 50, 4, 8], False, [((4, 0, 4, 1024, 0), {2}), ((4, 0, 4, 1024, 512), {2}), ((4, 0, 4, 1024, 513), set())]),
    ("equal means: the index decides", P((0, 2), (2, 1), (0, 3), (3, 1)), [5, 5, 4, 4], [50, 50, 4, 4], False,
     [((4, 0, 4, 1024, 0), {3}), ((4, 0, 4, 1024, 256), {3}), ((4, 0, 4, 1024, 257), set())]),
    ("coverage 2 : 1", TWO, [5, 5, 4, 2, 2], [50, 50, 4, 4, 4], False,
     [((4, 0, 4, 1024, 0), {2}), ((4, 0, 4, 1024, 256), {2}), ((4, 0, 4, 1024, 512), {2}), ((4, 0, 4, 1024, 513), set())]),
    ("the path enters a unitig in - orientation", [(0, 0, 2, 0), (2, 0, 1, 0), (0, 0, 3, 0), (3, 0, 4, 1), (4, 1, 1, 0)],
     [5, 5, 4, 2, 2], [50, 50, 4, 6, 6], True, [((4, 0, 4, 1024, 0), {2})]),
    ("a circular arm is no arm", TWO, [5, 5, 4, 2, 2], [50, 50, 4, 6, 6], False, [((4, 0, 4, 1024, 0), set())]),
]


def hand_cases(canonical):
    """-> [(name, units, link_ptr, links, params, popped)]"""
    out = []
    for name, edges, n, kc, canon_only, runs in HAND:
        if canon_only and not canonical:
            continue
        units = units_of(n, kc)
        if name.startswith("a circular arm"):
            units[2] = units[2][:3] + (True,)
        ptr, rows = rows_of(len(n), edges, canonical)
        out += [(name, units, ptr, rows, params, popped) for params, popped in runs]
    return out


def ladder(d, canonical):
    """S = 0, T = 1, the arm 2 of 2 d + 2 k-mers, and d two-way diamonds S -> {a_i, b_i} -> c_i -> .. -> c_d -> T of one k-mer
    each: every one of the 2^d ways through has 2 d k-mers, two short of the window"""
    edges, prev, nxt = [(0, 2), (2, 1)], 0, 3
    for _ in range(d):
        a, b, c = nxt, nxt + 1, nxt + 2
        edges += [(prev, a), (prev, b), (a, c), (b, c)]
        prev, nxt = c, nxt + 3
    edges.append((prev, 1))
    n = [5, 5, 2 * d + 2] + [1] * (3 * d)
    kc = [50, 50, 2 * d + 2] + [3] * (3 * d)
    return (units_of(n, kc),) + rows_of(len(n), P(*edges), canonical)


def _bulges_device(ctx, g, rec, link_ptr, links, params, skew=3, visits=True, paths=True, cap=None):
    """the device form into guarded arrays: a sizes-only call, then the call with room for exactly n_path (or cap) ->
    (pop, visits, path_ptr, path, stats)"""
    import cfrk_amd
    nS = len(rec)
    ins = [_upload(ctx, rec), _upload(ctx, link_ptr), _upload(ctx, links)]
    d_pop, d_visits, d_ptr = _Guarded(ctx, nS, skew), _Guarded(ctx, nS * 4), _Guarded(ctx, (nS + 1) * 8)
    d_path = None
    call = lambda path, room: g.unitig_bulges_device(ins[0], nS, ins[1], ins[2], len(links), *params, d_pop.ptr, d_visits.ptr if visits else 0,
                                                     d_ptr.ptr if paths else 0, path, room)
    try:
        try:
            n_path, stats = call(0, 0)
        except cfrk_amd.CfrkError as e:
            if e.code != CFRK_ERR_SMALL_BUF:
                raise
            n_path, stats = e.n_path, e.stats
            assert n_path > 0 and paths
            ctx.sync()
            sized = (d_pop.fetch(nS).tobytes(), d_visits.fetch(nS * 4 if visits else 0).tobytes(), d_ptr.fetch((nS + 1) * 8).tobytes())
            room = n_path if cap is None else cap
            d_path = _Guarded(ctx, room * 4)
            assert call(d_path.ptr, room) == (n_path, stats)
            ctx.sync()
            # the sizes-only call had left everything but the paths complete
            assert sized == (d_pop.fetch(nS).tobytes(), d_visits.fetch(nS * 4 if visits else 0).tobytes(), d_ptr.fetch((nS + 1) * 8).tobytes())
        ctx.sync()
        path = d_path.fetch(n_path * 4, np.uint32) if d_path else np.zeros(0, np.uint32)
        return (d_pop.fetch(nS, np.uint8), d_visits.fetch(nS * 4 if visits else 0, np.uint32), d_ptr.fetch((nS + 1) * 8 if paths else 0, np.int64),
                path, tuple(stats[f] for f in STATS))
    finally:
        ctx.sync()
        for b, used in ((d_pop, nS), (d_visits, nS * 4 if visits else 0), (d_ptr, (nS + 1) * 8 if paths else 0)):
            b.fetch(used)                                           # whatever happened: nothing outside the arrays
            b.free()
        if d_path:
            d_path.free()
        for p in ins:
            ctx.free(p)


def _equal(got, want, what=""):
    for name, a, b in zip(("pop", "visits", "path_ptr", "path"), got, want):
        assert a.dtype == b.dtype and a.tolist() == b.tolist(), (what, name, a.tolist(), b.tolist())
    assert tuple(got[4]) == tuple(want[4]), (what, got[4], want[4])


def _both_forms(ctx, g, rec, ptr, rows, params, want, what=""):
    pop, visits, path_ptr, path, stats = g.unitig_bulges(rec, ptr, rows, *params)
    _equal((pop, visits, path_ptr, path, tuple(stats[f] for f in STATS)), want, what)
    _equal(_bulges_device(ctx, g, rec, ptr, rows, params), want, what)


@pytest.mark.parametrize("canonical", [False, True])
def test_hand_made_graphs(ctx, canonical):
    g = _counter(ctx, canonical)
    for name, units, ptr, rows, params, popped in hand_cases(canonical):
        assert len(units) <= 20
        want = gr.bulges(units, ptr, rows, canonical, *params)
        assert set(np.flatnonzero(want[0]).tolist()) == popped, (name, params)
        _both_forms(ctx, g, records(units), ptr, rows, params, want, (name, params))


@pytest.mark.parametrize("canonical", [False, True])
def test_the_budget(ctx, canonical):
    """2^d dead ends: undecided at 64 links, decided (and not popped) with the largest budget"""
    g = _counter(ctx, canonical)
    for d, max_visits, undecided in ((6, 64, True), (6, 65536, False), (3, 64, False)):
        units, ptr, rows = ladder(d, canonical)
        params = (2 * d + 2, 0, 2 * d, max_visits, 0)
        want = gr.bulges(units, ptr, rows, canonical, *params)
        assert want[0][2] == 0 and (want[1][2] == max_visits + 1) == undecided and (want[4][2] >= 1) == undecided
        assert undecided or want[1][2] > (1 << d)
        _both_forms(ctx, g, records(units), ptr, rows, params, want, (d, max_visits))
    assert gr.bulges(*ladder(6, canonical), canonical, 14, 0, 12, 64, 0)[1][2] == 65


# ------------------------------------------------------------------ real graphs: reads with errors

# (genome, coverage, read length, seed) per (k, min_count): picked by a seed search on the REFERENCE for graphs with no
# undecided arm at 1024 links and a popped arm of two or more hops; they are data.  One input serves both strand rules
# except at k = 5 with min_count 1, where errors at 1 % nearly fill the 1024 nodes and each rule has its own.
REAL = {
    (5, 1): {False: (300, 35, 60, 5), True: (350, 30, 100, 76)}, (5, 2): (300, 30, 40, 6),
    (15, 1): (1500, 40, 60, 0), (15, 2): (1500, 40, 60, 2),
    (21, 1): (900, 35, 60, 0), (21, 2): (1200, 40, 70, 0),
    (31, 1): (900, 35, 80, 0), (31, 2): (1200, 40, 90, 1),
    (33, 1): (900, 35, 90, 0), (33, 2): (900, 35, 90, 1),
    (63, 1): (1000, 40, 150, 0), (63, 2): (1500, 40, 160, 12),
}


def real_input(k, canonical, min_count):
    shape = REAL[(k, min_count)]
    return shape[canonical] if isinstance(shape, dict) else shape


def error_reads(genome, cov, length, seed, rate=0.01):
    """reads of a random genome with substitutions and one-base indels planted at `rate` per base"""
    rng = np.random.default_rng(seed)
    g = "".join(ur.BASES[i] for i in rng.integers(0, 4, genome))
    out = []
    for _ in range(genome * cov // length):
        a = int(rng.integers(0, genome - length + 1))
        r = []
        for c in g[a:a + length]:
            if rng.random() >= rate:
                r.append(c)
            elif rng.random() < 0.7:                                # a substitution
                r.append(ur.BASES[(ur.BASES.index(c) + int(rng.integers(1, 4))) % 4])
            elif rng.random() < 0.5:                                # an insertion in front of c
                r += [ur.BASES[int(rng.integers(4))], c]
        out.append("".join(r))                                      # (else: c is deleted)
    return out


_REAL = {}


def real_graph(k, canonical, min_count):
    """(table, units, link_ptr, links) of the reads of REAL, computed once"""
    key = (k, canonical, min_count)
    if key not in _REAL:
        table = {}
        ur.count_kmers(error_reads(*real_input(k, canonical, min_count)), k, canonical, 1, table)
        _REAL[key] = (table,) + tr.graph(table, k, canonical, min_count)
    return _REAL[key]


@pytest.mark.parametrize("min_count", [1, 2])
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [5, 15, 21, 31, 33, 63])
def test_real_graphs(ctx, k, canonical, min_count):
    _, units, ptr, rows = real_graph(k, canonical, min_count)
    params = (k, 1, min(k + 1, 64), 1024, 0)
    want = gr.bulges(units, ptr, rows, canonical, *params)
    assert want[4][2] == 0 and (np.diff(want[2]) >= 2).any()        # not vacuous: no undecided arm, a path of two hops or more
    g = _counter(ctx, canonical)
    _both_forms(ctx, g, records(units), ptr, rows, params, want)
    params = (k, 0, 3, 8, 300)                                       # a small budget and a ratio: undecided arms are compared too
    _both_forms(ctx, g, records(units), ptr, rows, params, gr.bulges(units, ptr, rows, canonical, *params))


# ------------------------------------------------------------------ rows that pass the check without being link sets

def fuzz_case(rng, canonical):
    nS = int(rng.integers(1, 201))
    rec = np.zeros(nS, REC)
    rec["kc"], rec["n_kmers"] = rng.integers(1, 60, nS), rng.integers(1, 5, nS)
    rec["flags"] = rng.random(nS) < 0.05
    kind = int(rng.integers(4))
    row_max = 16 if canonical else 4
    if kind == 0:                                                   # every unitig links to one target
        many = nS if canonical else min(nS, 4)
        frm, to = np.arange(many), np.full(many, int(rng.integers(nS)))
    elif kind == 1:                                                 # chains with rows that point back: j -> j + 1 -> j
        frm = np.concatenate([np.arange(nS - 1), np.arange(1, nS)])
        to = np.concatenate([np.arange(1, nS), np.arange(nS - 1)])
        if not canonical:                                           # (in-degree 2)
            keep = rng.random(len(frm)) < 0.8
            frm, to = frm[keep], to[keep]
    elif kind == 2:                                                 # random rows; not canonical: in-degree at most 4
        m = int(rng.integers(0, 3 * nS + 1))
        frm = np.sort(rng.integers(0, nS, m))
        to = rng.integers(0, nS, m) if canonical else np.concatenate([rng.permutation(nS) for _ in range(3)])[:m]
        keep = np.ones(m, bool)
        keep[row_max:] = frm[row_max:] != frm[:-row_max]
        frm, to = frm[keep], to[keep]
    else:                                                           # a backbone with arms that skip 1 .. 3 of its unitigs, some links lost
        spine = max(1, nS // 2)
        edges = [(i, i + 1) for i in range(spine - 1)]
        for a in range(spine, nS):
            i = int(rng.integers(0, spine))
            edges += [(i, a), (a, min(spine - 1, i + int(rng.integers(1, 5))))]
        rec["kc"][:spine] += 200
        ptr, rows = rows_of(nS, P(*edges), canonical)               # (with the mirrors, most of which stay)
        frm = np.repeat(np.arange(nS), np.diff(ptr))
        keep = rng.random(len(frm)) < 0.95
        keep[row_max:] &= frm[row_max:] != frm[:-row_max]
        frm, to, flags = frm[keep], rows["to"][keep], rows["flags"][keep]
        indeg = np.bincount(to, minlength=nS)
        if not canonical and indeg.max() > 4:                       # (more arms end on one unitig than 4 bases allow: drop them)
            keep = indeg[to] <= 4
            frm, to, flags = frm[keep], to[keep], flags[keep]
    if kind != 3:
        flags = rng.integers(0, 4, len(frm)) if canonical else np.zeros(len(frm), np.int64)     # no mirrors
    order = np.argsort(frm, kind="stable")
    rows = np.zeros(len(frm), lr.UNITIG_LINK_DTYPE)
    rows["to"], rows["flags"] = np.asarray(to)[order], np.asarray(flags)[order]
    ptr = np.zeros(nS + 1, np.int64)
    np.cumsum(np.bincount(np.asarray(frm, np.int64), minlength=nS), out=ptr[1:])
    params = (int(rng.integers(0, 6)), int(rng.integers(0, 4)), int(rng.choice([0, 1, 3, 8, 64])), int(rng.choice([0, 5, 64, 300])),
              int(rng.choice([0, 256, 300, 65536])))
    return rec, ptr, rows, params


@pytest.mark.parametrize("canonical", [False, True])
def test_hostile_rows_that_pass_the_check(ctx, canonical):
    g = _counter(ctx, canonical)
    rng = np.random.default_rng(31 + canonical)
    popped = undecided = 0
    for i in range(100):
        rec, ptr, rows, params = fuzz_case(rng, canonical)
        want = gr.bulges_rows(rec, ptr, rows, canonical, *params)
        popped, undecided = popped + want[4][1], undecided + want[4][2]
        if i % 2:
            got = _bulges_device(ctx, g, rec, ptr, rows, params)
        else:
            pop, visits, path_ptr, path, stats = g.unitig_bulges(rec, ptr, rows, *params)
            got = (pop, visits, path_ptr, path, tuple(stats[f] for f in STATS))
        _equal(got, want, (i, params))
        assert (got[3] < 2 * len(rec)).all()
    assert popped > 20 and undecided > 20                           # (the reference says so: the comparison is not vacuous)


@pytest.mark.parametrize("canonical", [False, True])
def test_refuses_bad_rows(ctx, canonical):
    """the five CFRK_ERR_LAYOUT reasons, with every output cleared in both forms"""
    k = 15
    _, units, link_ptr, links = real_graph(k, canonical, 1)
    g = _counter(ctx, canonical)
    rec, nS = records(units), len(units)
    j = next(i for i in range(1, nS) if link_ptr[i + 1] - link_ptr[i] >= 1)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def refused(ptr, rows, unitig):
        ins = [_upload(ctx, rec), _upload(ctx, ptr), _upload(ctx, rows)]
        outs = [_Guarded(ctx, nS), _Guarded(ctx, nS * 4), _Guarded(ctx, (nS + 1) * 8), _Guarded(ctx, 64)]
        n, stats = C.c_int64(-1), np.full(3, 7, np.int64)
        rc = ctx._L.cfrk_global_unitig_bulges_device(ctx._h, C.c_void_p(ins[0]), nS, C.c_void_p(ins[1]), C.c_void_p(ins[2]), len(rows), k, 1, 16,
                                                     1024, 0, *(C.c_void_p(o.ptr) for o in outs), 16, C.byref(n), vp(stats))
        assert rc == CFRK_ERR_LAYOUT and ("unitig %d " % unitig) in ctx._L.cfrk_last_error(ctx._h).decode()
        ctx.sync()
        assert not outs[0].fetch(nS).any() and not outs[1].fetch(nS * 4).any() and not outs[2].fetch((nS + 1) * 8).any()
        outs[3].fetch(0)
        assert n.value == 0 and not stats.any()
        for o in outs:
            o.free()
        for p in ins:
            ctx.free(p)
        pop, visits, pptr, path = np.full(nS, 7, np.uint8), np.full(nS, 7, np.uint32), np.full(nS + 1, 7, np.int64), np.full(16, 7, np.uint32)
        n, stats = C.c_int64(-1), np.full(3, 7, np.int64)
        assert ctx._L.cfrk_global_unitig_bulges(ctx._h, vp(rec), nS, vp(ptr), vp(rows), len(rows), k, 1, 16, 1024, 0, vp(pop), vp(visits),
                                                vp(pptr), vp(path), 16, C.byref(n), vp(stats)) == CFRK_ERR_LAYOUT
        assert not pop.any() and not visits.any() and not pptr.any() and (path == 7).all() and n.value == 0 and not stats.any()

    bad = link_ptr.copy()                                           # link_ptr descends
    bad[j] = link_ptr[j + 1] + 1
    row_max = 16 if canonical else 4                                # (row j - 1 now ends behind row j: it may be refused first)
    refused(bad, links, j - 1 if bad[j] > len(links) or bad[j] - link_ptr[j - 1] > row_max else j)
    bad = link_ptr.copy()                                           # ... does not begin at 0
    bad[0] = 1
    refused(bad, links, 0)
    rows = links.copy()                                             # a target that is no unitig
    rows[link_ptr[j]]["to"] = nS
    refused(link_ptr, rows, j)
    rows = links.copy()                                             # an undefined flag bit
    rows[link_ptr[j]]["flags"] |= 4
    refused(link_ptr, rows, j)
    long_row = 17 if canonical else 5                               # a row longer than an oriented end can have
    rows = np.zeros(long_row, lr.UNITIG_LINK_DTYPE)
    ptr = np.full(nS + 1, long_row, np.int64)
    ptr[0] = 0
    refused(ptr, rows, 0)
    if not canonical:                                               # more links into one unitig than 4 bases can give
        rows = np.zeros(5, lr.UNITIG_LINK_DTYPE)
        rows["to"] = nS - 1
        refused(np.array([0, 1, 2, 3, 4] + [5] * (nS - 4), np.int64), rows, nS - 1)


# ------------------------------------------------------------------ the protocol

@pytest.mark.parametrize("canonical", [False, True])
def test_capacity_protocol_and_arguments(ctx, canonical):
    import cfrk_amd
    k = 15
    _, units, link_ptr, links = real_graph(k, canonical, 1)
    g = _job(ctx, [("ACGTTGCATGCCGATAGCTAGCTAGGATCGAT", 2)], k, canonical)          # a job with counts: its digest must not move
    digest = g.digest()
    rec, nS = records(units), len(units)
    params = (k, 1, 16, 1024, 0)
    want = gr.bulges(units, link_ptr, links, canonical, *params)
    n_path = int(want[2][nS])
    assert n_path > 10
    _equal(_bulges_device(ctx, g, rec, link_ptr, links, params), want)              # sizes-only, then exact
    with pytest.raises(cfrk_amd.CfrkError) as e:                                    # one short: everything but the paths
        _bulges_device(ctx, g, rec, link_ptr, links, params, cap=n_path - 1)
    assert e.value.code == CFRK_ERR_SMALL_BUF and e.value.n_path == n_path and tuple(e.value.stats[f] for f in STATS) == want[4]
    _equal(_bulges_device(ctx, g, rec, link_ptr, links, params, cap=n_path + 5), want)     # more room than needed: the rest untouched
    got = _bulges_device(ctx, g, rec, link_ptr, links, params, skew=1, visits=False, paths=False)     # visits and path_ptr may be NULL
    assert got[0].tolist() == want[0].tolist() and got[4] == want[4] and len(got[1]) == len(got[2]) == len(got[3]) == 0
    # the host form: sizes only, one short, exact
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    L, h = ctx._L, ctx._h
    pop, visits, pptr, n, stats = np.zeros(nS, np.uint8), np.zeros(nS, np.uint32), np.zeros(nS + 1, np.int64), C.c_int64(), np.zeros(3, np.int64)
    head = (vp(rec), nS, vp(link_ptr), vp(links), len(links)) + params
    for room in (0, n_path - 1):
        pop[:], visits[:], pptr[:], stats[:] = 9, 9, 9, 9
        path = np.full(room + 1, 0xA5A5A5A5, np.uint32)
        assert L.cfrk_global_unitig_bulges(h, *head, vp(pop), vp(visits), vp(pptr), vp(path) if room else None, room, C.byref(n),
                                           vp(stats)) == CFRK_ERR_SMALL_BUF
        assert n.value == n_path and (path == 0xA5A5A5A5).all()
        _equal((pop, visits, pptr, want[3], tuple(stats.tolist())), want)
    path = np.full(n_path + 1, 0xA5A5A5A5, np.uint32)
    assert L.cfrk_global_unitig_bulges(h, *head, vp(pop), vp(visits), vp(pptr), vp(path), n_path, C.byref(n), vp(stats)) == 0
    assert path[n_path] == 0xA5A5A5A5
    _equal((pop, visits, pptr, path[:n_path], tuple(stats.tolist())), want)
    assert L.cfrk_global_unitig_bulges(h, *head, vp(pop), None, None, None, 0, None, vp(stats)) == 0 and tuple(stats.tolist()) == want[4]
    # CFRK_ERR_ARG
    path = np.zeros(n_path, np.uint32)
    ok = head + (vp(pop), vp(visits), vp(pptr), vp(path), n_path, C.byref(n), vp(stats))
    for fn in (L.cfrk_global_unitig_bulges, L.cfrk_global_unitig_bulges_device):
        for pos, value in ((0, None), (2, None), (3, None), (10, None), (13, None), (15, None), (16, None), (1, -1), (4, -1), (1, 1 << 31),
                           (7, 65), (8, 65537), (9, 65537)):
            args = list(ok)
            args[pos] = value
            assert fn(h, *args) == CFRK_ERR_ARG, (pos, value)
        st = np.full(3, 7, np.int64)
        assert fn(h, None, 0, None, None, 0, k, 0, 4, 64, 0, None, None, None, None, 0, C.byref(n), vp(st)) == 0    # nS = 0 is fine
        assert n.value == 0 and not st.any()
    for pos, value in ((7, 64), (8, 65536), (9, 65536)):                            # the bounds themselves are fine
        args = list(ok)
        args[pos] = value
        assert L.cfrk_global_unitig_bulges(h, *args) == 0, (pos, value)
    with cfrk_amd.Context(0) as c:                                                  # no job
        for fn in (c._L.cfrk_global_unitig_bulges, c._L.cfrk_global_unitig_bulges_device):
            assert fn(c._h, None, 0, None, None, 0, 1, 0, 1, 1, 0, None, None, None, None, 0, C.byref(n), vp(stats)) == CFRK_ERR_STATE
    assert g.digest() == digest


# ------------------------------------------------------------------ the loop

def _rows(rows):
    """the reference's bulge rows in the shape simplify() returns them"""
    return [(rnd, j, p, (kc, n, 1 if circ else 0), seq, spelled) for rnd, j, p, (seq, kc, n, circ), spelled in rows]


@pytest.mark.parametrize("k,canonical,min_count", [(15, False, 1), (15, True, 1), (21, True, 2), (33, False, 1)])
def test_simplify_with_bulges_round_for_round(ctx, k, canonical, min_count):
    from .test_gpu_bubbles import _rows as _bubble_rows
    table = real_graph(k, canonical, min_count)[0]
    reads = [(r, 1) for r in error_reads(*real_input(k, canonical, min_count))]
    want_units, want_report, reduced, want_rows, want_bulges = gr.simplify(table, k, canonical, min_count, rounds=3, bubble_max_diff=1,
                                                                           bulge_max_diff=1)
    assert want_report[0][3] >= 1 and len(want_report) >= 2 and want_bulges
    g = _job(ctx, reads, k, canonical)
    digest = g.digest()
    got, report, rows, bulges = g.simplify(min_count, rounds=3, bubble_max_diff=1, bulges=True, bulge_max_diff=1)
    assert report == want_report
    assert rows == _bubble_rows(want_rows) and bulges == _rows(want_bulges)
    _same(got, ur.layout(want_units))
    _same_links(g.unitig_links(got[0], got[1], got[2], min_count), lr.links(want_units, reduced, k, canonical, min_count))
    assert g.mask_count() == len(table) - len(reduced) and g.digest() == digest
    # without bulges: three values, four fields, what the bubble loop's reference says
    from . import bubbles_ref as br
    g2 = _job(ctx, reads, k, canonical)
    got, report, rows = g2.simplify(min_count, rounds=2, bubble_max_diff=1)
    want_units, want_report, _, want_rows = br.simplify(table, k, canonical, min_count, rounds=2, bubble_max_diff=1)
    assert report == want_report and rows == _bubble_rows(want_rows)
    _same(got, ur.layout(want_units))


# ------------------------------------------------------------------ CLI

@pytest.mark.parametrize("k,canonical,min_count,tips,bubbles", [(15, True, 1, True, True), (33, False, 1, False, False)])
def test_cli_pop_bulges(tmp_path, k, canonical, min_count, tips, bubbles):
    import subprocess
    from . import bubbles_ref as br
    from .test_gpu_query import _cli
    table = real_graph(k, canonical, min_count)[0]
    fasta = tmp_path / "in.fa"
    with open(fasta, "w") as f:
        for i, r in enumerate(error_reads(*real_input(k, canonical, min_count))):
            f.write(">r%d\n%s\n" % (i, r))
    units, report, reduced, rows, bulges = gr.simplify(table, k, canonical, min_count, tips, bubbles, True, rounds=3, bubble_max_diff=1,
                                                       bulge_max_diff=1)
    assert report[0][3] >= 3 and len(report) >= 2
    link_ptr, links = lr.links(units, reduced, k, canonical, min_count)
    tail = [str(k), "--global"] + (["--canonical"] if canonical else [])
    Q = lambda name: str(tmp_path / name)
    outs = lambda t: ["--unitigs-out", Q(t + ".fa"), "--unitigs-links", "--unitigs-gfa", Q(t + ".gfa"), "--unitigs-min-count", str(min_count)]
    both = (["--unitigs-clip-tips"] if tips else []) + (["--unitigs-pop-bubbles", "--bubble-max-diff", "1", "--bubble-report", Q("b.tsv")] if bubbles else [])
    opts = ["--unitigs-pop-bulges", "--bulge-max-diff", "1", "--simplify-rounds", "3", "--tip-report", Q("r.tsv"), "--bulge-report", Q("g.tsv")]
    subprocess.run([_cli(), str(fasta), Q("a.out")] + tail + outs("pop") + both + opts, check=True, timeout=300)
    read = lambda name: open(tmp_path / name, "rb").read()
    assert read("pop.fa") == lr.fasta_text_links(units, link_ptr, links)
    assert read("pop.gfa") == lr.gfa_text(units, k, link_ptr, links)
    assert read("r.tsv") == gr.report_text(report)
    assert read("g.tsv") == gr.bulge_lines(bulges, k) and read("g.tsv").count(b"\n") == sum(r[3] for r in report)
    if bubbles:
        assert read("b.tsv") == br.bubble_lines(rows)
    # the other options: one round, longer arms, a ratio, six hops, a budget; no report files
    more = ["--unitigs-pop-bulges", "--bulge-max-kmers", str(k + 2), "--bulge-ratio", "1.5", "--bulge-max-hops", "6", "--bulge-max-visits", "64",
            "--simplify-rounds", "1"]
    subprocess.run([_cli(), str(fasta), Q("c.out")] + tail + ["--unitigs-out", Q("c.fa"), "--unitigs-min-count", str(min_count)] + more,
                   check=True, timeout=300)
    units2, report2 = gr.simplify(table, k, canonical, min_count, False, False, True, rounds=1, bulge_max_kmers=k + 2, bulge_max_hops=6,
                                  bulge_max_visits=64, bulge_ratio_q8=384)[:2]
    assert 1 <= report2[0][3] < gr.simplify(table, k, canonical, min_count, False, False, True, rounds=1, bulge_max_kmers=k + 2)[1][0][3]
    assert read("c.fa") == ur.fasta_text(units2)
    assert read("a.out") == read("c.out")                           # the counts' own output does not see the options
    # without the new options: the bubble loop's texts, five fields, as before
    old = ["--unitigs-pop-bubbles", "--bubble-max-diff", "1", "--simplify-rounds", "3", "--tip-report", Q("r5.tsv"), "--bubble-report", Q("b5.tsv")]
    subprocess.run([_cli(), str(fasta), Q("d.out")] + tail + outs("old") + old + (["--unitigs-clip-tips"] if tips else []), check=True, timeout=300)
    ounits, oreport, oreduced, orows = br.simplify(table, k, canonical, min_count, tips, True, 3, None, 512, None, 1, 0)
    optr, olinks = lr.links(ounits, oreduced, k, canonical, min_count)
    assert read("old.fa") == lr.fasta_text_links(ounits, optr, olinks) and read("old.gfa") == lr.gfa_text(ounits, k, optr, olinks)
    assert read("r5.tsv") == br.report_text(oreport) and read("b5.tsv") == br.bubble_lines(orows)
    assert read("d.out") == read("a.out")
