"""GPU: the weak rule (cfrk_global_unitig_weak) in its device form and its host form against tests/weak_ref.py: planted
jobs on a k grid under both strand rules; crafted records and rows at the block seams, at the bound of 16 x 16 links, at
in-degree 4, at the 128-bit edge and on ties; rows it must refuse and hostile rows that pass the check; the simplify
loop with the rule round for round, with and without compaction; simplify() and the CLI without it as they were; the
CLI with it."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from . import bubbles_ref as br
from . import tips_ref as tr
from . import unitig_links_ref as lr
from . import unitig_ref as ur
from . import weak_ref as wr
from .test_gpu_bubbles import _csr, _rows
from .test_gpu_filter import _Guarded, _upload
from .test_gpu_query import _cli
from .test_gpu_unitig_links import _same_links
from .test_gpu_unitigs import _job, _same, _table
from .weak_cases import KS, PARAMS, ref, weak_input

pytestmark = pytest.mark.gpu

CFRK_ERR_ARG, CFRK_ERR_STATE, CFRK_ERR_LAYOUT = -1, -4, -5
FM, TM = lr.FROM_MINUS, lr.TO_MINUS


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


_WANT = {}


def _want(k, canonical, params):
    key = (k, canonical, params)
    if key not in _WANT:
        _, units, link_ptr, links = ref(k, canonical)
        _WANT[key] = wr.weak(units, link_ptr, links, canonical, *params)
    return _WANT[key]


def _weak_device(ctx, g, rec, link_ptr, links, params, skew=3):
    """the device form into a guarded array `skew` bytes off its boundary -> (weak, stats)"""
    nS = len(rec)
    ins = [_upload(ctx, rec), _upload(ctx, link_ptr), _upload(ctx, links)]
    d_weak = _Guarded(ctx, nS, skew)
    try:
        stats = g.unitig_weak_device(ins[0], nS, ins[1], ins[2], len(links), *params, d_weak.ptr)
        ctx.sync()
        return d_weak.fetch(nS, np.uint8), stats
    finally:
        ctx.sync()
        d_weak.fetch(nS)                                            # whatever happened: nothing outside the array
        d_weak.free()
        for p in ins:
            ctx.free(p)


def _both_forms(ctx, g, rec, link_ptr, links, params, want, skew=3):
    want_weak, want_stats = want
    weak, stats = g.unitig_weak(rec, link_ptr, links, *params)
    assert weak.dtype == np.uint8 and weak.tolist() == want_weak.tolist() and stats == want_stats, params
    weak, stats = _weak_device(ctx, g, rec, link_ptr, links, params, skew)
    assert weak.tolist() == want_weak.tolist() and stats == want_stats, params


def _counter(ctx, canonical):
    """a job that supplies the strand rule and nothing else: the rule reads records and rows"""
    import cfrk_amd
    return cfrk_amd.GlobalCounter(ctx, 21, cfrk_amd.CFRK_CANONICAL if canonical else 0, 1000)


# ------------------------------------------------------------------ the rule on the grid

@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", KS)
def test_unitig_weak(ctx, k, canonical):
    table, units, link_ptr, links = ref(k, canonical)
    g = _job(ctx, weak_input(k), k, canonical)
    digest, histo = g.digest(), g.histogram(16)
    data, start, length, rec = g.unitigs(1)
    _same((data, start, length, rec), ur.layout(units))
    _same_links(g.unitig_links(data, start, length), (link_ptr, links))
    for params in PARAMS(k):
        _both_forms(ctx, g, rec, link_ptr, links, params, _want(k, canonical, params))
    _both_forms(ctx, g, rec, link_ptr, links, PARAMS(k)[4], _want(k, canonical, PARAMS(k)[4]), skew=1)
    assert g.digest() == digest and (g.histogram(16) == histo).all()


# ------------------------------------------------------------------ crafted records and rows, no k-mers

def _random_rows(rng, nS, canonical):
    """rows that pass the check: at most 4 links a row and 4 links into a unitig where there is one strand; in a canonical
    job at most 16 a row, random strand flags, no mirrors"""
    m = 2 * nS if not canonical else 6 * nS
    frm = np.sort(rng.integers(0, nS, m))
    to = rng.integers(0, nS, m)
    row_max = 16 if canonical else 4
    keep = np.ones(m, bool)
    keep[row_max:] = frm[row_max:] != frm[:-row_max]
    if not canonical:                                               # in-degree 4 at most
        seen = {}
        for i in np.flatnonzero(keep):
            seen[int(to[i])] = seen.get(int(to[i]), 0) + 1
            keep[i] = seen[int(to[i])] <= 4
    flags = rng.integers(0, 4, m).astype(np.uint32) if canonical else np.zeros(m, np.uint32)
    return _csr(nS, frm[keep], to[keep], flags[keep])


def _random_rec(rng, nS):
    import cfrk_amd
    rec = np.zeros(nS, cfrk_amd.UNITIG_DTYPE)
    rec["n_kmers"] = rng.integers(1, 6, nS)
    rec["kc"] = rec["n_kmers"] * rng.integers(1, 4, nS) + rng.integers(0, 2, nS)      # few distinct means: ties are common
    rec["flags"] = rng.integers(0, 8, nS) == 0
    return rec


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("nS", [1, 255, 256, 257, 513])
def test_block_seams(ctx, nS, canonical):
    """one lane per unitig in blocks of 256 and waves of 64: every byte and all three counts at the seams, unitigs without
    a link among them"""
    g = _counter(ctx, canonical)
    rng = np.random.default_rng(400 + 2 * nS + canonical)
    rec = _random_rec(rng, nS)
    cases = [_random_rows(rng, nS, canonical), (np.zeros(nS + 1, np.int64), np.zeros(0, lr.UNITIG_LINK_DTYPE))]
    if nS == 1:                                                     # the one unitig linked to itself
        cases.append(_csr(1, [0], [0], np.zeros(1, np.uint32)))
    found = set()
    for ptr, rows in cases:
        for params in ((5, 0, 5, 1024), (3, 512, 2, 512), (5, 256, 0, 0)):
            want = wr.weak_rows(rec, ptr, rows, canonical, *params)
            _both_forms(ctx, g, rec, ptr, rows, params, want)
            found |= set(want[0].tolist())
    assert found == {0, 1, 2} or nS == 1


def test_a_row_of_16_links_whose_targets_have_rows_of_16(ctx):
    """the bound of the header: unitig 0 leaves (0,+) and (0,-) by 8 links each, to 16 targets; every target has 8 links on
    the entering side, 7 siblings that do not beat unitig 0 and, last in the row, one that does; 8 links on its other
    side pad the row.  Only after all 128 comparisons is unitig 0 a connection; with one of the 16 strong siblings
    weakened it is none.  Then the same with all 16 links of every target's row on the entering side (no real link set,
    but it passes the check): 256 comparisons"""
    import cfrk_amd
    g = _counter(ctx, True)
    for entering in (8, 16):
        nS = 17 + 16 * 16
        rec = np.zeros(nS, cfrk_amd.UNITIG_DTYPE)
        rec["n_kmers"], rec["kc"] = 2, 2                            # the fill: mean 1, below unitig 0's
        rec["n_kmers"][0], rec["kc"][0] = 3, 6                      # mean 2
        frm, to, fl = [], [], []
        for i in range(16):
            v = 1 + i
            minus = i >= 8                                          # (0,+) -> (v,+) for the first 8, (0,-) -> (v,+) for the others
            frm.append(0), to.append(v), fl.append(FM if minus else 0)
            # in(v,+) is read off the links that leave (v,-): the siblings, the strong one last; unitig 0 among them
            sib = [17 + 16 * i + s for s in range(16)]
            for s in range(entering - 1):
                frm.append(v), to.append(sib[s]), fl.append(FM)
            frm.append(v), to.append(0), fl.append(FM | (0 if minus else TM))
            for s in range(entering, 16):
                frm.append(v), to.append(sib[s]), fl.append(0)
            strong = sib[entering - 2]
            rec["n_kmers"][strong], rec["kc"][strong] = 1, 8        # mean 8: four times unitig 0's
        ptr, rows = _csr(nS, np.array(frm), np.array(to), np.array(fl, np.uint32))
        assert (np.diff(ptr)[:17] == 16).all() and len(rows) == 16 * 17
        params = (3, 1024, 0, 0)
        want = wr.weak_rows(rec, ptr, rows, True, *params)
        assert want[0][0] == 1 and want[1]["connections"] == 1
        _both_forms(ctx, g, rec, ptr, rows, params, want)
        weaker = rec.copy()
        weaker["kc"][17 + 16 * 15 + entering - 2] = 7               # the last target's strong sibling: not four times any more
        want = wr.weak_rows(weaker, ptr, rows, True, *params)
        assert want[0][0] == 0 and want[1]["connections"] == 0 and want[1]["candidates"] >= 1
        _both_forms(ctx, g, weaker, ptr, rows, params, want)


def test_in_degree_4_where_there_is_one_strand(ctx):
    """b1 is entered by four unitigs, x among them, and a0 left by four: the in-rows at their bound.  x goes when a sibling
    at each end beats it, whichever place in the in-row it has"""
    import cfrk_amd
    g = _counter(ctx, False)
    # a0 = 0 -> {1, 2, 3, x = 9};  {4, 5, 6, x} -> b1 = 7;  8 is not linked
    frm, to = [0, 0, 0, 0, 4, 5, 6, 9], [1, 2, 3, 9, 7, 7, 7, 7]
    ptr, rows = _csr(10, frm, to, np.zeros(8, np.uint32))
    rec = np.zeros(10, cfrk_amd.UNITIG_DTYPE)
    rec["n_kmers"], rec["kc"] = 4, 4
    rec["n_kmers"][9], rec["kc"][9] = 2, 4                          # x: mean 2, everything else mean 1
    for strong_out, strong_in, weak9 in ((None, None, 0), (3, None, 0), (None, 6, 0), (1, 4, 1), (3, 6, 1), (2, 5, 1)):
        r = rec.copy()
        for s in (strong_out, strong_in):
            if s is not None:
                r["kc"][s] = 16                                     # mean 4
        want = wr.weak_rows(r, ptr, rows, False, 4, 512, 4, 512)
        assert want[0].tolist() == [0] * 8 + [2, weak9]             # (8 floats free at mean 1; the others have dead ends)
        _both_forms(ctx, g, r, ptr, rows, (4, 512, 4, 512), want)


@pytest.mark.parametrize("canonical", [False, True])
def test_products_at_the_128_bit_edge(ctx, canonical):
    """kc = 2^63, n_kmers = 2^32 - 1, ratio_q8 = 65536: 256 kc_w n_j = 2^71 (2^32 - 1) against ratio_q8 kc_j n_w = 2^16 2^55
    (2^32 - 1), equal, which 64 bits cannot tell from the sibling with one count fewer"""
    import cfrk_amd
    g = _counter(ctx, canonical)
    N = (1 << 32) - 1
    # two bridges x = 4 and y = 5 between a0 = 0 and b1 = 3; a1 = 1 and b0 = 2 are the siblings
    frm, to = [0, 2, 0, 4, 0, 5], [1, 3, 4, 3, 5, 3]
    fl = np.zeros(6, np.uint32)
    if canonical:
        frm, to, fl = frm + to, to + frm, np.concatenate([fl, np.full(6, FM | TM, np.uint32)])
    ptr, rows = _csr(6, frm, to, fl)
    rec = np.zeros(6, cfrk_amd.UNITIG_DTYPE)
    rec["n_kmers"] = N
    rec["kc"] = [1 << 63, 1 << 63, 1 << 63, 1 << 63, 1 << 55, (1 << 55) + 1]
    want = wr.weak_rows(rec, ptr, rows, canonical, N, 65536, 0, 0)
    assert want[0].tolist() == [0, 0, 0, 0, 1, 0] and want[1]["candidates"] == 2
    _both_forms(ctx, g, rec, ptr, rows, (N, 65536, 0, 0), want)
    rec["kc"][2] = (1 << 63) - 1                                    # b0 one count short: x stays too
    want = wr.weak_rows(rec, ptr, rows, canonical, N, 65536, 0, 0)
    assert not want[0].any()
    _both_forms(ctx, g, rec, ptr, rows, (N, 65536, 0, 0), want)
    # the isolated test at its edge: 256 kc = 2^71 against iso_mean_q8 n < 2^64; kc = 2^64 - 1; and the largest mean that goes
    rec = np.zeros(4, cfrk_amd.UNITIG_DTYPE)
    rec["n_kmers"] = [N, N, N, 1]
    rec["kc"] = [1 << 63, (1 << 64) - 1, ((N * N) >> 8), (1 << 24) - 1]
    ptr, rows = np.zeros(5, np.int64), np.zeros(0, lr.UNITIG_LINK_DTYPE)
    want = wr.weak_rows(rec, ptr, rows, canonical, 0, 0, N, N)
    assert want[0].tolist() == [0, 0, 2, 2]
    _both_forms(ctx, g, rec, ptr, rows, (0, 0, N, N), want)


@pytest.mark.parametrize("canonical", [False, True])
def test_equal_means_are_decided_by_index(ctx, canonical):
    """a chain of 2000 bubbles src_i -> {a_i, b_i} -> src_i+1 with equal means on both arms: the arm with the higher index
    goes, at every ratio up to 256, none at 257; in the canonical variant every other b_i is stored reversed"""
    import cfrk_amd
    N = 2000
    nS = 3 * N + 1
    i = np.arange(N, dtype=np.int64)
    src, nxt = 3 * i, 3 * i + 3
    lowfirst = i % 3 != 0                                           # a third of the sites: the arm with the lower index is b
    a, b = np.where(lowfirst, 3 * i + 1, 3 * i + 2), np.where(lowfirst, 3 * i + 2, 3 * i + 1)
    rec = np.zeros(nS, cfrk_amd.UNITIG_DTYPE)
    rec["n_kmers"], rec["kc"] = 5, 50
    rec["n_kmers"][a], rec["kc"][a] = 3, 6
    rec["n_kmers"][b], rec["kc"][b] = 2, 4                          # 6 / 3 = 4 / 2
    rev = (i % 2 == 1) if canonical else np.zeros(N, bool)
    rb = rev.astype(np.uint32)
    frm, to = [src, a, src, b], [a, nxt, b, nxt]
    flags = [np.zeros(N, np.uint32), np.zeros(N, np.uint32), rb * TM, rb * FM]
    if canonical:
        frm, to = frm + [a, nxt, b, nxt], to + [src, a, src, b]
        flags += [np.full(N, FM | TM, np.uint32), np.full(N, FM | TM, np.uint32), (1 - rb) * FM + TM, FM + (1 - rb) * TM]
    ptr, rows = _csr(nS, np.concatenate(frm), np.concatenate(to), np.concatenate(flags).astype(np.uint32))
    g = _counter(ctx, canonical)
    for ratio_q8, gone in ((0, True), (256, True), (257, False)):
        want = wr.weak_rows(rec, ptr, rows, canonical, 3, ratio_q8, 0, 0)
        expect = np.zeros(nS, np.uint8)
        if gone:
            expect[np.maximum(a, b)] = 1
        assert want[0].tolist() == expect.tolist() and want[1]["candidates"] == 2 * N
        _both_forms(ctx, g, rec, ptr, rows, (3, ratio_q8, 0, 0), want)


# ------------------------------------------------------------------ untrusted rows

@pytest.mark.parametrize("canonical", [False, True])
def test_unitig_weak_refuses_bad_rows(ctx, canonical):
    import cfrk_amd
    k = 21
    table, units, link_ptr, links = ref(k, canonical)
    g = _job(ctx, weak_input(k), k, canonical)
    rec = ur.layout(units)[3]
    nS = len(units)
    j = next(i for i in range(nS) if link_ptr[i + 1] - link_ptr[i] >= 1 and i > 0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    stats_t = C.c_int64 * 3

    def refused(ptr, rows, unitig):
        with pytest.raises(cfrk_amd.CfrkError) as e:
            _weak_device(ctx, g, rec, ptr, rows, (k, 0, 2 * k, 512))
        assert e.value.code == CFRK_ERR_LAYOUT and ("unitig %d " % unitig) in str(e.value)
        # every byte is written whatever is refused, and the stats are 0: the device array ...
        ins = [_upload(ctx, rec), _upload(ctx, ptr), _upload(ctx, rows)]
        d_weak = _Guarded(ctx, nS)
        st = stats_t(-1, -1, -1)
        assert ctx._L.cfrk_global_unitig_weak_device(ctx._h, C.c_void_p(ins[0]), nS, C.c_void_p(ins[1]), C.c_void_p(ins[2]), len(rows),
                                                     k, 0, 2 * k, 512, C.c_void_p(d_weak.ptr), st) == CFRK_ERR_LAYOUT
        ctx.sync()
        assert not d_weak.fetch(nS).any() and list(st) == [0, 0, 0]
        d_weak.free()
        for p in ins:
            ctx.free(p)
        # ... and the host array
        weak, st = np.full(nS, 7, np.uint8), stats_t(-1, -1, -1)
        assert ctx._L.cfrk_global_unitig_weak(ctx._h, vp(rec), nS, vp(ptr), vp(rows), len(rows), k, 0, 2 * k, 512, vp(weak), st) == CFRK_ERR_LAYOUT
        assert not weak.any() and list(st) == [0, 0, 0]

    bad = link_ptr.copy()                                           # link_ptr descends
    bad[j] = link_ptr[j + 1] + 1
    row_max = 16 if canonical else 4                                # (row j - 1 now ends behind row j: it may be refused first)
    refused(bad, links, j - 1 if bad[j] > len(links) or bad[j] - link_ptr[j - 1] > row_max else j)
    bad = link_ptr.copy()                                           # ... does not begin at 0, does not end at n_links
    bad[0] = 1
    refused(bad, links, 0)
    bad = link_ptr.copy()
    bad[nS] -= 1
    refused(bad, links, nS - 1)
    long_row = 17 if canonical else 5                               # a row longer than an oriented end can have
    rows = np.zeros(long_row, lr.UNITIG_LINK_DTYPE)
    ptr = np.full(nS + 1, long_row, np.int64)
    ptr[0] = 0
    refused(ptr, rows, 0)
    rows = links.copy()                                             # a target that is no unitig
    rows[link_ptr[j]]["to"] = nS
    refused(link_ptr, rows, j)
    rows = links.copy()                                             # an undefined flag bit
    rows[link_ptr[j]]["flags"] |= 4
    refused(link_ptr, rows, j)
    if not canonical:                                               # a strand flag where there is one strand
        rows = links.copy()
        rows[link_ptr[j]]["flags"] = 1
        refused(link_ptr, rows, j)
        rows = np.zeros(5, lr.UNITIG_LINK_DTYPE)                    # more links into one unitig than 4 bases can give
        rows["to"] = nS - 1
        ptr = np.array([0, 1, 2, 3, 4] + [5] * (nS - 4), np.int64)
        refused(ptr, rows, nS - 1)
    # CFRK_ERR_ARG
    L, h = ctx._L, ctx._h
    weak, st = np.zeros(nS, np.uint8), stats_t()
    ok = (vp(rec), nS, vp(link_ptr), vp(links), len(links), k, 0, 0, 0, vp(weak), st)
    for fn in (L.cfrk_global_unitig_weak, L.cfrk_global_unitig_weak_device):
        for pos, value in ((0, None), (2, None), (3, None), (9, None), (10, None), (1, -1), (4, -1), (1, 1 << 32), (6, 65537)):
            args = list(ok)
            args[pos] = value
            assert fn(h, *args) == CFRK_ERR_ARG, (pos, value)
        st = stats_t(-1, -1, -1)
        assert fn(h, None, 0, None, None, 0, k, 0, 0, 0, None, st) == 0 and list(st) == [0, 0, 0]      # nS = 0: nothing found
    st = stats_t()
    assert L.cfrk_global_unitig_weak(h, *ok[:6], 65536, *ok[7:10], st) == 0                            # the bound itself is fine
    assert L.cfrk_global_unitig_weak(h, *ok[:10], st) == 0 and st[0] == _want(k, canonical, (k, 0, 0, 0))[1]["connections"]
    with cfrk_amd.Context(0) as c:                                                                     # no job
        assert c._L.cfrk_global_unitig_weak(c._h, None, 0, None, None, 0, 1, 0, 0, 0, None, st) == CFRK_ERR_STATE
        assert c._L.cfrk_global_unitig_weak_device(c._h, None, 0, None, None, 0, 1, 0, 0, 0, None, st) == CFRK_ERR_STATE


@pytest.mark.parametrize("canonical", [False, True])
def test_hostile_rows_that_pass_the_check(ctx, canonical):
    """rows that are no real link set but pass the check: CFRK_OK, every byte written, and what the rule says of the rows
    as given, in() of a canonical job read off the rows by the mirror convention"""
    import cfrk_amd
    g = _counter(ctx, canonical)
    nS = 700
    rng = np.random.default_rng(177 + canonical)
    rec = np.zeros(nS, cfrk_amd.UNITIG_DTYPE)
    rec["kc"], rec["n_kmers"] = rng.integers(1, 1000, nS), rng.integers(1, 4, nS)
    rec["n_kmers"][::50] = 0                                        # records no unitig has
    cases = []
    # 0 -> 1 -> 0 -> ..., a two-cycle 2 <-> 3, a chain behind them
    frm, to = [0, 1, 2, 3] + list(range(4, nS - 1)), [1, 0, 3, 2] + list(range(5, nS))
    cases.append(_csr(nS, frm, to, np.zeros(len(frm), np.uint32)))
    # all targets equal: every unitig links to unitig 5 once (in-degree 4 at most where there is one strand)
    many = nS if canonical else 4
    cases.append(_csr(nS, np.arange(many), np.full(many, 5), np.zeros(many, np.uint32)))
    # the same link several times in one row
    cases.append(_csr(nS, [0, 0, 1, 1, 2, 2], [1, 1, 2, 2, 1, 1], np.zeros(6, np.uint32)))
    for seed in range(3):
        cases.append(_random_rows(np.random.default_rng(1000 + 10 * seed + canonical), nS, canonical))
    found = 0
    for ptr, rows in cases:
        for params in ((3, 0, 3, 1 << 20), (3, 512, 0, 0), (0, 0, 0, 0)):
            want = wr.weak_rows(rec, ptr, rows, canonical, *params)
            _both_forms(ctx, g, rec, ptr, rows, params, want)
            found += want[1]["connections"]
    assert found > 0


# ------------------------------------------------------------------ the loop

def _weak_rows_of(rows):
    """the reference's weak rows in the shape simplify() returns them"""
    return [(rnd, j, kind, (kc, n, 1 if circ else 0), seq) for rnd, j, kind, (seq, kc, n, circ) in rows]


_LOOP = {}


def _loop(k, canonical, mode):
    """the reference loop, once per point: (units, report, reduced, rows, bulge rows, weak rows)"""
    key = (k, canonical, mode)
    if key not in _LOOP:
        table = ref(k, canonical)[0]
        others = mode == "all"
        _LOOP[key] = wr.simplify(table, k, canonical, 1, others, others, False, True, rounds=8, bubble_max_diff=1)
    return _LOOP[key]


@pytest.mark.parametrize("recompact", [False, True])
@pytest.mark.parametrize("mode", ["weak", "all"])
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [12, 21, 33])
def test_simplify_with_weak_round_for_round(ctx, k, canonical, mode, recompact):
    table = ref(k, canonical)[0]
    others = mode == "all"
    want_units, want_report, reduced, want_rows, _, want_weak = _loop(k, canonical, mode)
    assert want_report[-1][1:4] == (0, 0, 0) and want_report[-1][5:] == (0, 0) and len(want_report) >= 2
    assert sum(r[5] for r in want_report) >= 2 and sum(r[6] for r in want_report) >= 1
    g = _job(ctx, weak_input(k), k, canonical)
    digest, histo = g.digest(), g.histogram(16)
    got, report, rows, weak_rows = g.simplify(1, others, others, rounds=8, bubble_max_diff=1, weak=True, recompact=recompact)
    assert report == wr.report_rows(want_report, True, False, True)
    assert rows == _rows(want_rows) and weak_rows == _weak_rows_of(want_weak)
    _same(got, ur.layout(want_units))
    _same_links(g.unitig_links(got[0], got[1], got[2]), lr.links(want_units, reduced, k, canonical, 1))
    assert g.mask_count() == len(table) - len(reduced)
    assert g.digest() == digest and (g.histogram(16) == histo).all()


@pytest.mark.parametrize("canonical", [False, True])
def test_simplify_other_parameters_and_bulges(ctx, canonical):
    """one round at other thresholds, and all four rules in one loop"""
    k = 21
    table = ref(k, canonical)[0]
    g = _job(ctx, weak_input(k), k, canonical)
    got, report, rows, weak_rows = g.simplify(1, False, False, rounds=1, weak=True, weak_max_kmers=k - 2, weak_ratio=2.0, weak_iso_max_kmers=4,
                                              weak_iso_mean=1.5)
    want = wr.simplify(table, k, canonical, 1, False, False, False, True, 1, weak_max_kmers=k - 2, weak_ratio_q8=512, weak_iso_max_kmers=4,
                       weak_iso_mean_q8=384)
    assert report == wr.report_rows(want[1], True, False, True) and rows == [] and weak_rows == _weak_rows_of(want[5])
    _same(got, ur.layout(want[0]))
    g = _job(ctx, weak_input(k), k, canonical)
    got, report, rows, bulge_rows, weak_rows = g.simplify(1, True, True, rounds=8, bubble_max_diff=1, bulges=True, bulge_max_diff=1, weak=True)
    want = wr.simplify(table, k, canonical, 1, True, True, True, True, 8, bubble_max_diff=1, bulge_max_diff=1)
    assert report == wr.report_rows(want[1], True, True, True) and rows == _rows(want[3]) and weak_rows == _weak_rows_of(want[5])
    assert [(r, j, p) for r, j, p, _, _, _ in bulge_rows] == [(r, j, p) for r, j, p, _, _ in want[4]]
    _same(got, ur.layout(want[0]))


@pytest.mark.parametrize("canonical", [False, True])
def test_simplify_without_weak_is_what_it_was(ctx, canonical):
    k = 21
    table = ref(k, canonical)[0]
    want_units, want_report, reduced, want_rows = br.simplify(table, k, canonical, 1, True, True, rounds=8, bubble_max_diff=1)
    for kw in ({}, {"weak": False, "weak_ratio": 0.0, "weak_iso_mean": 100.0}):
        g = _job(ctx, weak_input(k), k, canonical)
        out = g.simplify(1, True, True, rounds=8, bubble_max_diff=1, **kw)
        assert len(out) == 3
        got, report, rows = out
        assert report == want_report and rows == _rows(want_rows)
        _same(got, ur.layout(want_units))
        assert g.mask_count() == len(table) - len(reduced)


# ------------------------------------------------------------------ CLI

def _fasta(path, seqs):
    with open(path, "w") as f:
        i = 0
        for s, t in seqs:
            for _ in range(t):
                f.write(">r%d\n%s\n" % (i, s))
                i += 1


@pytest.mark.parametrize("k,canonical,mode", [(12, False, "weak"), (21, True, "all"), (31, True, "weak"), (33, False, "tips")])
def test_cli_drop_weak(tmp_path, k, canonical, mode):
    seqs = weak_input(k)
    fasta = tmp_path / "in.fa"
    _fasta(fasta, seqs)
    table = _table(seqs, k, canonical)
    tips, bubbles = mode != "weak", mode == "all"
    units, report, reduced, rows, _, weak_rows = wr.simplify(table, k, canonical, 1, tips, bubbles, False, True, 4, bubble_max_diff=1)
    assert sum(r[5] for r in report) >= 2 and sum(r[6] for r in report) >= 1
    link_ptr, links = lr.links(units, reduced, k, canonical, 1)
    tail = [str(k), "--global"] + (["--canonical"] if canonical else [])
    P = lambda name: str(tmp_path / name)
    outs = lambda t: ["--unitigs-out", P(t + ".fa"), "--unitigs-links", "--unitigs-gfa", P(t + ".gfa")]
    opts = ["--unitigs-drop-weak", "--tip-report", P("r.tsv"), "--weak-report", P("w.tsv")]
    opts += (["--unitigs-clip-tips"] if tips else []) + (["--unitigs-pop-bubbles", "--bubble-max-diff", "1"] if bubbles else [])
    subprocess.run([_cli(), str(fasta), P("a.out")] + tail + outs("weak") + opts, check=True, timeout=300)
    read = lambda name: open(tmp_path / name, "rb").read()
    assert read("weak.fa") == lr.fasta_text_links(units, link_ptr, links)
    assert read("weak.gfa") == lr.gfa_text(units, k, link_ptr, links)
    assert read("r.tsv") == wr.report_text(report, bubbles, False, True)
    assert read("w.tsv") == wr.weak_lines(weak_rows) and read("w.tsv").count(b"\n") == sum(r[5] + r[6] for r in report)
    # the same with compaction between the rounds
    subprocess.run([_cli(), str(fasta), P("b.out")] + tail + outs("re") + opts[:1] + opts[5:] + ["--simplify-recompact", "--weak-report", P("w2.tsv")],
                   check=True, timeout=300)
    assert read("re.fa") == read("weak.fa") and read("re.gfa") == read("weak.gfa") and read("w2.tsv") == read("w.tsv")
    # the other options: one round, the other thresholds; no report files
    more = ["--unitigs-drop-weak", "--weak-max-kmers", str(k - 2), "--weak-ratio", "2", "--weak-iso-max-kmers", "4", "--weak-iso-mean", "1.5",
            "--simplify-rounds", "1"]
    subprocess.run([_cli(), str(fasta), P("c.out")] + tail + ["--unitigs-out", P("c.fa")] + more, check=True, timeout=300)
    units2 = wr.simplify(table, k, canonical, 1, False, False, False, True, 1, weak_max_kmers=k - 2, weak_ratio_q8=512, weak_iso_max_kmers=4,
                         weak_iso_mean_q8=384)[0]
    assert read("c.fa") == ur.fasta_text(units2)
    assert read("a.out") == read("b.out") == read("c.out")          # the counts' own output does not see the options


@pytest.mark.parametrize("k,canonical", [(21, True), (33, False)])
def test_cli_without_the_option_is_what_it_was(tmp_path, k, canonical):
    seqs = weak_input(k)
    fasta = tmp_path / "in.fa"
    _fasta(fasta, seqs)
    table = _table(seqs, k, canonical)
    tail = [str(k), "--global"] + (["--canonical"] if canonical else [])
    P = lambda name: str(tmp_path / name)
    outs = lambda t: ["--unitigs-out", P(t + ".fa"), "--unitigs-links", "--unitigs-gfa", P(t + ".gfa")]
    read = lambda name: open(tmp_path / name, "rb").read()
    # tips and bubbles: the five-field report and the bubble report of the bubble reference
    units, report, reduced, rows = br.simplify(table, k, canonical, 1, True, True, 4, None, 512, None, 1, 0)
    link_ptr, links = lr.links(units, reduced, k, canonical, 1)
    subprocess.run([_cli(), str(fasta), P("a.out")] + tail + outs("pop") + ["--unitigs-clip-tips", "--unitigs-pop-bubbles", "--bubble-max-diff", "1",
                                                                             "--tip-report", P("r.tsv"), "--bubble-report", P("b.tsv")],
                   check=True, timeout=300)
    assert read("pop.fa") == lr.fasta_text_links(units, link_ptr, links) and read("pop.gfa") == lr.gfa_text(units, k, link_ptr, links)
    assert read("r.tsv") == br.report_text(report) and read("b.tsv") == br.bubble_lines(rows)
    # tips alone: the tip loop and its four-field report
    subprocess.run([_cli(), str(fasta), P("d.out")] + tail + outs("clip") + ["--unitigs-clip-tips", "--tip-report", P("r4.tsv")], check=True, timeout=300)
    cunits, creport, creduced = tr.clip(table, k, canonical, 1, None, 512, rounds=4)
    cptr, clinks = lr.links(cunits, creduced, k, canonical, 1)
    assert read("clip.fa") == lr.fasta_text_links(cunits, cptr, clinks) and read("clip.gfa") == lr.gfa_text(cunits, k, cptr, clinks)
    assert read("r4.tsv") == tr.report_text(creport)
    # no rule at all: the graph as counted
    units0, ptr0, links0 = tr.graph(table, k, canonical, 1)
    subprocess.run([_cli(), str(fasta), P("e.out")] + tail + outs("plain"), check=True, timeout=300)
    assert read("plain.fa") == lr.fasta_text_links(units0, ptr0, links0) and read("plain.gfa") == lr.gfa_text(units0, k, ptr0, links0)
    assert read("a.out") == read("d.out") == read("e.out")
