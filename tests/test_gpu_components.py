"""GPU: the connected components of the unitig graph (cfrk_global_unitig_components) and the component of every read
(cfrk_global_read_components), host and device forms, against tests/components_ref.py: the planted graphs of
tests/weak_cases.py, crafted rows without k-mers (deep chains, stars, interleaved chains, the seams of the launch), the
capacity protocol, the refusals, and drop_small_components().  Outputs of the device forms lie in guarded arrays 1 and 3
ELEMENTS off a 64-byte boundary (the contract asks for the alignment of the element type: 4 bytes for comp and the reads'
rows, 8 for the table, whose sums are 64-bit atomics)."""
import ctypes as C

import numpy as np
import pytest

from . import compact_ref as cr
from . import components_ref as cc
from . import unitig_links_ref as lr
from . import unitig_ref as ur
from . import weak_ref as wr
from .test_gpu_bubbles import _csr
from .test_gpu_filter import _Guarded, _upload
from .test_gpu_unitig_links import _same_links
from .test_gpu_unitigs import _job, _same
from .test_gpu_weak import _random_rec, _random_rows
from .weak_cases import KS, PARAMS, ref, weak_input

pytestmark = pytest.mark.gpu

CFRK_ERR_ARG, CFRK_ERR_STATE, CFRK_ERR_LAYOUT, CFRK_ERR_SMALL_BUF = -1, -4, -5, -9
NONE = cc.COMP_NONE


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


def _counter(ctx, canonical):
    """a job that supplies the strand rule and nothing else: the call reads records and rows"""
    import cfrk_amd
    return cfrk_amd.GlobalCounter(ctx, 21, cfrk_amd.CFRK_CANONICAL if canonical else 0, 1000)


def _rec(nS, rng=None):
    import cfrk_amd
    rec = np.zeros(nS, cfrk_amd.UNITIG_DTYPE)
    rec["n_kmers"] = 1 + (np.arange(nS) % 7) if rng is None else rng.integers(1, 50, nS)
    rec["kc"] = rec["n_kmers"] * 3 + (np.arange(nS) % 2)
    return rec


def _device(ctx, g, rec, ptr, links, drop, skew=3, cap=None):
    """the device form: a sizes-only call, then the table at exact capacity (or `cap` rows) -> (comp, table, stats)"""
    import cfrk_amd
    nS = len(rec)
    ins = [_upload(ctx, rec), _upload(ctx, ptr), _upload(ctx, links), _upload(ctx, drop) if drop is not None else 0]
    d_comp = _Guarded(ctx, nS * 4, 4 * skew)
    d_tab = None
    try:
        try:
            n, st = g.unitig_components_device(ins[0], nS, ins[1], ins[2], len(links), ins[3], d_comp.ptr)
            assert n == 0
        except cfrk_amd.CfrkError as e:
            assert e.code == CFRK_ERR_SMALL_BUF
            n, st = e.n_comps, e.stats
        ctx.sync()
        first = d_comp.fetch(nS * 4, np.uint32)
        rows = n if cap is None else cap
        d_tab = _Guarded(ctx, rows * 32, 8 * skew)
        n2, st2 = g.unitig_components_device(ins[0], nS, ins[1], ins[2], len(links), ins[3], d_comp.ptr, d_tab.ptr if rows else 0, rows)
        ctx.sync()
        assert (n2, st2) == (n, st) and (d_comp.fetch(nS * 4, np.uint32) == first).all()
        return first, d_tab.fetch(n * 32, cc.UNITIG_COMPONENT_DTYPE), st
    finally:
        ctx.sync()
        d_comp.fetch(nS * 4)                                        # whatever happened: nothing outside the arrays
        d_comp.free()
        if d_tab is not None:
            d_tab.free()
        for p in ins:
            if p:
                ctx.free(p)


def _equal(got, want, what):
    comp, table, stats = got
    wcomp, wtable, wstats = want
    assert comp.dtype == np.uint32 and comp.shape == wcomp.shape, what
    if not (comp == wcomp).all():
        i = int(np.flatnonzero(comp != wcomp)[0])
        raise AssertionError(f"{what}: comp differs at {int((comp != wcomp).sum())} unitigs, the first {i}: {comp[i]} against {wcomp[i]}")
    assert table.dtype == wtable.dtype and table.tolist() == wtable.tolist(), what
    assert stats == wstats, what


def _both_forms(ctx, g, rec, ptr, links, drop, want=None, what=""):
    want = want if want is not None else cc.components(rec, ptr, links, drop)
    _equal(g.unitig_components(rec, ptr, links, drop), want, (what, "host"))
    for skew in (1, 3):
        _equal(_device(ctx, g, rec, ptr, links, drop, skew), want, (what, "device", skew))
    return want


def _pulled_back(comp_new, into, drop):
    """the components of the compacted graph as a partition of the old kept unitigs, numbered by first appearance"""
    out = np.full(len(into), NONE, np.uint32)
    number = {}
    for j in range(len(into)):
        if drop[j]:
            continue
        c = int(comp_new[int(into[j]["unitig"])])
        out[j] = number.setdefault(c, len(number))
    return out


# ------------------------------------------------------------------ real graphs

@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", KS)
def test_components_of_planted_graphs(ctx, k, canonical):
    """the planted jobs of the weak rule: nothing dropped, and the weak rule's bytes as drop; then the compaction property:
    comp through `into` is the partition of compact_unitigs()' result under its fresh links"""
    table, units, link_ptr, links = ref(k, canonical)
    g = _job(ctx, weak_input(k), k, canonical)
    digest, histo = g.digest(), g.histogram(16)
    data, start, length, rec = g.unitigs(1)
    _same((data, start, length, rec), ur.layout(units))
    _same_links(g.unitig_links(data, start, length), (link_ptr, links))
    want = _both_forms(ctx, g, rec, link_ptr, links, None, what="no drop")
    assert want[2]["n_links"] == len(links)
    assert k == 5 or want[2]["n_components"] >= 3                   # (the floating pieces; at k = 5 everything repeats and joins)
    assert g.digest() == digest and (g.histogram(16) == histo).all()
    drop = (wr.weak(units, link_ptr, links, canonical, *PARAMS(k)[4])[0] != 0).astype(np.uint8)
    want = _both_forms(ctx, g, rec, link_ptr, links, drop, what="weak bytes as drop")
    assert g.digest() == digest and (g.histogram(16) == histo).all()
    new = g.compact_unitigs(data, start, length, rec, link_ptr, links, drop)
    g.mask_unitigs(data, start, length, drop)                       # (links live on the mask)
    new_ptr, new_links = g.unitig_links(new[0], new[1], new[2])
    comp_new = g.unitig_components(new[3], new_ptr, new_links)[0]
    assert (_pulled_back(comp_new, new[4], drop) == want[0]).all()


# ------------------------------------------------------------------ crafted rows, no k-mers

def _no_links(nS):
    return np.zeros(nS + 1, np.int64), np.zeros(0, lr.UNITIG_LINK_DTYPE)


@pytest.mark.parametrize("canonical", [False, True])
def test_a_single_unitig(ctx, canonical):
    g = _counter(ctx, canonical)
    rec = _rec(1)
    for ptr, rows in (_no_links(1), _csr(1, [0], [0], np.zeros(1, np.uint32))):
        want = _both_forms(ctx, g, rec, ptr, rows, None)
        assert want[0].tolist() == [0] and want[1]["n_unitigs"].tolist() == [1] and want[1]["n_links"].tolist() == [len(rows)]
        want = _both_forms(ctx, g, rec, ptr, rows, np.ones(1, np.uint8))
        assert want[0].tolist() == [NONE] and len(want[1]) == 0 and want[2] == {"n_components": 0, "n_unitigs": 0, "n_kmers": 0, "n_links": 0}


def _chain(nS, forward, step=1):
    """unitig i linked to i + step (or i + step to i)"""
    a, b = np.arange(nS - step), np.arange(step, nS)
    return _csr(nS, a if forward else b, b if forward else a, np.zeros(nS - step, np.uint32))


def _want_blocks(rec, ptr, links, comp, drop=None):
    """(comp, table, stats) from a partition known in closed form (ids ascending by first member): numpy only"""
    kept = comp != NONE
    n = int(comp[kept].max()) + 1 if kept.any() else 0
    table = np.zeros(n, cc.UNITIG_COMPONENT_DTYPE)
    c = comp[kept].astype(np.int64)
    src = np.repeat(np.arange(len(rec)), np.diff(ptr))
    live = kept[src] & kept[links["to"]]
    nl = np.bincount(src[live], minlength=len(rec))
    table["kc"] = np.bincount(c, rec["kc"][kept].astype(np.float64), n).astype(np.uint64)      # (small sums: exact in a double)
    table["n_kmers"] = np.bincount(c, rec["n_kmers"][kept], n).astype(np.uint64)
    table["n_links"] = np.bincount(c, nl[kept], n).astype(np.uint64)
    table["n_unitigs"] = np.bincount(c, minlength=n)
    first = np.full(n, len(rec), np.int64)
    np.minimum.at(first, c, np.flatnonzero(kept))
    table["first"] = first
    assert n == 0 or (np.diff(first) > 0).all()
    stats = {"n_components": n, "n_unitigs": int(kept.sum()), "n_kmers": int(table["n_kmers"].sum()), "n_links": int(table["n_links"].sum())}
    return comp, table, stats


@pytest.mark.parametrize("forward", [True, False])
@pytest.mark.parametrize("canonical", [False, True])
def test_a_chain_of_70000(ctx, canonical, forward):
    """one deep tree across every workgroup: where a find without halving, or a missing flatten, shows"""
    nS = 70000
    g = _counter(ctx, canonical)
    rec = _rec(nS)
    ptr, rows = _chain(nS, forward)
    _both_forms(ctx, g, rec, ptr, rows, None, _want_blocks(rec, ptr, rows, np.zeros(nS, np.uint32)))
    drop = np.zeros(nS, np.uint8)                                   # cut in the middle: two components, one unitig without
    drop[35001] = 1
    comp = np.where(np.arange(nS) > 35001, 1, 0).astype(np.uint32)
    comp[35001] = NONE
    _both_forms(ctx, g, rec, ptr, rows, drop, _want_blocks(rec, ptr, rows, comp), "cut")
    _both_forms(ctx, g, rec, ptr, rows, np.ones(nS, np.uint8), _want_blocks(rec, ptr, rows, np.full(nS, NONE, np.uint32)), "all dropped")


@pytest.mark.parametrize("canonical", [False, True])
def test_two_chains_interleaved(ctx, canonical):
    """even and odd unitigs: every wave holds two components, the table's wave loop takes two turns"""
    nS = 70001
    g = _counter(ctx, canonical)
    rec = _rec(nS)
    ptr, rows = _chain(nS, True, 2)
    _both_forms(ctx, g, rec, ptr, rows, None, _want_blocks(rec, ptr, rows, (np.arange(nS) % 2).astype(np.uint32)))


def test_a_star_of_65537(ctx):
    """every unitig links into unitig 0 (canonical rows without mirrors pass the check); without the centre every ray is
    alone, and its link into the dropped centre does not exist"""
    nS = 65537
    g = _counter(ctx, True)
    rec = _rec(nS)
    ptr, rows = _csr(nS, np.arange(1, nS), np.zeros(nS - 1, np.int64), np.zeros(nS - 1, np.uint32))
    want = _both_forms(ctx, g, rec, ptr, rows, None, _want_blocks(rec, ptr, rows, np.zeros(nS, np.uint32)))
    assert want[1]["n_links"].tolist() == [nS - 1]
    drop = np.zeros(nS, np.uint8)
    drop[0] = 1
    comp = (np.arange(nS) - 1).astype(np.uint32)
    comp[0] = NONE
    want = _both_forms(ctx, g, rec, ptr, rows, drop, _want_blocks(rec, ptr, rows, comp), "no centre")
    assert want[2]["n_links"] == 0


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("nS", [255, 256, 257])
def test_block_seams(ctx, nS, canonical):
    g = _counter(ctx, canonical)
    rng = np.random.default_rng(900 + 2 * nS + canonical)
    rec = _random_rec(rng, nS)
    ptr, rows = _random_rows(rng, nS, canonical)
    _both_forms(ctx, g, rec, ptr, rows, None)
    _both_forms(ctx, g, rec, ptr, rows, (rng.integers(0, 4, nS) == 0).astype(np.uint8))
    _both_forms(ctx, g, rec, *_no_links(nS), None)


@pytest.mark.parametrize("side", [-1, 1])
@pytest.mark.parametrize("per_block", [64, 256])
def test_seams_of_the_largest_launch(ctx, per_block, side):
    """nS one below and one above 64 g and 256 g for the g workgroups of the largest launch (16 per compute unit): where
    the grid-stride loops start their second turn.  Chains in blocks of 8, so that the table is large too"""
    grid = 16 * 256                                                 # (an MI355X has 256 compute units; on another device: just sizes)
    nS = per_block * grid + side
    g = _counter(ctx, True)
    rec = _rec(nS)
    a = np.arange(nS - 1)
    a = a[a % 8 != 7]
    ptr, rows = _csr(nS, a, a + 1, np.zeros(len(a), np.uint32))
    want = _want_blocks(rec, ptr, rows, (np.arange(nS) // 8).astype(np.uint32))
    _equal(g.unitig_components(rec, ptr, rows), want, "host")
    _equal(_device(ctx, g, rec, ptr, rows, None, 1), want, "device")


@pytest.mark.parametrize("canonical", [False, True])
def test_random_rows_at_100000(ctx, canonical):
    nS = 100000
    g = _counter(ctx, canonical)
    rng = np.random.default_rng(77 + canonical)
    rec = _rec(nS, rng)
    ptr, rows = _random_rows(rng, nS, canonical)
    want = cc.components(rec, ptr, rows, None)
    assert (want[0] == cc.components_bfs(nS, ptr, rows)).all()
    _equal(g.unitig_components(rec, ptr, rows), want, "host")
    _equal(_device(ctx, g, rec, ptr, rows, None, 3), want, "device")
    # links inside the rows in another order, and a second run: the same bytes
    perm = rows.copy()
    for j in range(nS):
        perm[ptr[j]:ptr[j + 1]] = perm[ptr[j]:ptr[j + 1]][::-1]
    again = _device(ctx, g, rec, ptr, perm, None, 3)
    _equal(again, want, "rows reversed")
    drop = (rng.integers(0, 3, nS) == 0).astype(np.uint8)
    want = cc.components(rec, ptr, rows, drop)
    _equal(_device(ctx, g, rec, ptr, rows, drop, 1), want, "device, drop")
    got = [_device(ctx, g, rec, ptr, rows, drop, 1) for _ in range(2)]
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].tobytes() == got[1][1].tobytes()


def test_links_that_all_point_one_way(ctx):
    """not canonical: 0 -> 1 <- 2 -> 3 <- 4 is one weakly connected component; no unitig reaches all the others"""
    g = _counter(ctx, False)
    ptr, rows = _csr(6, [0, 2, 2, 4], [1, 1, 3, 3], np.zeros(4, np.uint32))
    want = _both_forms(ctx, g, _rec(6), ptr, rows, None)
    assert want[0].tolist() == [0, 0, 0, 0, 0, 1]


def test_full_rows(ctx):
    """rows of exactly 16 links (canonical) and exactly 4 (not canonical), the last link the only one that leaves the block"""
    for canonical, width in ((True, 16), (False, 4)):
        g = _counter(ctx, canonical)
        nS = 40
        frm, to = [], []
        for j in range(0, nS, 10):                                  # unitig j: width - 1 self-links, then the link to j + 9
            frm += [j] * width
            to += [j] * (width - 1) + [j + 9]
        ptr, rows = _csr(nS, frm, to, np.zeros(len(frm), np.uint32))
        assert int(np.diff(ptr).max()) == width
        want = _both_forms(ctx, g, _rec(nS), ptr, rows, None)
        assert want[0][0] == want[0][9] and want[0][10] == want[0][19] != want[0][0]


@pytest.mark.parametrize("canonical", [False, True])
def test_capacity_protocol(ctx, canonical):
    import cfrk_amd
    g = _counter(ctx, canonical)
    rng = np.random.default_rng(5)
    nS = 600
    rec = _random_rec(rng, nS)
    a = np.arange(nS - 1)
    a = a[a % 8 != 7]                                               # chains of 8: 75 components
    ptr, rows = _csr(nS, a, a + 1, np.zeros(len(a), np.uint32))
    want = cc.components(rec, ptr, rows, None)
    n = len(want[1])
    assert n == 75
    _equal(_device(ctx, g, rec, ptr, rows, None, 1, cap=n), want, "cap = n")
    for cap in (n - 1, 0):                                          # too small: comp and the sizes complete, the table untouched
        ins = [_upload(ctx, rec), _upload(ctx, ptr), _upload(ctx, rows)]
        d_comp, d_tab = _Guarded(ctx, nS * 4, 4), _Guarded(ctx, max(cap, 1) * 32, 8)
        with pytest.raises(cfrk_amd.CfrkError) as e:
            g.unitig_components_device(ins[0], nS, ins[1], ins[2], len(rows), 0, d_comp.ptr, d_tab.ptr if cap else 0, cap)
        ctx.sync()
        assert e.value.code == CFRK_ERR_SMALL_BUF and e.value.n_comps == n and e.value.stats == want[2]
        assert (d_comp.fetch(nS * 4, np.uint32) == want[0]).all()
        d_tab.fetch(0)
        d_comp.free(), d_tab.free()
        for p in ins:
            ctx.free(p)
    # the host form
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    comp, tab, st, m = np.zeros(nS, np.uint32), np.full(n * 4, 0xA5A5A5A5A5A5A5A5, np.uint64), (C.c_uint64 * 4)(), C.c_int64()
    rc = ctx._L.cfrk_global_unitig_components(ctx._h, vp(rec), nS, vp(ptr), vp(rows), len(rows), None, vp(comp), vp(tab), n - 1, C.byref(m), st)
    assert rc == CFRK_ERR_SMALL_BUF and m.value == n and (comp == want[0]).all() and list(st) == list(want[2].values())
    assert (tab == 0xA5A5A5A5A5A5A5A5).all()


# ------------------------------------------------------------------ refusals

@pytest.mark.parametrize("canonical", [False, True])
def test_components_refuse_bad_rows(ctx, canonical):
    """each of the five reasons of the shared check, at the first and at the last unitig: CFRK_ERR_LAYOUT naming it, comp all
    CFRK_COMP_NONE, the sizes and stats 0, in both forms"""
    import cfrk_amd
    g = _counter(ctx, canonical)
    nS = 700
    rng = np.random.default_rng(31)
    rec = _random_rec(rng, nS)
    a = np.arange(nS - 1)
    ptr, rows = _csr(nS, a, a + 1, np.zeros(nS - 1, np.uint32))
    ptr, rows = ptr.copy(), rows.copy()
    ptr[nS] = nS                                                    # (the last unitig gets a row too: a self-link)
    rows = np.append(rows, np.array([(nS - 1, 0)], lr.UNITIG_LINK_DTYPE))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def refused(p, r, unitig):
        comp, st, m = np.zeros(nS, np.uint32), (C.c_uint64 * 4)(7, 7, 7, 7), C.c_int64(7)
        rc = ctx._L.cfrk_global_unitig_components(ctx._h, vp(rec), nS, vp(p), vp(r), len(r), None, vp(comp), None, 0, C.byref(m), st)
        assert rc == CFRK_ERR_LAYOUT and ("unitig %d " % unitig) in ctx._L.cfrk_last_error(ctx._h).decode()
        assert (comp == NONE).all() and list(st) == [0, 0, 0, 0] and m.value == 0
        ins = [_upload(ctx, rec), _upload(ctx, p), _upload(ctx, r)]
        d_comp = _Guarded(ctx, nS * 4, 4)
        with pytest.raises(cfrk_amd.CfrkError) as e:
            g.unitig_components_device(ins[0], nS, ins[1], ins[2], len(r), 0, d_comp.ptr)
        ctx.sync()
        assert e.value.code == CFRK_ERR_LAYOUT and ("unitig %d " % unitig) in str(e.value) and e.value.n_comps == 0
        assert (d_comp.fetch(nS * 4, np.uint32) == NONE).all()
        d_comp.free()
        for q in ins:
            ctx.free(q)

    bad = ptr.copy()                                                # link_ptr: does not begin at 0, does not end at n_links
    bad[0] = 1
    refused(bad, rows, 0)
    bad = ptr.copy()
    bad[nS] -= 1
    refused(bad, rows, nS - 1)
    width = 17 if canonical else 5                                  # a row too long: the first, the last
    for at in (0, nS - 1):
        p = np.zeros(nS + 1, np.int64)
        p[at + 1:] = width
        refused(p, np.zeros(width, lr.UNITIG_LINK_DTYPE), at)
    for at in (0, nS - 1):                                          # a target that is no unitig; an undefined flag bit
        r = rows.copy()
        r[ptr[at]]["to"] = nS
        refused(ptr, r, at)
        r = rows.copy()
        r[ptr[at]]["flags"] = 4
        refused(ptr, r, at)
    if not canonical:                                               # more links into one unitig than 4 bases can give
        for target in (0, nS - 1):
            src = [j for j in range(1, 6)]
            p, r = _csr(nS, src, [target] * 5, np.zeros(5, np.uint32))
            refused(p, r, target)
    # CFRK_ERR_ARG, nS = 0, no job
    L, h = ctx._L, ctx._h
    comp, st, m = np.zeros(nS, np.uint32), (C.c_uint64 * 4)(), C.c_int64()
    ok = (vp(rec), nS, vp(ptr), vp(rows), len(rows), None, vp(comp), None, 0, C.byref(m), st)
    for fn in (L.cfrk_global_unitig_components, L.cfrk_global_unitig_components_device):
        for pos, value in ((0, None), (2, None), (3, None), (6, None), (9, None), (10, None), (1, -1), (4, -1), (1, 1 << 32), (8, 1)):
            args = list(ok)
            args[pos] = value
            assert fn(h, *args) == CFRK_ERR_ARG, (pos, value)
        m.value = 7
        assert fn(h, None, 0, None, None, 0, None, None, None, 0, C.byref(m), st) == 0 and m.value == 0 and list(st) == [0, 0, 0, 0]
    with cfrk_amd.Context(0) as c:
        assert c._L.cfrk_global_unitig_components(c._h, None, 0, None, None, 0, None, None, None, 0, C.byref(m), st) == CFRK_ERR_STATE
        assert c._L.cfrk_global_unitig_components_device(c._h, None, 0, None, None, 0, None, None, None, 0, C.byref(m), st) == CFRK_ERR_STATE


# ------------------------------------------------------------------ reads

def _hits(rows):
    """[[(unitig, n_windows), ...] per read] -> (hit_ptr, hits)"""
    import cfrk_amd
    flat = [x for r in rows for x in r]
    hits = np.zeros(len(flat), cfrk_amd.READ_HIT_DTYPE)
    if flat:
        hits["unitig"], hits["n_windows"] = [x[0] for x in flat], [x[1] for x in flat]
    ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=ptr[1:])
    return ptr, hits


def _reads_device(ctx, g, hit_ptr, hits, comp, skew=3):
    nR = len(hit_ptr) - 1
    ins = [_upload(ctx, hit_ptr), _upload(ctx, hits), _upload(ctx, comp)]
    d_out = _Guarded(ctx, nR * 16, 4 * skew)
    try:
        st = g.read_components_device(ins[0], nR, ins[1], len(hits), ins[2], len(comp), d_out.ptr)
        ctx.sync()
        return d_out.fetch(nR * 16, cc.READ_COMPONENT_DTYPE), st
    finally:
        ctx.sync()
        d_out.free()
        for p in ins:
            ctx.free(p)


def _reads_both(ctx, g, hit_ptr, hits, comp):
    want = cc.read_components(hit_ptr, hits, comp)
    got = g.read_components(hit_ptr, hits, comp)
    assert got[0].tolist() == want[0].tolist() and got[1] == want[1]
    for skew in (1, 3):
        got = _reads_device(ctx, g, hit_ptr, hits, comp, skew)
        assert got[0].tolist() == want[0].tolist() and got[1] == want[1], skew
    return want


def test_read_components_crafted(ctx):
    g = _counter(ctx, True)
    comp = np.array([0, 0, 1, NONE, 2, 1], np.uint32)
    rows = [[],                                                     # no hit
            [(1, 5)],                                               # one hit
            [(0, 4), (2, 9), (5, 9), (1, 9)],                       # a tie on windows: the earliest wins; split
            [(0, 3), (1, 8)],                                       # two hits, one component: not split
            [(3, 50)],                                              # a dropped unitig alone
            [(3, 50), (4, 2)],                                      # ... and beside an eligible one
            [(2, 1 << 31), (4, (1 << 32) - 1)],                     # window counts up to 2^32 - 1
            []]                                                     # an empty last row
    ptr, hits = _hits(rows)
    want = _reads_both(ctx, g, ptr, hits, comp)
    assert want[0].tolist() == [(NONE, NONE, 0, 0), (0, 0, 5, 0), (1, 1, 9, 1), (0, 1, 8, 0), (NONE, NONE, 0, 2), (2, 1, 2, 2),
                                (2, 1, (1 << 32) - 1, 1), (NONE, NONE, 0, 0)]
    assert want[1] == {"n_assigned": 5, "n_unassigned": 3, "n_split": 2, "n_dropped": 2}
    # hit_ptr[nR] below n_hits: the hits behind it belong to no read and are not looked at, whatever they hold
    more = np.append(hits, hits[:2])
    more[-1]["unitig"], more[-2]["n_windows"] = 99, 0
    got = g.read_components(ptr, more, comp)
    assert got[0].tolist() == want[0].tolist() and got[1] == want[1]
    _reads_both(ctx, g, np.zeros(1, np.int64), hits[:0], comp)      # no read at all
    _reads_both(ctx, g, ptr, hits, np.full(6, NONE, np.uint32))     # nothing has a component


def test_one_read_of_5000_hits_among_reads_of_one(ctx):
    g = _counter(ctx, True)
    rng = np.random.default_rng(8)
    nS = 3000
    comp = rng.integers(0, 40, nS).astype(np.uint32)
    comp[rng.integers(0, nS, 300)] = NONE
    rows = [[(int(rng.integers(0, nS)), int(rng.integers(1, 9)))] for _ in range(700)]
    rows[333] = [(int(rng.integers(0, nS)), int(rng.integers(1, 9))) for _ in range(5000)]
    _reads_both(ctx, g, *_hits(rows), comp)


def test_read_components_refusals(ctx):
    import cfrk_amd
    g = _counter(ctx, True)
    comp = np.array([0, 1, NONE], np.uint32)
    nR = 600
    rows = [[(i % 3, 1 + i % 5)] for i in range(nR)]
    ptr, hits = _hits(rows)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def refused(p, h, read, why):
        out, st = np.zeros(nR, cc.READ_COMPONENT_DTYPE), (C.c_uint64 * 4)(7, 7, 7, 7)
        rc = ctx._L.cfrk_global_read_components(ctx._h, vp(p), nR, vp(h), len(h), vp(comp), 3, vp(out), st)
        msg = ctx._L.cfrk_last_error(ctx._h).decode()
        assert rc == CFRK_ERR_LAYOUT and ("read %d " % read) in msg and why in msg and list(st) == [0, 0, 0, 0]
        with pytest.raises(cfrk_amd.CfrkError) as e:
            _reads_device(ctx, g, p, h, comp)
        assert e.value.code == CFRK_ERR_LAYOUT and ("read %d " % read) in str(e.value)

    for at in (0, nR - 1):
        bad = ptr.copy()
        if at == 0:
            bad[0] = 1                                              # does not start at 0
        else:
            bad[nR] = len(hits) + 1                                 # leaves [0, n_hits]
        refused(bad, hits, at, "hit_ptr")
        h = hits.copy()
        h[ptr[at]]["unitig"] = 3
        refused(ptr, h, at, "not in the list")
        h = hits.copy()
        h[ptr[at]]["n_windows"] = 0
        refused(ptr, h, at, "no windows")
    bad = ptr.copy()                                                # descends in the middle
    bad[300] = bad[301] + 1
    refused(bad, hits, 299 if bad[300] > len(hits) else 300, "hit_ptr")
    L, h_ = ctx._L, ctx._h
    out, st = np.zeros(nR, cc.READ_COMPONENT_DTYPE), (C.c_uint64 * 4)()
    ok = (vp(ptr), nR, vp(hits), len(hits), vp(comp), 3, vp(out), st)
    for fn in (L.cfrk_global_read_components, L.cfrk_global_read_components_device):
        for pos, value in ((0, None), (2, None), (4, None), (6, None), (7, None), (1, -1), (3, -1), (5, -1), (5, 1 << 32), (3, 1 << 32)):
            args = list(ok)
            args[pos] = value
            assert fn(h_, *args) == CFRK_ERR_ARG, (pos, value)
    with cfrk_amd.Context(0) as c:
        assert c._L.cfrk_global_read_components(c._h, vp(ptr), 0, None, 0, None, 0, None, st) == CFRK_ERR_STATE


@pytest.mark.parametrize("canonical", [False, True])
def test_reads_of_a_real_job(ctx, canonical):
    """read_hits() -> read_components() end to end: the planted strings as reads on their own graph, with the weak rule's
    bytes as drop, so that dropped hits and unassigned reads occur"""
    from .test_gpu_unitigs import _reads
    k = 21
    table, units, link_ptr, links = ref(k, canonical)
    g = _job(ctx, weak_input(k), k, canonical)
    digest = g.digest()
    data, start, length, rec = g.unitigs(1)
    g.unitig_index(data, start, length, 1)
    hit_ptr, hits = g.read_hits(*_reads(weak_input(k)))
    for drop in (None, (wr.weak(units, link_ptr, links, canonical, *PARAMS(k)[4])[0] != 0).astype(np.uint8)):
        comp = g.unitig_components(rec, link_ptr, links, drop)[0]
        want = _reads_both(ctx, g, hit_ptr, hits, comp)
        assert want[1]["n_assigned"] >= 3 and (drop is None or want[1]["n_dropped"] >= 1)
    assert g.digest() == digest


# ------------------------------------------------------------------ drop_small_components

@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [12, 21, 33])
def test_drop_small_components(ctx, k, canonical):
    """the planted input has one large component and floating pieces of 4, 4, k + 3 and 2k + 1 k-mers: what is left is
    exactly the kept unitigs of the first list, byte for byte and in their order"""
    table, units, link_ptr, links = ref(k, canonical)
    comp, tab, _ = cc.components(ur.layout(units)[3], link_ptr, links)
    for min_kmers in (0, 5, k + 4, 2 * k + 2):
        g = _job(ctx, weak_input(k), k, canonical)
        digest = g.digest()
        small = tab["n_kmers"] < min_kmers
        keep = [j for j in range(len(units)) if not small[comp[j]]]
        got, counts = g.drop_small_components(min_kmers)
        assert counts == (int(small.sum()), len(units) - len(keep))
        _same(got, ur.layout([units[j] for j in keep]))
        assert g.digest() == digest
        assert g.mask_count() == sum(int(units[j][2]) for j in range(len(units)) if small[comp[j]])
    assert int((tab["n_kmers"] < 2 * k + 2).sum()) >= 4 and int((tab["n_kmers"] >= 2 * k + 2).sum()) >= 1


# ------------------------------------------------------------------ CLI

@pytest.mark.parametrize("k,canonical", [(12, False), (21, True), (33, False)])
def test_cli_components(ctx, tmp_path, k, canonical):
    """CFILE, RFILE and --unitigs-min-component-kmers against the reference texts on the planted input (one large component
    and floating pieces); the subset property; every other output byte for byte what it is without the new options"""
    import subprocess
    from .test_gpu_query import _cli
    from .test_gpu_unitigs import _reads
    from .test_gpu_weak import _fasta
    seqs = weak_input(k)
    fasta = tmp_path / "in.fa"
    _fasta(fasta, seqs)
    table, units, link_ptr, links = ref(k, canonical)
    rec = ur.layout(units)[3]
    comp, tab, _ = cc.components(rec, link_ptr, links)
    tail = [str(k), "--global"] + (["--canonical"] if canonical else [])
    P = lambda name: str(tmp_path / name)
    read = lambda name: open(tmp_path / name, "rb").read()
    outs = lambda t: ["--unitigs-out", P(t + ".fa"), "--unitigs-links", "--unitigs-gfa", P(t + ".gfa"), "--unitigs-map", str(fasta), "--unitigs-map-out", P(t + ".gaf")]
    subprocess.run([_cli(), str(fasta), P("a.out")] + tail + outs("plain"), check=True, timeout=300)
    subprocess.run([_cli(), str(fasta), P("b.out")] + tail + outs("comp") + ["--unitigs-components", P("c.tsv"), "--unitigs-map-components", P("r.tsv")],
                   check=True, timeout=300)
    for ext in (".fa", ".gfa", ".gaf"):
        assert read("comp" + ext) == read("plain" + ext), ext
    assert read("plain.fa") == lr.fasta_text_links(units, link_ptr, links) and read("a.out") == read("b.out")
    assert read("c.tsv").decode() == cc.components_text(tab, k)
    subprocess.run([_cli(), str(fasta), P("t.out")] + tail + outs("tag") + ["--unitigs-component-tags"], check=True, timeout=300)
    assert read("tag.fa") == cc.tagged_fasta(read("plain.fa"), comp) and read("tag.gfa") == cc.tagged_gfa(read("plain.gfa"), comp)
    assert read("tag.gaf") == read("plain.gaf") and read("tag.fa").count(b" CC:i:") == len(units)
    g = _job(ctx, seqs, k, canonical)
    lay = g.unitigs(1)
    g.unitig_index(*lay[:3], 1)
    hit_ptr, hits = g.read_hits(*_reads(seqs))
    want_rows, want_stats = cc.read_components(hit_ptr, hits, comp)
    assert read("r.tsv").decode() == cc.read_components_text(want_rows) and want_stats["n_assigned"] == len(want_rows)
    # every component below 2k + 2 k-mers goes: the four floating pieces at least, the large component stays
    N = 2 * k + 2
    small = tab["n_kmers"] < N
    assert small.sum() >= 4 and not small.all()
    keep = [j for j in range(len(units)) if not small[comp[j]]]
    new_of = {j: i for i, j in enumerate(keep)}
    kept_units = [units[j] for j in keep]
    rows = [[(new_of[int(to)], int(f)) for to, f in links[link_ptr[j]:link_ptr[j + 1]].tolist()] for j in keep]
    kptr = np.zeros(len(keep) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=kptr[1:])
    klinks = np.array([x for r in rows for x in r], lr.UNITIG_LINK_DTYPE).reshape(int(kptr[-1]))
    subprocess.run([_cli(), str(fasta), P("d.out")] + tail + outs("big") + ["--unitigs-components", P("c2.tsv"), "--unitigs-map-components", P("r2.tsv"),
                                                                           "--unitigs-min-component-kmers", str(N), "--unitigs-component-tags"],
                   check=True, timeout=300)
    kcomp, ktab, _ = cc.components(ur.layout(kept_units)[3], kptr, klinks)
    assert read("big.fa") == cc.tagged_fasta(lr.fasta_text_links(kept_units, kptr, klinks), kcomp)    # the subset property, links renumbered
    assert read("big.gfa") == cc.tagged_gfa(lr.gfa_text(kept_units, k, kptr, klinks), kcomp)
    assert read("c2.tsv").decode() == cc.components_text(ktab, k) and all((ktab[f] == tab[~small][f]).all() for f in ("kc", "n_kmers", "n_links", "n_unitigs"))
    g2, counts = g.drop_small_components(N)
    _same(g2, ur.layout(kept_units))
    assert counts == (int(small.sum()), len(units) - len(keep))
    g.unitig_index(*g2[:3], 1)
    hit_ptr, hits = g.read_hits(*_reads(seqs))
    want_rows, want_stats = cc.read_components(hit_ptr, hits, kcomp)
    assert read("r2.tsv").decode() == cc.read_components_text(want_rows) and want_stats["n_unassigned"] >= 4
    assert read("d.out") == read("a.out")                           # the counts' own output does not see the options
