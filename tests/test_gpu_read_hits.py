"""GPU: the position map, point lookups in it and the hits of reads on the unitigs (cfrk_global_unitig_index / _locate /
_read_hits and their device forms) against tests/read_hits_ref.py, a dictionary-and-strings statement of the contract
that shares nothing with the product: the unitig tests' k grid on both strand rules and two thresholds; the seams of the
read size classes with the most hits (every window its own) and the fewest (one hit across all lanes and rounds); a
300 000-node chain and ring beside 10 000 single-node unitigs; the k = 32 all-T key; crafted hash collisions; the capacity
protocol and the state rules; the consistency check; reads and unitigs past 2^32 bytes; the CLI."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from . import hash_craft as hc
from . import read_hits_ref as hr
from . import unitig_ref as ur
from .test_gpu_filter import _Guarded, _upload
from .test_gpu_query import _cli
from .test_gpu_unitigs import KS, _input, _job, _kmers31, _rand, _reads, _table, long_genome  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu

CFRK_ERR_ARG, CFRK_ERR_STATE, CFRK_ERR_LAYOUT, CFRK_ERR_SMALL_BUF = -1, -4, -5, -9
NONE = hr.POS_NONE


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


_GRAPHS = {}


def _graph(k, canonical, min_count):
    key = (k, canonical, min_count)
    if key not in _GRAPHS:
        _GRAPHS[key] = hr.Graph(_table(_input(k), k, canonical), k, canonical, min_count)
    return _GRAPHS[key]


def _keys(kmers):
    return (np.array([ur.key_of(x)[0] for x in kmers], np.uint64), np.array([ur.key_of(x)[1] for x in kmers], np.uint64))


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if not (got == want).all():
        i = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{what}: {int((got != want).sum())} differ, the first at {i}: {got[i]} against {want[i]}")


def _locate_device(ctx, g, lo, hi, skew=4):
    """the device form with the output `skew` bytes off a 64-byte boundary"""
    n = len(lo)
    d_lo, d_hi, d_out = _upload(ctx, lo), (_upload(ctx, hi) if hi is not None else 0), _Guarded(ctx, n * 8, skew)
    g.locate_device(d_lo, d_hi, n, d_out.ptr)
    ctx.sync()
    out = d_out.fetch(n * 8, hr.UNITIG_POS_DTYPE)
    for p in (d_lo, d_hi):
        if p:
            ctx.free(p)
    d_out.free()
    return out


def _hits_device(ctx, g, data, start, length, skew=3):
    """the device form: a sizes-only call, then exact capacity, the read data `skew` bytes off a 64-byte boundary"""
    import cfrk_amd
    nS = len(start)
    d_data, d_start, d_length = _upload(ctx, data, skew), _upload(ctx, start), _upload(ctx, length)
    d_ptr = _Guarded(ctx, (nS + 1) * 8)
    args = (d_data + skew, d_start, d_length, len(data), nS, d_ptr.ptr)
    try:
        n = g.read_hits_device(*args, 0, 0)
        assert n == 0
    except cfrk_amd.CfrkError as e:
        assert e.code == CFRK_ERR_SMALL_BUF
        n = e.n_hits
    ptr = d_ptr.fetch((nS + 1) * 8, np.int64)
    assert ptr[0] == 0 and ptr[-1] == n
    d_hits = _Guarded(ctx, n * 16, 4)
    assert g.read_hits_device(*args, d_hits.ptr, n) == n
    ctx.sync()
    hits = d_hits.fetch(n * 16, hr.READ_HIT_DTYPE)
    _same(d_ptr.fetch((nS + 1) * 8, np.int64), ptr, "hit_ptr of the second call")
    for p in (d_data, d_start, d_length):
        ctx.free(p)
    d_ptr.free()
    d_hits.free()
    return ptr, hits


def _index(g, G, min_count):
    data, start, length, _ = ur.layout(G.units)
    g.unitig_index(data, start, length, min_count)
    return data, start, length


# ------------------------------------------------------------------ the grid against the reference

@pytest.mark.parametrize("min_count", [1, 2])
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", KS)
def test_locate_and_read_hits(ctx, k, canonical, min_count):
    seqs = _input(k)
    table = _table(seqs, k, canonical)
    G = _graph(k, canonical, min_count)
    g = _job(ctx, seqs, k, canonical)
    digest = g.digest()
    _index(g, G, min_count)
    rng = np.random.default_rng(100 + k)
    stored = sorted(table)                                          # (at min_count 2 some of them are not solid)
    kmers = stored + [ur.rc(x) for x in stored] + [_rand(rng, k) for _ in range(200)]
    lo, hi = _keys(kmers)
    want = G.locate_rows(kmers)
    assert (want["unitig"] != NONE).sum() >= len(G.solid) and (k < 12 or (want["unitig"] == NONE).sum() >= 100)
    _same(g.locate(lo, hi), want, "locate, host form")
    _same(_locate_device(ctx, g, lo, hi), want, "locate, device form")
    if k <= 32:
        _same(g.locate(lo, None), want, "locate without keys_hi")
    # bits at or above 2k: no such k-mer
    if k < 32:
        bad = (lo[:50] | np.uint64(1 << (2 * k)), hi[:50])
    elif k == 32:
        bad = (lo[:50], hi[:50] | np.uint64(1))
    elif k < 64:
        bad = (lo[:50], hi[:50] | np.uint64(1 << (2 * k - 64)))
    else:
        bad = None
    if bad is not None:
        got = g.locate(*bad)
        assert (got["unitig"] == NONE).all() and (got["at"] == NONE).all()
    # the reads: the input, its reverse complements, every circle walked twice, an invalid code in the middle, short reads
    strings = [s for s, _ in seqs]
    reads = strings + [ur.rc(s) for s in strings] + [s + s[k - 1:] for s, _, _, circ in G.units if circ]
    g0 = strings[0]
    reads += [g0[:1500] + "N" + g0[1501:], g0[:k - 1], ""]
    w_ptr, w_hits = G.hit_rows(reads)
    assert len(w_hits) > len(reads) // 2
    data, start, length = hr.read_codes(reads)
    ptr, hits = g.read_hits(data, start, length)
    _same(ptr, w_ptr, "hit_ptr, host form")
    _same(hits, w_hits, "hits, host form")
    ptr, hits = _hits_device(ctx, g, data, start, length)
    _same(ptr, w_ptr, "hit_ptr, device form")
    _same(hits, w_hits, "hits, device form")
    assert g.digest() == digest


# ------------------------------------------------------------------ the seams of the size classes

@pytest.mark.parametrize("canonical", [False, True])
def test_size_class_seams_every_window_its_own_hit(ctx, canonical):
    """all 256 4-mers counted once: every unitig is one node, so n_hits is the number of windows"""
    k = 4
    every = [("".join(ur.BASES[(i >> s) & 3] for s in (6, 4, 2, 0)), 1) for i in range(256)]
    G = hr.Graph(_table(every, k, canonical), k, canonical)
    assert all(len(s) == k for s in G.seqs)
    g = _job(ctx, every, k, canonical)
    _index(g, G, 1)
    rng = np.random.default_rng(8)
    windows = [256, 257, 2048, 2049, 10000]
    reads = [_rand(rng, w + k - 1) for w in windows]
    data, start, length = hr.read_codes(reads)
    w_ptr, w_hits = G.hit_rows(reads)
    assert w_ptr.tolist() == np.concatenate([[0], np.cumsum(windows)]).tolist() and (w_hits["n_windows"] == 1).all()
    for ptr, hits in (_hits_device(ctx, g, data, start, length), g.read_hits(data, start, length)):
        assert ptr[-1] == sum(windows)
        _same(ptr, w_ptr, "hit_ptr")
        _same(hits, w_hits, "hits")


def _chain_job(ctx, G, extra=()):
    import cfrk_amd
    g = cfrk_amd.GlobalCounter(ctx, 31, cfrk_amd.CFRK_CANONICAL, 400000)
    if len(extra):
        g.add(np.concatenate([G, [np.int8(-1)], extra]).astype(np.int8))
    else:
        g.add(np.append(G, np.int8(-1)))
    return g


def test_size_class_seams_one_hit_per_read(ctx, long_genome):
    """error-free reads of 257, 2049 and 10 000 windows from the 300 000-base chain, forward and reverse-complemented:
    one hit each that spans every lane and round, at an offset known in closed form"""
    G = long_genome
    R = (3 - G[::-1]).astype(np.int8)
    g = _chain_job(ctx, G)
    data, start, length, rec = g.unitigs(1)
    assert list(length) == [len(G)]
    as_given = bool((data[:len(G)] == G).all())                     # else the unitig is the reverse complement
    g.unitig_index(data, start, length, 1)
    pieces, want = [], []
    for W, a in ((257, 1000), (2049, 7), (10000, 123456), (257, len(G) - 257 - 30), (12289, 0)):
        n = W + 30
        b = len(G) - a - n                                          # where rc(G[a : a + n]) begins in R
        pieces += [G[a:a + n], R[b:b + n]]
        fwd, rev = (a, 0), (b, 1)                                   # offset and minus when the unitig is G
        if not as_given:
            fwd, rev = (b, 1), (a, 0)
        want += [(0, fwd[0] << 1 | fwd[1], 0, W), (0, (len(G) - rev[0] - n) << 1 | rev[1], 0, W)]
    rdata = np.concatenate([np.append(p, np.int8(-1)) for p in pieces]).astype(np.int8)
    rlen = np.array([len(p) for p in pieces], np.int32)
    rstart = (np.concatenate([[0], np.cumsum(rlen + 1)[:-1]])).astype(np.int64)
    ptr, hits = _hits_device(ctx, g, rdata, rstart, rlen)
    assert ptr.tolist() == list(range(len(pieces) + 1))
    _same(hits, np.array(want, hr.READ_HIT_DTYPE), "one hit per read")


# ------------------------------------------------------------------ a long unitig beside many short ones

def _expect_positions(udata, ustart, ulength, j, q_fwd, q_rc):
    """where the oriented 31-mers q (forward words and their reverse complements) lie on unitig j, by numpy"""
    u = udata[ustart[j]:ustart[j] + ulength[j]]
    u_fwd = _kmers31(u)
    u_rc = _kmers31((3 - u[::-1]).astype(np.int8))[::-1]
    u_node = np.minimum(u_fwd, u_rc)
    order = np.argsort(u_node)
    p = order[np.searchsorted(u_node[order], np.minimum(q_fwd, q_rc))]
    assert (u_node[p] == np.minimum(q_fwd, q_rc)).all()
    out = np.zeros(len(q_fwd), hr.UNITIG_POS_DTYPE)
    out["unitig"] = j
    out["at"] = (p.astype(np.uint32) << 1) | (u_fwd[p] != q_fwd).astype(np.uint32)
    return out


@pytest.mark.parametrize("ring", [False, True])
def test_long_unitig_beside_single_nodes(ctx, long_genome, ring):
    """one unitig of 300 000 nodes among 10 000 single-node ones (the chain), and the ring alone: locate of every key
    of the genome in genome order steps through the unitig one position at a time"""
    G = long_genome
    n = len(G)
    rng = np.random.default_rng(77)
    if ring:
        seq, extra = np.concatenate([G, G[:30]]).astype(np.int8), ()
    else:
        singles = rng.integers(0, 4, (10000, 32)).astype(np.int8)
        singles[:, 31] = -1
        seq, extra = G, singles.reshape(-1)
    g = _chain_job(ctx, seq, extra)
    udata, ustart, ulength, rec = g.unitigs(1)
    j = int(np.argmax(ulength))
    assert rec["n_kmers"][j] == (n if ring else n - 30)
    if not ring:
        assert len(ustart) >= 10001 - 5 and (np.delete(ulength, j) <= 33).all()
    d = [_upload(ctx, udata), _upload(ctx, ustart), _upload(ctx, ulength)]
    g.unitig_index_device(1, d[0], d[1], d[2], len(udata), len(ustart))
    q_fwd = _kmers31(seq)
    q_rc = _kmers31((3 - seq[::-1]).astype(np.int8))[::-1]
    want = _expect_positions(udata, ustart, ulength, j, q_fwd, q_rc)
    step = np.diff((want["at"] >> 1).astype(np.int64))
    assert (want["at"] & 1).min() == (want["at"] & 1).max()
    assert ((np.abs(step) == 1).sum() >= len(step) - 1)             # arange, up or down, but for the ring's cut
    lo = q_fwd
    _same(_locate_device(ctx, g, lo, None, 0), want, "locate in genome order")
    _same(g.locate(q_rc[:5000]), _expect_positions(udata, ustart, ulength, j, q_rc[:5000], q_fwd[:5000]), "reverse complements")
    if not ring:                                                    # every single node: its own unitig, p = 0
        s_fwd = _kmers31(np.ascontiguousarray(singles[:, :31]).reshape(-1))[::31][:len(singles)]
        got = g.locate(s_fwd)
        assert (got["unitig"] != NONE).all() and (got["unitig"] != j).sum() >= len(singles) - 5
        small = got[got["unitig"] != j]
        assert ((small["at"] >> 1) <= 2).all()
    for p in d:
        ctx.free(p)


# ------------------------------------------------------------------ special keys and indexes

def test_k32_all_t(ctx):
    rng = np.random.default_rng(32)
    seqs = [(_rand(rng, 50) + "T" * 45 + _rand(rng, 50), 2), ("G" + "T" * 32 + "C", 1), (_rand(rng, 200), 1)]
    table = _table(seqs, 32, False)
    assert "T" * 32 in table
    g = _job(ctx, seqs, 32, False)
    for min_count in (1, 2):
        G = hr.Graph(table, 32, False, min_count)
        _index(g, G, min_count)
        kmers = sorted(table) + ["T" * 31 + "A"]
        lo, hi = _keys(kmers)
        want = G.locate_rows(kmers)
        assert want[kmers.index("T" * 32)]["unitig"] != NONE
        _same(g.locate(lo), want, "locate")
        reads = [s for s, _ in seqs]
        data, start, length = hr.read_codes(reads)
        w_ptr, w_hits = G.hit_rows(reads)
        ptr, hits = _hits_device(ctx, g, data, start, length)
        _same(ptr, w_ptr, "hit_ptr")
        _same(hits, w_hits, "hits")


@pytest.mark.parametrize("k", [21, 33])
def test_crafted_collisions(ctx, k):
    """a chain in an index of 1024 slots beside 300 keys crafted to home on the slot of one of its nodes and on the last
    slot, through the wrap: the slot-returning probes of the claims and of the lookups run long"""
    rng = np.random.default_rng(k)
    chain = _rand(rng, 100 + k - 1)
    two = k > 32
    first = min(chain[40:40 + k], ur.rc(chain[40:40 + k]))
    slot = int(hc.home(*[np.uint64(w) for w in ur.key_of(first)], 10, two)[0])
    seqs = [(chain, 1)]
    for s in (slot, 1023):
        lo, hi = hc.keys_homing_on(s, 10, k, 150, canonical=True, two_word=two, rng=rng)
        seqs += [(ur.str_of(a, b, k), 1) for a, b in zip(lo, hi)]
    table = _table(seqs, k, True)
    G = hr.Graph(table, k, True, 1)
    g = _job(ctx, seqs, k, True)
    _index(g, G, 1)
    assert g.hash_geometry()[1] == 10
    kmers = sorted(table) + [ur.rc(x) for x in sorted(table)]
    _same(g.locate(*_keys(kmers)), G.locate_rows(kmers), "locate")
    reads = [chain, ur.rc(chain)] + [s for s, _ in seqs[1:40]]
    data, start, length = hr.read_codes(reads)
    w_ptr, w_hits = G.hit_rows(reads)
    ptr, hits = _hits_device(ctx, g, data, start, length)
    _same(ptr, w_ptr, "hit_ptr")
    _same(hits, w_hits, "hits")


# ------------------------------------------------------------------ protocol and state

def test_protocol_and_state(ctx):
    import cfrk_amd
    k, canonical = 21, True
    seqs = _input(k)
    G = _graph(k, canonical, 1)
    g = _job(ctx, seqs, k, canonical)
    L, h = ctx._L, ctx._h
    udata, ustart, ulength, _ = ur.layout(G.units)
    reads = [s for s, _ in seqs[:12]]
    data, start, length = hr.read_codes(reads)
    nS = len(start)
    w_ptr, w_hits = G.hit_rows(reads)
    n = len(w_hits)
    assert n >= 3
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    lo, hi = _keys(sorted(G.solid)[:10])
    out, ptr, got_n = np.zeros(10, hr.UNITIG_POS_DTYPE), np.zeros(nS + 1, np.int64), C.c_int64(-1)
    d_word = ctx.alloc(64)

    def state_errors():
        assert L.cfrk_global_locate(h, vp(lo), vp(hi), 10, vp(out)) == CFRK_ERR_STATE
        assert L.cfrk_global_locate(h, None, None, 0, None) == CFRK_ERR_STATE
        assert L.cfrk_global_read_hits(h, vp(data), vp(start), vp(length), len(data), nS, vp(ptr), None, 0, C.byref(got_n)) == CFRK_ERR_STATE
        with pytest.raises(cfrk_amd.CfrkError) as e:
            g.read_hits_device(0, 0, 0, 0, 0, d_word, 0, 0)
        assert e.value.code == CFRK_ERR_STATE
        with pytest.raises(cfrk_amd.CfrkError) as e:
            g.locate_device(0, 0, 0, 0)
        assert e.value.code == CFRK_ERR_STATE

    state_errors()                                                  # before unitig_index
    g.unitig_index(udata, ustart, ulength, 1)
    _same(g.locate(lo, hi), G.locate_rows(sorted(G.solid)[:10]), "locate")
    # sizes only and a capacity one short, host and device form: hit_ptr complete, hits untouched
    assert L.cfrk_global_read_hits(h, vp(data), vp(start), vp(length), len(data), nS, vp(ptr), None, 0, C.byref(got_n)) == CFRK_ERR_SMALL_BUF
    assert got_n.value == n
    _same(ptr, w_ptr, "hit_ptr of the sizes-only call")
    short = np.full(n - 1, 0x5A5A5A5A, np.uint32).repeat(4).view(hr.READ_HIT_DTYPE)
    ptr[:] = -1
    assert L.cfrk_global_read_hits(h, vp(data), vp(start), vp(length), len(data), nS, vp(ptr), vp(short), n - 1, C.byref(got_n)) == CFRK_ERR_SMALL_BUF
    assert got_n.value == n and (short["unitig"] == 0x5A5A5A5A).all() and (short["n_windows"] == 0x5A5A5A5A).all()
    _same(ptr, w_ptr, "hit_ptr of the short call")
    d = [_upload(ctx, data), _upload(ctx, start), _upload(ctx, length)]
    d_ptr, d_hits = _Guarded(ctx, (nS + 1) * 8), _Guarded(ctx, (n - 1) * 16, 4)
    for hits_ptr, cap in ((0, 0), (d_hits.ptr, n - 1)):
        with pytest.raises(cfrk_amd.CfrkError) as e:
            g.read_hits_device(d[0], d[1], d[2], len(data), nS, d_ptr.ptr, hits_ptr, cap)
        assert e.value.code == CFRK_ERR_SMALL_BUF and e.value.n_hits == n
        ctx.sync()
        _same(d_ptr.fetch((nS + 1) * 8, np.int64), w_ptr, "device hit_ptr")
        d_hits.fetch(0)                                             # nothing written: every byte is still a guard byte
    # cap = the number of windows is always enough
    windows = int(sum(max(0, len(r) - k + 1) for r in reads))
    big = np.zeros(windows, hr.READ_HIT_DTYPE)
    assert L.cfrk_global_read_hits(h, vp(data), vp(start), vp(length), len(data), nS, vp(ptr), vp(big), windows, C.byref(got_n)) == 0
    _same(big[:n], w_hits, "hits in a roomy array")
    # no reads; a read outside [0, nN) gets an empty row in the device form
    d_one = _Guarded(ctx, 8)
    assert g.read_hits_device(0, 0, 0, 0, 0, d_one.ptr, 0, 0) == 0
    assert d_one.fetch(8, np.int64)[0] == 0
    d_one.free()
    wild = start.copy()
    wild[1], wild[2] = -5, len(data) - 3
    ctx.h2d(d[1], wild)
    with pytest.raises(cfrk_amd.CfrkError) as e:
        g.read_hits_device(d[0], d[1], d[2], len(data), nS, d_ptr.ptr, 0, 0)
    row = np.diff(d_ptr.fetch((nS + 1) * 8, np.int64))
    assert row[1] == 0 and row[2] == 0 and (row[3:] == np.diff(w_ptr)[3:]).all()
    # the CFRK_ERR_ARG cases
    a = (vp(data), vp(start), vp(length))
    assert L.cfrk_global_read_hits(h, *a, -1, nS, vp(ptr), None, 0, C.byref(got_n)) == CFRK_ERR_ARG
    assert L.cfrk_global_read_hits(h, *a, len(data), -1, vp(ptr), None, 0, C.byref(got_n)) == CFRK_ERR_ARG
    assert L.cfrk_global_read_hits(h, *a, len(data), nS, vp(ptr), None, 0, None) == CFRK_ERR_ARG
    assert L.cfrk_global_read_hits(h, *a, len(data), nS, None, None, 0, C.byref(got_n)) == CFRK_ERR_ARG
    assert L.cfrk_global_read_hits(h, *a, len(data), nS, vp(ptr), None, 5, C.byref(got_n)) == CFRK_ERR_ARG
    assert L.cfrk_global_read_hits_device(h, None, None, None, len(data), nS, vp(ptr), None, 0, C.byref(got_n)) == CFRK_ERR_ARG
    u = (vp(udata), vp(ustart), vp(ulength))
    assert L.cfrk_global_locate(h, vp(lo), vp(hi), -1, vp(out)) == CFRK_ERR_ARG
    assert L.cfrk_global_locate(h, None, None, 3, vp(out)) == CFRK_ERR_ARG
    assert L.cfrk_global_locate_device(h, vp(lo), vp(hi), 3, None) == CFRK_ERR_ARG
    _same(g.locate(lo, hi), G.locate_rows(sorted(G.solid)[:10]), "the map survives refused calls")
    assert L.cfrk_global_unitig_index(h, 1, *u, -1, len(ustart)) == CFRK_ERR_ARG
    assert L.cfrk_global_unitig_index(h, 1, *u, len(udata), -1) == CFRK_ERR_ARG
    assert L.cfrk_global_unitig_index(h, 1, None, None, None, len(udata), len(ustart)) == CFRK_ERR_ARG
    assert L.cfrk_global_unitig_index_device(h, 1, *u, len(udata), 1 << 32) == CFRK_ERR_ARG
    # a further add: the result changed, the map is gone until it is built again
    g.add(*_reads([(_rand(np.random.default_rng(1), 60), 1)]))
    state_errors()
    with pytest.raises(cfrk_amd.CfrkError) as e:                    # (and the old list is no longer this job's)
        g.unitig_index(udata, ustart, ulength, 1)
    assert e.value.code == CFRK_ERR_LAYOUT
    state_errors()
    for p in d + [d_word]:
        ctx.free(p)
    d_ptr.free()
    d_hits.free()


def test_need_a_job():
    import cfrk_amd
    with cfrk_amd.Context(0) as c:
        L, h = c._L, c._h
        z, n = np.zeros(4, np.uint64), C.c_int64()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        assert L.cfrk_global_unitig_index(h, 1, None, None, None, 0, 0) == CFRK_ERR_STATE
        assert L.cfrk_global_unitig_index_device(h, 1, None, None, None, 0, 0) == CFRK_ERR_STATE
        assert L.cfrk_global_locate(h, vp(z), vp(z), 1, vp(z)) == CFRK_ERR_STATE
        assert L.cfrk_global_read_hits(h, None, None, None, 0, 0, vp(z), None, 0, C.byref(n)) == CFRK_ERR_STATE
        # a job without solid keys: nS = 0 is fine, every key is nowhere, every read has no hit
        for k in (5, 31, 40):
            g = cfrk_amd.GlobalCounter(c, k, 0, 1000)
            g.unitig_index(np.zeros(0, np.int8), np.zeros(0, np.int64), np.zeros(0, np.int32))
            got = g.locate(z, z)
            assert (got["unitig"] == NONE).all() and (got["at"] == NONE).all()
            ptr, hits = g.read_hits(*hr.read_codes(["ACGT" * 20, ""]))
            assert ptr.tolist() == [0, 0, 0] and len(hits) == 0


# ------------------------------------------------------------------ the consistency check

def _refused(ctx, g, data, start, length, min_count):
    import cfrk_amd
    d = [_upload(ctx, data), _upload(ctx, start), _upload(ctx, length)]
    with pytest.raises(cfrk_amd.CfrkError) as e:
        g.unitig_index_device(min_count, d[0], d[1], d[2], len(data), len(start))
    for p in d:
        ctx.free(p)
    assert e.value.code == CFRK_ERR_LAYOUT
    with pytest.raises(cfrk_amd.CfrkError) as e2:                   # after an error there is no map
        g.locate(np.zeros(1, np.uint64), np.zeros(1, np.uint64))
    assert e2.value.code == CFRK_ERR_STATE
    m = re.search(r"unitig (\d+) ", str(e.value))
    return (int(m.group(1)) if m else None), str(e.value)


@pytest.mark.parametrize("k,canonical", [(21, True), (12, False), (40, True)])
def test_consistency_check(ctx, k, canonical):
    g = _job(ctx, _input(k), k, canonical)
    G1, G2 = _graph(k, canonical, 1), _graph(k, canonical, 2)
    data, start, length, _ = ur.layout(G1.units)
    digest = g.digest()
    # the unitigs of threshold 2 against min_count 1: every k-mer of theirs is solid and claimed once, so none of them
    # offends; the keys counted once lie in none of them
    named, msg = _refused(ctx, g, *ur.layout(G2.units)[:3], 1)
    assert named is None and "lies in none of the unitigs" in msg
    # the unitigs of threshold 1 against min_count 2: the first unitig with a key counted once
    weak = {x for x in G1.solid if x not in G2.solid}
    first = min(j for j, s in enumerate(G1.seqs) if any(G1.node(s[p:p + k]) in weak for p in range(len(s) - k + 1)))
    named, msg = _refused(ctx, g, data, start, length, 2)
    assert named == first and "not a solid key" in msg
    # one base edited in the middle of the longest unitig: its ends are untouched
    j = int(np.argmax(length))
    assert length[j] >= 3 * k
    table = _table(_input(k), k, canonical)
    at = int(start[j]) + int(length[j]) // 2
    for c in range(1, 4):
        edited = data.copy()
        edited[at] = (edited[at] + c) & 3
        s = "".join(ur.BASES[x] for x in edited[start[j]:start[j] + length[j]])
        mid = int(length[j]) // 2
        if any(G1.node(s[p:p + k]) not in table for p in range(mid - k + 1, mid + 1)):
            break
    named, msg = _refused(ctx, g, edited, start, length, 1)
    assert named == j
    bad = data.copy()
    bad[at] = -1
    named, msg = _refused(ctx, g, bad, start, length, 1)
    assert named == j and "invalid code" in msg
    # a unitig entered twice: the second copy is the one that claims again
    j = 3
    seq = data[start[j]:start[j] + length[j] + 1]
    named, msg = _refused(ctx, g, np.concatenate([data, seq]), np.append(start, len(data)), np.append(length, length[j]), 1)
    assert named == len(start) and "as well" in msg
    # a length below k; a start that runs backwards
    short = length.copy()
    short[5] = k - 1
    named, msg = _refused(ctx, g, data, start, short, 1)
    assert named == 5 and "shorter than k" in msg
    back = start.copy()
    back[7] = start[6]
    named, msg = _refused(ctx, g, data, back, length, 1)
    assert named == 7
    # a unitig removed from the list: no unitig offends
    named, msg = _refused(ctx, g, data, np.delete(start, 2), np.delete(length, 2), 1)
    assert named is None and "lies in none of the unitigs" in msg
    # wild tables: nothing outside the buffers is touched, the call returns
    rng = np.random.default_rng(5)
    wild_s = rng.integers(-2 ** 62, 2 ** 62, len(start)).astype(np.int64)
    wild_l = rng.integers(-2 ** 31, 2 ** 31 - 1, len(start)).astype(np.int32)
    assert _refused(ctx, g, data, wild_s, wild_l, 1)[0] is not None
    assert _refused(ctx, g, data, np.sort(wild_s), length, 1)[0] is not None
    # and the right list is accepted afterwards
    g.unitig_index(data, start, length, 1)
    assert g.digest() == digest


# ------------------------------------------------------------------ far offsets

FAR_N = (1 << 32) + (1 << 20)


def test_far_offsets(ctx):
    """reads, and separately the unitig list, whose last element lies past 2^32 bytes of one device buffer"""
    k, canonical = 31, True
    seqs = _input(k)
    G = _graph(k, canonical, 1)
    g = _job(ctx, seqs, k, canonical)
    udata, ustart, ulength, _ = ur.layout(G.units)
    g.unitig_index(udata, ustart, ulength, 1)
    reads = [s for s, _ in seqs[:6]] + [ur.rc(seqs[0][0])]
    data, start, length = hr.read_codes(reads)
    w_ptr, w_hits = G.hit_rows(reads)
    d_big = ctx.alloc(FAR_N)
    fill = np.full(1 << 26, -1, np.int8)
    try:
        # the reads: the first half at the buffer's beginning, the rest behind 2^31 and 2^32 (what lies between is never read)
        half = len(reads) // 2
        cut = int(start[half])
        far_start = start.copy()
        far_start[half:] += (1 << 31) + 5 - cut
        far_start[-1] = FAR_N - int(length[-1]) - 1
        assert far_start[-1] > 1 << 32
        ctx.h2d(d_big, data[:cut])
        ctx.h2d(d_big + int(far_start[half]), data[cut:int(start[-1])])
        ctx.h2d(d_big + int(far_start[-1]), data[int(start[-1]):])
        d_s, d_l = _upload(ctx, far_start), _upload(ctx, length)
        d_ptr, d_hits = _Guarded(ctx, (len(reads) + 1) * 8), _Guarded(ctx, len(w_hits) * 16)
        assert g.read_hits_device(d_big, d_s, d_l, FAR_N, len(reads), d_ptr.ptr, d_hits.ptr, len(w_hits)) == len(w_hits)
        ctx.sync()
        _same(d_ptr.fetch((len(reads) + 1) * 8, np.int64), w_ptr, "hit_ptr of far reads")
        _same(d_hits.fetch(len(w_hits) * 16, hr.READ_HIT_DTYPE), w_hits, "hits of far reads")
        for p in (d_s, d_l):
            ctx.free(p)
        d_ptr.free()
        d_hits.free()
        # the unitig list: terminators everywhere, the unitigs' first half at the beginning, the rest behind 2^31 and 2^32
        for a in range(0, FAR_N, len(fill)):
            ctx.h2d(d_big + a, fill[:min(len(fill), FAR_N - a)])
        half = len(ustart) // 2
        cut = int(ustart[half])
        far_u = ustart.copy()
        far_u[half:] += (1 << 31) + 7 - cut
        far_u[-1] = FAR_N - int(ulength[-1]) - 1
        ctx.h2d(d_big, udata[:cut])
        ctx.h2d(d_big + int(far_u[half]), udata[cut:int(ustart[-1])])
        ctx.h2d(d_big + int(far_u[-1]), udata[int(ustart[-1]):])
        d_s, d_l = _upload(ctx, far_u), _upload(ctx, ulength)
        g.unitig_index_device(1, d_big, d_s, d_l, FAR_N, len(far_u))
        kmers = sorted(G.solid)
        _same(g.locate(*_keys(kmers)), G.locate_rows(kmers), "locate after the far list")
        for p in (d_s, d_l):
            ctx.free(p)
    finally:
        ctx.free(d_big)


# ------------------------------------------------------------------ CLI

@pytest.mark.parametrize("k,canonical,min_count,fastq,gfa", [(21, True, 1, True, False), (31, True, 2, False, True), (5, False, 1, False, False)])
def test_cli_unitigs_map(tmp_path, k, canonical, min_count, fastq, gfa):
    seqs = _input(k)
    fasta = tmp_path / "in.fa"
    with open(fasta, "w") as f:
        i = 0
        for s, t in seqs:
            for _ in range(t):
                f.write(">r%d\n%s\n" % (i, s))
                i += 1
    G = _graph(k, canonical, min_count)
    reads = [s for s, _ in seqs] + [ur.rc(s) for s, _ in seqs[:10]] + ["ACGT"[:min(k - 1, 4)]]
    q = tmp_path / ("q.fq" if fastq else "q.fa")
    with open(q, "w") as f:
        for i, s in enumerate(reads):
            f.write("@q%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) if fastq else ">q%d\n%s\n" % (i, s))
    tail = [str(k), "--global"] + (["--canonical"] if canonical else [])
    subprocess.run([_cli(), str(fasta), str(tmp_path / "a.out")] + tail, check=True, timeout=300)
    extra = ["--unitigs-map", str(q), "--unitigs-map-out", str(tmp_path / "m.gaf"), "--unitigs-min-count", str(min_count)]
    if gfa:
        extra += ["--unitigs-gfa", str(tmp_path / "g.gfa")]
    subprocess.run([_cli(), str(fasta), str(tmp_path / "b.out")] + tail + extra, check=True, timeout=300)
    assert open(tmp_path / "m.gaf", "rb").read() == G.gaf_text(reads)
    assert open(tmp_path / "a.out", "rb").read() == open(tmp_path / "b.out", "rb").read()
    if gfa:
        text = open(tmp_path / "g.gfa", "rb").read()
        assert text.count(b"\nS\t") == len(G.units)
