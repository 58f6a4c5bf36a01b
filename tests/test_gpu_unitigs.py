"""GPU: neighbour masks and unitigs of a finished global result (cfrk_global_neighbors / _unitigs and their device
forms) against tests/unitig_ref.py, a dictionary-and-strings statement of the contract that shares nothing with the
product: a k grid on both strand rules and two thresholds over an input with branches, tips, bubbles, circles, repeats,
hairpins, palindromes and a homopolymer; every splitter period that forces multi-segment stitching, rings of segments
and splitter-free rings at tiny sizes; the k = 32 all-T key; crafted hash collisions; a 300 000-node chain and ring
against numpy; the recount property; the capacity protocol; the CLI."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from . import hash_craft as hc
from . import oracle_lib as orc
from . import unitig_ref as ur
from .test_gpu_filter import _Guarded
from .test_gpu_query import _cli

pytestmark = pytest.mark.gpu

CFRK_ERR_ARG, CFRK_ERR_STATE, CFRK_ERR_SMALL_BUF = -1, -4, -9
COUNT_MAX = 0xFFFFFFFE
KS = [3, 4, 12, 13, 16, 21, 31, 32, 33, 47, 64]
NEIGHBOR_KS = [3, 4, 12, 13, 21, 32, 33, 64]


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


def _rand(rng, n):
    return "".join(ur.BASES[i] for i in rng.integers(0, 4, n))


_INPUTS = {}


def _input(k):
    """[(string, times counted)]: a random genome of 3000 bases counted twice and 40 error reads counted once (min_count
    1: branches, tips, bubbles; 2: one chain), and, counted twice, circles of k + 1, 2k and 700 k-mers, a period-2 and a
    period-3 repeat, hairpins h + rc(h), even-k palindromes and a homopolymer run"""
    if k in _INPUTS:
        return _INPUTS[k]
    rng = np.random.default_rng(4200 + k)
    genome = _rand(rng, 3000)
    seqs = [(genome, 2)]
    for _ in range(40):
        a = int(rng.integers(0, len(genome) - 100))
        r = list(genome[a:a + 100])
        p = int(rng.integers(0, 100))
        r[p] = ur.BASES[(ur.BASES.index(r[p]) + int(rng.integers(1, 4))) % 4]
        seqs.append(("".join(r), 1))
    for n in (k + 1, 2 * k, 700):
        c = _rand(rng, n)
        seqs.append((c + c[:k - 1], 2))
    seqs.append(("AC" * (k + 4), 2))
    seqs.append(("ACG" * (k + 4), 2))
    for n in (k, k + 7):
        h = _rand(rng, n)
        seqs.append((h + ur.rc(h), 2))
    if k % 2 == 0:
        for _ in range(2):
            h = _rand(rng, k // 2)
            seqs.append((_rand(rng, 20) + h + ur.rc(h) + _rand(rng, 20), 2))
    seqs.append((_rand(rng, 15) + "A" * (k + 10) + _rand(rng, 15), 2))
    _INPUTS[k] = seqs
    return seqs


def _reads(seqs):
    """[(string, times)] -> (data, start, length) in the struct-read layout, every string `times` times"""
    data, start, length = [], [], []
    for s, t in seqs:
        for _ in range(t):
            start.append(len(data))
            length.append(len(s))
            data.extend(ur.BASES.index(c) for c in s)
            data.append(-1)
    return np.array(data, np.int8), np.array(start, np.int64), np.array(length, np.int32)


def _table(seqs, k, canonical):
    table = {}
    for s, t in seqs:
        ur.count_kmers([s], k, canonical, t, table)
    return table


def _job(ctx, seqs, k, canonical, hint=0):
    import cfrk_amd
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL if canonical else 0, hint or 200000)
    g.add(*_reads(seqs))
    return g


def _device_unitigs(ctx, g, min_count, skew=0):
    """the device form with exact capacities after a sizes-only call -> (data, start, length, rec)"""
    import cfrk_amd
    with pytest.raises(cfrk_amd.CfrkError) as e:
        g.unitigs_device(min_count, 0, 0, 0, 0, 0, 0)
    assert e.value.code == CFRK_ERR_SMALL_BUF
    nN, nS = e.value.nN, e.value.nS
    bufs = [_Guarded(ctx, nN, skew), _Guarded(ctx, nS * 8), _Guarded(ctx, nS * 4), _Guarded(ctx, nS * 16)]
    assert g.unitigs_device(min_count, bufs[0].ptr, nN, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, nS) == (nN, nS)
    ctx.sync()
    out = (bufs[0].fetch(nN, np.int8), bufs[1].fetch(nS * 8, np.int64), bufs[2].fetch(nS * 4, np.int32),
           bufs[3].fetch(nS * 16, cfrk_amd.UNITIG_DTYPE))
    for b in bufs:
        b.free()
    return out


def _same(got, want):
    for name, a, b in zip(("data", "start", "length", "rec"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.shape, b.shape)
        assert (a == b).all(), name


_REF = {}


def _ref(k, canonical, min_count):
    key = (k, canonical, min_count)
    if key not in _REF:
        _REF[key] = ur.layout(ur.unitigs(_table(_input(k), k, canonical), k, canonical, min_count))
    return _REF[key]


# ------------------------------------------------------------------ neighbour masks

@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", NEIGHBOR_KS)
def test_neighbors(ctx, k, canonical):
    seqs = _input(k)
    table = _table(seqs, k, canonical)
    g = _job(ctx, seqs, k, canonical)
    rng = np.random.default_rng(k)
    present = sorted(table)
    if canonical:                                               # both orientations are asked, exactly as given
        present = present + [ur.rc(x) for x in present[::3]]
    absent = [_rand(rng, k) for _ in range(300)]
    keys = present + absent
    lo = np.array([ur.key_of(x)[0] for x in keys], np.uint64)
    hi = np.array([ur.key_of(x)[1] for x in keys], np.uint64)
    for min_count in (1, 2):
        want = np.array([ur.neighbor_mask(table, x, k, canonical, min_count) for x in keys], np.uint8)
        got = g.neighbors(lo, hi, min_count)
        assert (got == want).all()
        if min_count == 1:
            assert (g.neighbors(lo, hi, 0) == want).all()        # 0 reads as 1
    if k <= 32:
        assert (g.neighbors(lo, None, 1) == g.neighbors(lo, hi, 1)).all()
    # bits at or above 2k: no such k-mer
    if k < 32:
        bad_lo, bad_hi = lo[:50] | np.uint64(1 << (2 * k)), hi[:50]
    elif k == 32:
        bad_lo, bad_hi = lo[:50], hi[:50] | np.uint64(1)
    elif k < 64:
        bad_lo, bad_hi = lo[:50], hi[:50] | np.uint64(1 << (2 * k - 64))
    else:
        bad_lo = None
    if bad_lo is not None:
        assert (g.neighbors(bad_lo, bad_hi, 1) == 0).all()
    # device form
    n = len(keys)
    d_lo, d_hi, d_out = ctx.alloc(n * 8), ctx.alloc(n * 8), _Guarded(ctx, n, 3)
    ctx.h2d(d_lo, lo)
    ctx.h2d(d_hi, hi)
    g.neighbors_device(d_lo, d_hi, n, 2, d_out.ptr)
    ctx.sync()
    assert (d_out.fetch(n) == np.array([ur.neighbor_mask(table, x, k, canonical, 2) for x in keys], np.uint8)).all()
    for p in (d_lo, d_hi):
        ctx.free(p)
    d_out.free()


# ------------------------------------------------------------------ unitigs against the reference

@pytest.mark.parametrize("min_count", [1, 2])
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", KS)
def test_unitigs(ctx, k, canonical, min_count):
    want = _ref(k, canonical, min_count)
    g = _job(ctx, _input(k), k, canonical)
    digest = g.digest()
    _same(g.unitigs(min_count), want)
    _same(_device_unitigs(ctx, g, min_count), want)
    assert g.digest() == digest


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [4, 13, 31, 33])
def test_unitigs_splitter_period(ctx, k, canonical):
    """s = 0 (every node a splitter), 1, 2, 4 and the default give the same bytes: multi-segment stitching, rings of
    segments and, from s = 2 on, rings without a splitter (the circles of k + 1 and 2k k-mers)"""
    import cfrk_amd
    g = _job(ctx, _input(k), k, canonical)
    try:
        for s in (0, 1, 2, 4, None):
            g.set_debug_param(cfrk_amd.CFRK_PARAM_UNITIG_SPLIT_LOG2, 0 if s is None else s + 1)
            for min_count in (1, 2):
                _same(g.unitigs(min_count), _ref(k, canonical, min_count))
    finally:
        g.set_debug_param(cfrk_amd.CFRK_PARAM_UNITIG_SPLIT_LOG2, 0)


def test_unitigs_k32_all_t(ctx):
    """the all-T key (the table's side word) as a node with neighbours, on the strand as given"""
    rng = np.random.default_rng(32)
    seqs = [(_rand(rng, 50) + "T" * 45 + _rand(rng, 50), 2), ("G" + "T" * 32 + "C", 1), (_rand(rng, 200), 1)]
    table = _table(seqs, 32, False)
    assert "T" * 32 in table
    g = _job(ctx, seqs, 32, False)
    keys = sorted(table)
    lo = np.array([ur.key_of(x)[0] for x in keys], np.uint64)
    want = np.array([ur.neighbor_mask(table, x, 32, False, 1) for x in keys], np.uint8)
    assert (g.neighbors(lo) == want).all()
    for min_count in (1, 2):
        _same(g.unitigs(min_count), ur.layout(ur.unitigs(table, 32, False, min_count)))


@pytest.mark.parametrize("k", [21, 33])
def test_unitigs_crafted_collisions(ctx, k):
    """a chain in an index of 1024 slots beside 300 keys crafted to home on the slot of one of its nodes and on the last
    slot, through the wrap: the slot-returning probes run long"""
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
    assert len(table) <= 512
    g = _job(ctx, seqs, k, True)
    _same(g.unitigs(1), ur.layout(ur.unitigs(table, k, True, 1)))
    assert g.hash_geometry()[1] == 10
    keys = sorted(table)
    lo = np.array([ur.key_of(x)[0] for x in keys], np.uint64)
    hi = np.array([ur.key_of(x)[1] for x in keys], np.uint64)
    assert (g.neighbors(lo, hi) == np.array([ur.neighbor_mask(table, x, k, True, 1) for x in keys], np.uint8)).all()


# ------------------------------------------------------------------ a long chain and a long ring, against numpy

def _kmers31(codes):
    """the 31-mer starting at every position of a code array, as uint64"""
    n = len(codes) - 30
    v = np.zeros(n, np.uint64)
    for j in range(31):
        v = (v << np.uint64(2)) | codes[j:j + n].astype(np.uint64)
    return v


@pytest.fixture(scope="module")
def long_genome():
    return np.random.default_rng(31).integers(0, 4, 300000).astype(np.int8)


def test_long_chain(ctx, long_genome):
    import cfrk_amd
    G = long_genome
    R = (3 - G[::-1]).astype(np.int8)
    n = len(G) - 30
    assert len(np.unique(np.minimum(_kmers31(G), _kmers31(R)[::-1]))) == n      # every node once: one chain
    g = cfrk_amd.GlobalCounter(ctx, 31, cfrk_amd.CFRK_CANONICAL, 400000)
    g.add(np.append(G, np.int8(-1)))
    data, start, length, rec = g.unitigs(1)
    want = G if _kmers31(G[:31])[0] < _kmers31(R[:31])[0] else R               # a1 < rc(an)
    assert list(start) == [0] and list(length) == [len(G)]
    assert (data == np.append(want, np.int8(-1))).all()
    assert rec.tolist() == [(n, n, 0)]


def test_long_ring(ctx, long_genome):
    import cfrk_amd
    G = long_genome
    n = len(G)
    R = (3 - G[::-1]).astype(np.int8)
    fwd, rev = _kmers31(np.append(G, G[:30])), _kmers31(np.append(R, R[:30]))
    assert len(np.unique(np.concatenate([fwd, rev]))) == 2 * n                   # one ring and its distinct mirror
    ring, v = (G, fwd) if fwd.min() < rev.min() else (R, rev)
    p = int(v.argmin())                                                          # cut at the smallest oriented k-mer
    want = np.concatenate([ring[p:], ring[:p], np.roll(ring, -p)[:30], [np.int8(-1)]]).astype(np.int8)
    g = cfrk_amd.GlobalCounter(ctx, 31, cfrk_amd.CFRK_CANONICAL, 400000)
    g.add(np.concatenate([G, G[:30], [np.int8(-1)]]).astype(np.int8))
    data, start, length, rec = g.unitigs(1)
    assert list(start) == [0] and list(length) == [n + 30]
    assert (data == want).all()
    assert rec.tolist() == [(n, n, cfrk_amd.CFRK_UNITIG_CIRCULAR)]


# ------------------------------------------------------------------ recount

def test_unitigs_recount(ctx):
    """the unitigs of the keys counted twice or more, fed to a fresh job on the device, hold exactly those keys, once each"""
    import cfrk_amd
    data, start, length = orc.synth_reads(7, 20000, 100, 150000)
    g = cfrk_amd.GlobalCounter(ctx, 31, cfrk_amd.CFRK_CANONICAL, 2000000)
    g.add(data, start, length)
    wlo, _, wcnt = g.export_range(2, COUNT_MAX, g.finish())
    assert len(wlo) > 10000
    with pytest.raises(cfrk_amd.CfrkError) as e:
        g.unitigs_device(2, 0, 0, 0, 0, 0, 0)
    nN, nS = e.value.nN, e.value.nS
    assert nS <= len(wlo) and nN <= len(wlo) * 32
    d = [ctx.alloc(nN + 64), ctx.alloc(nS * 8 + 8), ctx.alloc(nS * 4 + 8), ctx.alloc(nS * 16 + 16)]
    assert g.unitigs_device(2, d[0], nN, d[1], d[2], d[3], nS) == (nN, nS)
    rec = np.zeros(nS, cfrk_amd.UNITIG_DTYPE)
    ctx.d2h(rec, d[3])
    assert int(rec["n_kmers"].sum()) == len(wlo) and int(rec["kc"].sum()) == int(wcnt.astype(np.uint64).sum())
    g2 = cfrk_amd.GlobalCounter(ctx, 31, cfrk_amd.CFRK_CANONICAL, 2000000)
    g2.add_device(d[0], nN)
    lo, _, cnt = g2.export()
    assert len(lo) == len(wlo) and (lo == wlo).all() and (cnt == 1).all()
    for p in d:
        ctx.free(p)


# ------------------------------------------------------------------ protocol

def test_unitigs_protocol(ctx):
    import cfrk_amd
    k, canonical, min_count = 21, True, 1
    want = _ref(k, canonical, min_count)
    nN, nS = len(want[0]), len(want[1])
    g = _job(ctx, _input(k), k, canonical)
    digest = g.digest()
    L, h = ctx._L, ctx._h
    a, b = C.c_int64(-1), C.c_int64(-1)
    # sizes only, host and device form
    assert L.cfrk_global_unitigs(h, min_count, None, 0, None, None, None, 0, C.byref(a), C.byref(b)) == CFRK_ERR_SMALL_BUF
    assert (a.value, b.value) == (nN, nS)
    for short_data, short_recs in ((1, 0), (0, 1)):
        bufs = [_Guarded(ctx, nN - short_data, 1), _Guarded(ctx, (nS - short_recs) * 8), _Guarded(ctx, (nS - short_recs) * 4),
                _Guarded(ctx, (nS - short_recs) * 16)]
        with pytest.raises(cfrk_amd.CfrkError) as e:
            g.unitigs_device(min_count, bufs[0].ptr, nN - short_data, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, nS - short_recs)
        assert e.value.code == CFRK_ERR_SMALL_BUF and (e.value.nN, e.value.nS) == (nN, nS)
        ctx.sync()
        for x in bufs:
            x.fetch(0)                                          # nothing written: every byte is still a guard byte
            x.free()
        host = [np.full(nN - short_data, 0x5A, np.int8), np.full(nS - short_recs, 0x5A5A, np.int64),
                np.full(nS - short_recs, 0x5A5A, np.int32), np.zeros(nS - short_recs, cfrk_amd.UNITIG_DTYPE)]
        rc = L.cfrk_global_unitigs(h, min_count, host[0].ctypes.data_as(C.c_void_p), host[0].size, host[1].ctypes.data_as(C.c_void_p),
                                   host[2].ctypes.data_as(C.c_void_p), host[3].ctypes.data_as(C.c_void_p), host[3].size,
                                   C.byref(a), C.byref(b))
        assert rc == CFRK_ERR_SMALL_BUF and (a.value, b.value) == (nN, nS)
        assert (host[0] == 0x5A).all() and (host[1] == 0x5A5A).all() and (host[2] == 0x5A5A).all() and (host[3]["kc"] == 0).all()
    # exact capacities, the data at every offset from a 16-byte boundary that matters (odd included)
    for skew in (0, 1, 7):
        _same(_device_unitigs(ctx, g, min_count, skew), want)
    assert g.digest() == digest
    # NULL size outputs, a NULL array with a capacity
    assert L.cfrk_global_unitigs(h, 1, None, 0, None, None, None, 0, None, C.byref(b)) == CFRK_ERR_ARG
    assert L.cfrk_global_unitigs_device(h, 1, None, 0, None, None, None, 0, C.byref(a), None) == CFRK_ERR_ARG
    assert L.cfrk_global_unitigs_device(h, 1, None, 8, None, None, None, 0, C.byref(a), C.byref(b)) == CFRK_ERR_ARG
    assert L.cfrk_global_unitigs(h, 1, None, 0, None, None, None, 4, C.byref(a), C.byref(b)) == CFRK_ERR_ARG
    # a threshold nothing reaches, and a job without reads: the empty result
    data, start, length, rec = g.unitigs(COUNT_MAX)
    assert len(data) == 0 and len(start) == 0 and len(length) == 0 and len(rec) == 0
    assert g.unitigs_device(COUNT_MAX, 0, 0, 0, 0, 0, 0) == (0, 0)
    for kk in (5, 31, 40):
        e = cfrk_amd.GlobalCounter(ctx, kk, 0, 1000)
        assert e.unitigs_device(1, 0, 0, 0, 0, 0, 0) == (0, 0)
        assert len(e.neighbors(np.zeros(3, np.uint64), np.zeros(3, np.uint64))) == 3


def test_unitigs_need_a_job():
    import cfrk_amd
    with cfrk_amd.Context(0) as c:
        a, b = C.c_int64(), C.c_int64()
        assert c._L.cfrk_global_unitigs_device(c._h, 1, None, 0, None, None, None, 0, C.byref(a), C.byref(b)) == CFRK_ERR_STATE
        assert c._L.cfrk_global_unitigs(c._h, 1, None, 0, None, None, None, 0, C.byref(a), C.byref(b)) == CFRK_ERR_STATE
        m = np.zeros(1, np.uint8)
        z = np.zeros(1, np.uint64)
        assert c._L.cfrk_global_neighbors(c._h, z.ctypes.data_as(C.c_void_p), None, 1, 1, m.ctypes.data_as(C.c_void_p)) == CFRK_ERR_STATE


# ------------------------------------------------------------------ CLI

@pytest.mark.parametrize("k,canonical,min_count", [(5, False, 1), (21, True, 1), (31, True, 2), (40, False, 2)])
def test_cli_unitigs(tmp_path, k, canonical, min_count):
    seqs = _input(k)
    fasta = tmp_path / "in.fa"
    with open(fasta, "w") as f:
        i = 0
        for s, t in seqs:
            for _ in range(t):
                f.write(">r%d\n%s\n" % (i, s))
                i += 1
    want = ur.fasta_text(ur.unitigs(_table(seqs, k, canonical), k, canonical, min_count))
    tail = [str(k), "--global"] + (["--canonical"] if canonical else [])
    subprocess.run([_cli(), str(fasta), str(tmp_path / "a.out")] + tail, check=True, timeout=300)
    subprocess.run([_cli(), str(fasta), str(tmp_path / "b.out")] + tail + ["--unitigs-out", str(tmp_path / "u.fa"),
                                                                         "--unitigs-min-count", str(min_count)], check=True, timeout=300)
    assert open(tmp_path / "u.fa", "rb").read() == want
    assert open(tmp_path / "a.out", "rb").read() == open(tmp_path / "b.out", "rb").read()
