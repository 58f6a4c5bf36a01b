"""GPU: point queries on a finished global result (cfrk_global_query / _device, cfrk_global_query_reads / _device)
against the oracle on every counting path, the index's life cycle, a full-size invariant, and the CLI's --query /
--query-out / --query-only / --query-db.  References are numpy searchsorted over tests.oracle_lib.global_count."""
import os
import subprocess

import numpy as np
import pytest

from . import oracle_lib as orc
from . import refsem

pytestmark = pytest.mark.gpu

CFRK_ERR_ARG, CFRK_ERR_STATE, CFRK_ERR_ALIGN = -1, -4, -7
NONE = 0xFFFFFFFF
KS = [1, 2, 5, 7, 8, 12, 13, 15, 16, 17, 21, 26, 27, 31, 32, 33, 40, 47, 48, 55, 63, 64]
U2 = np.uint64(2)


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


def _random_reads(rng, n, lo, hi, p_invalid=0.02):
    reads = []
    for L in rng.integers(lo, hi, n):
        r = rng.integers(0, 4, int(L)).astype(np.int8)
        if p_invalid:
            r[rng.random(int(L)) < p_invalid] = -1
        reads.append(r)
    return reads


def _grid_reads(k):
    rng = np.random.default_rng(700 + k)
    reads = _random_reads(rng, 300, 1, 300)
    genome = rng.integers(0, 4, 3000).astype(np.int8)          # repeats: counts above 1
    for _ in range(200):
        a = int(rng.integers(0, len(genome) - 150))
        reads.append(genome[a:a + 150].copy())
    reads.append(np.full(200, 3, np.int8))                      # poly-T: the all-ones key at k = 32
    reads.append(np.full(200, 0, np.int8))                      # poly-A
    reads.append(np.zeros(0, np.int8))                          # empty read
    reads.append(np.array([0, 1, 2], np.int8))                  # shorter than most k
    return refsem.flatten(reads)


def _oracle(data, k, canonical):
    return orc.global_count(data, k, orc.ORC_CANONICAL if canonical else 0)


_DT = np.dtype([("hi", "<u8"), ("lo", "<u8")])


def _lookup(want, qlo, qhi):
    """oracle count of each (hi, lo) query key (already canonical), 0 when absent"""
    wlo, whi, wcnt = want
    ref = np.zeros(len(wlo), _DT)
    ref["hi"], ref["lo"] = whi, wlo                             # (sorted by (hi, lo))
    q = np.zeros(len(qlo), _DT)
    q["hi"], q["lo"] = qhi, qlo
    i = np.searchsorted(ref, q)
    ic = np.minimum(i, max(len(ref) - 1, 0))
    hit = (i < len(ref)) & (ref[ic] == q) if len(ref) else np.zeros(len(q), bool)
    c = np.where(hit, wcnt[ic] if len(ref) else 0, 0)
    return np.minimum(c, 0xFFFFFFFE).astype(np.uint32)


def _split(x, k):
    """python int keys -> (lo, hi) uint64 arrays"""
    return (np.array([v & ((1 << 64) - 1) for v in x], np.uint64), np.array([v >> 64 for v in x], np.uint64))


def _rc(x, k):
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (x & 3))
        x >>= 2
    return r


def _windows(data, k, canonical):
    """numpy restatement of the read query's windows -> (lo, hi, valid) per start position"""
    n = len(data)
    d = data.astype(np.int64)
    bad = (d < 0) | (d > 3)
    c = np.where(bad, 0, d).astype(np.uint64)
    m = max(n - k + 1, 0)
    lo = np.zeros(n, np.uint64)
    hi = np.zeros(n, np.uint64)
    valid = np.zeros(n, bool)
    if m == 0:
        return lo, hi, valid
    cs = np.concatenate([[0], np.cumsum(bad)])
    valid[:m] = (cs[k:k + m] - cs[:m]) == 0

    def pack(codes, idx):
        v = np.zeros(m, np.uint64)
        for j in idx:
            v = (v << U2) | codes[j:j + m]
        return v

    nl = min(k, 32)
    flo, fhi = pack(c, range(k - nl, k)), pack(c, range(0, k - nl))
    if canonical:
        r = np.uint64(3) - c                                     # rc base j of window p = 3 - c[p + k - 1 - j]
        rlo = pack(r, [k - 1 - j for j in range(k - nl, k)])
        rhi = pack(r, [k - 1 - j for j in range(0, k - nl)])
        take = (rhi < fhi) | ((rhi == fhi) & (rlo < flo))
        flo, fhi = np.where(take, rlo, flo), np.where(take, rhi, fhi)
    lo[:m], hi[:m] = flo, fhi
    return lo, hi, valid


def _want_reads(data, k, canonical, want):
    lo, hi, valid = _windows(data, k, canonical)
    return np.where(valid, _lookup(want, lo, hi), np.uint32(NONE)).astype(np.uint32)


def _check_keys(g, want, k, canonical, rng):
    wlo, whi, wcnt = want
    two = k > 32
    full = (1 << (2 * k)) - 1
    # every result key
    got = g.query(wlo, whi if two else None)
    assert (got == np.minimum(wcnt, 0xFFFFFFFE).astype(np.uint32)).all()
    # random keys (mostly absent), the all-A / all-T keys, reverse complements of present keys
    keys = [int(x) for x in rng.integers(0, 1 << 62, 500, dtype=np.uint64)]
    if two:
        keys = [(x << 64 | int(y)) & full for x, y in zip(keys, rng.integers(0, 1 << 62, 500, dtype=np.uint64))]
    else:
        keys = [x & full for x in keys]
    keys += [0, full]
    present = [int(h) << 64 | int(l) for l, h in zip(wlo[:300], whi[:300])]
    keys += [_rc(x, k) for x in present]
    canon = [min(x, _rc(x, k)) if canonical else x for x in keys]
    qlo, qhi = _split(keys, k)
    clo, chi = _split(canon, k)
    got = g.query(qlo, qhi if two or rng.random() < 0.5 else None)
    assert (got == _lookup(want, clo, chi)).all()
    if canonical:
        assert (got[-len(present):] == np.minimum(wcnt[:300], 0xFFFFFFFE).astype(np.uint32)).all()
    # out of range: bits at or above 2k
    if k < 64:
        olo, ohi = _split([x | (1 << (2 * k + int(s))) for x, s in zip(keys[:50], rng.integers(0, 128 - 2 * k, 50))], k)
        assert (g.query(olo, ohi) == 0).all()
    if k <= 32:
        assert (g.query(wlo[:50], np.ones(min(50, len(wlo)), np.uint64)) == 0).all()


def _check_reads(g, data, start, length, k, canonical, want):
    got = g.query_reads(data, start, length)
    assert got.dtype == np.uint32 and len(got) == len(data)
    exp = _want_reads(data, k, canonical, want)
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, (k, bad[:10], got[bad[:10]], exp[bad[:10]])


def _check_job(g, data, k, canonical, start=None, length=None, seed=0):
    want = _oracle(data, k, canonical)
    _check_keys(g, want, k, canonical, np.random.default_rng(seed + k))
    _check_reads(g, data, start, length, k, canonical, want)
    return want


# ------------------------------------------------------------------ keys and reads on the k grid

@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("force_hash", [False, True])
def test_query_keys_vs_oracle(ctx, k, canonical, force_hash):
    import cfrk_amd
    data, start, length = _grid_reads(k)
    flags = (cfrk_amd.CFRK_CANONICAL if canonical else 0) | (cfrk_amd.CFRK_FORCE_HASH if force_hash else 0)
    g = cfrk_amd.GlobalCounter(ctx, k, flags, 0)
    g.add(data, start, length)
    want = _oracle(data, k, canonical)
    _check_keys(g, want, k, canonical, np.random.default_rng(k))
    assert g.digest() == orc.digest(*want, two_word=k > 32)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("force_hash", [False, True])
def test_query_reads_vs_oracle(ctx, k, canonical, force_hash):
    import cfrk_amd
    data, start, length = _grid_reads(k)
    flags = (cfrk_amd.CFRK_CANONICAL if canonical else 0) | (cfrk_amd.CFRK_FORCE_HASH if force_hash else 0)
    g = cfrk_amd.GlobalCounter(ctx, k, flags, 0)
    g.add(data, start, length)
    want = _oracle(data, k, canonical)
    _check_reads(g, data, start, length, k, canonical, want)
    # other reads than the counted ones, without a layout; a length that is no multiple of the tile
    rng = np.random.default_rng(900 + k)
    other, _, _ = refsem.flatten(_random_reads(rng, 40, 1, 200, 0.05))
    _check_reads(g, other[:len(other) - 3], None, None, k, canonical, want)


# ------------------------------------------------------------------ every counting path

def test_query_k16_partitioned(ctx):
    import cfrk_amd
    rng = np.random.default_rng(16)
    reads = _random_reads(rng, 3000, 1, 300)
    reads.append(np.full(200, 0, np.int8))
    data, start, length = refsem.flatten(reads)
    g = cfrk_amd.GlobalCounter(ctx, 16, cfrk_amd.CFRK_CANONICAL, 1 << 20)
    g.set_debug_flags(cfrk_amd.CFRK_DEBUG_NO_RADIX16)
    try:
        g.add(data, start, length)
        assert g.msp_info()["l2_records"] > 0
        _check_job(g, data, 16, True, start, length)
    finally:
        g.set_debug_flags(0)


@pytest.mark.parametrize("k", [40, 63])
def test_query_two_word_shared_leaves(ctx, k):
    import cfrk_amd
    data, _, _ = orc.synth_reads(0, 20000, 150, 200_000)
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, 400_000)
    g.set_debug_flags(cfrk_amd.lib.CFRK_DEBUG_RECORD_SUBSETS)
    try:
        g.add(data)
    finally:
        g.set_debug_flags(0)
    _check_job(g, data, k, True)


@pytest.mark.parametrize("k", [25, 47])
def test_query_chunked_add(ctx, k):
    import cfrk_amd
    rng = np.random.default_rng(950 + k)
    reads = _random_reads(rng, 2500, 1, 500, 0.01)
    genome = rng.integers(0, 4, 20000).astype(np.int8)
    for _ in range(2000):
        a = int(rng.integers(0, len(genome) - 250))
        reads.append(genome[a:a + 250].copy())
    data, start, length = refsem.flatten(reads)
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, 0)
    g.set_debug_flags(cfrk_amd.CFRK_DEBUG_SMALL_PIPELINE)
    try:
        g.add(data, start, length)
    finally:
        g.set_debug_flags(0)
    _check_job(g, data, k, True, start, length)


def test_query_multi_pass_add(ctx):
    import cfrk_amd
    data, _, _ = orc.synth_reads(0, 200_000, 150, 300_000)
    d = ctx.alloc(len(data))
    ctx.h2d(d, data)
    try:
        budget = 6 << 30
        while True:
            g = cfrk_amd.GlobalCounter(ctx, 31, cfrk_amd.CFRK_CANONICAL, 400_000)
            g.set_mem_budget(budget)
            g.add_device(d, len(data))
            if g.last_add_passes() != 1:
                break
            budget = budget * 15 // 16
        g.set_mem_budget(0)
    finally:
        ctx.sync()
        ctx.free(d)
    _check_job(g, data, 31, True)


@pytest.mark.parametrize("k", [13, 31, 32, 63])
def test_query_after_two_adds(ctx, k):
    import cfrk_amd
    d1, _, _ = orc.synth_reads(0, 4000, 150, 30000)
    d2, _, _ = orc.synth_reads(4000, 4000, 150, 30000)
    g = cfrk_amd.GlobalCounter(ctx, k, 0, 100000)
    g.add(d1)
    g.add(d2)
    _check_job(g, np.concatenate([d1, d2]), k, False)


@pytest.mark.parametrize("k", [31, 63])
def test_query_merged_job(ctx, k):
    import cfrk_amd
    data, _, _ = orc.synth_reads(0, 3000, 150, 20000)
    wlo, whi, wcnt = _oracle(data, k, True)
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, 100000)
    cnt32 = wcnt.astype(np.uint32)
    d_lo, d_hi, d_cnt = ctx.alloc(wlo.nbytes), ctx.alloc(whi.nbytes), ctx.alloc(cnt32.nbytes)
    try:
        ctx.h2d(d_lo, wlo); ctx.h2d(d_hi, whi); ctx.h2d(d_cnt, cnt32)
        g.merge_device(d_lo, d_hi if k > 32 else 0, d_cnt, len(wlo))
        ctx.sync()
    finally:
        ctx.free(d_lo); ctx.free(d_hi); ctx.free(d_cnt)
    _check_job(g, data, k, True)


@pytest.mark.parametrize("k", [31, 63])
def test_query_pipelined_owner(ctx, k):
    """two emulated ranks through the pipelined runs exchange; each owner's answers are its key subset's counts: the
    owners' answers add to the oracle's"""
    import cfrk_amd
    R, L, world, ngroups, seg_cap = 6000, 150, 2, 2, 1 << 18
    data, _, _ = orc.synth_reads(0, R, L, 300_000)
    flags = cfrk_amd.CFRK_CANONICAL
    per_rank = []
    for r in range(world):
        shard = np.ascontiguousarray(data[R * r // world * (L + 1):R * (r + 1) // world * (L + 1)])
        g = cfrk_amd.GlobalCounter(ctx, k, flags | cfrk_amd.CFRK_RUNS_ONLY | cfrk_amd.CFRK_RUNS_DEFER, 300_000)
        g.add(shard)
        d = ctx.alloc(ngroups * world * seg_cap * 16)
        g.export_runs_async(d, seg_cap, world, ngroups)
        groups = []
        for gi in range(ngroups):
            rows = g.export_runs_wait(gi)
            host = np.empty((world * seg_cap, 2), np.uint64)
            ctx.d2h(host, d + gi * world * seg_cap * 16)
            groups.append((rows, host))
        ctx.sync()
        ctx.free(d)
        per_rank.append(groups)
    want = _oracle(data, k, True)
    reads_sum = np.zeros(len(data), np.uint64)
    keys_sum = np.zeros(len(want[0]), np.uint64)
    for owner in range(world):
        og = cfrk_amd.GlobalCounter(ctx, k, flags, 300_000)
        bufs = []
        for gi in range(ngroups):
            segs, recv = [], []
            for r in range(world):
                rows, host = per_rank[r][gi]
                segs.append(host[owner * seg_cap:owner * seg_cap + rows[owner]])
                recv.append(rows[owner])
            buf = np.concatenate(segs)
            d = ctx.alloc(len(buf) * 16)
            ctx.h2d(d, buf)
            og.merge_runs_group_device(d, recv, gi, ngroups)
            bufs.append(d)
        got_keys = og.query(want[0], want[1] if k > 32 else None)
        got_reads = og.query_reads(data)
        ctx.sync()
        for d in bufs:
            ctx.free(d)
        keys_sum += got_keys
        valid = got_reads != NONE
        reads_sum += np.where(valid, got_reads, 0)
    assert (keys_sum == want[2]).all()
    exp = _want_reads(data, k, True, want)
    assert (np.where(exp != NONE, exp, 0).astype(np.uint64) == reads_sum).all()


# ------------------------------------------------------------------ life cycle

def test_query_then_add_reflects_both(ctx):
    import cfrk_amd
    d1, _, _ = orc.synth_reads(0, 3000, 150, 20000)
    d2, _, _ = orc.synth_reads(3000, 3000, 150, 20000)
    g = cfrk_amd.GlobalCounter(ctx, 31, cfrk_amd.CFRK_CANONICAL, 100000)
    g.add(d1)
    _check_job(g, d1, 31, True)
    g.add(d2)
    _check_job(g, np.concatenate([d1, d2]), 31, True)


def test_new_begin_with_another_k_invalidates(ctx):
    import cfrk_amd
    data, _, _ = orc.synth_reads(0, 3000, 150, 20000)
    for k in (31, 21, 63, 9, 31):
        g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, 100000)
        g.add(data)
        _check_job(g, data, k, True)


@pytest.mark.parametrize("k", [12, 31, 63])
def test_queries_leave_the_result_untouched(ctx, k):
    import cfrk_amd
    data, _, _ = orc.synth_reads(0, 4000, 150, 20000)
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, 100000)
    g.add(data)
    before = (g.digest(), g.histogram(300), g.export())
    _check_job(g, data, k, True)
    after = (g.digest(), g.histogram(300), g.export())
    assert before[0] == after[0] and (before[1] == after[1]).all()
    assert all((a == b).all() for a, b in zip(before[2], after[2]))


def test_query_errors(ctx):
    import ctypes as C
    import cfrk_amd
    L = cfrk_amd.load_library()
    keys = np.zeros(4, np.uint64)
    out = np.zeros(4, np.uint32)
    data = np.zeros(64, np.int8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    fresh = cfrk_amd.Context(0)
    try:
        assert L.cfrk_global_query(fresh._h, vp(keys), None, 4, vp(out)) == CFRK_ERR_STATE
        assert L.cfrk_global_query_reads(fresh._h, vp(data), None, None, 64, 0, vp(out)) == CFRK_ERR_STATE
        assert L.cfrk_global_query_device(fresh._h, None, None, 4, None) == CFRK_ERR_STATE
        assert L.cfrk_global_query_reads_device(fresh._h, None, 64, None) == CFRK_ERR_STATE
    finally:
        fresh.close()
    reads, _, _ = orc.synth_reads(0, 2000, 150, 20000)
    g = cfrk_amd.GlobalCounter(ctx, 31, cfrk_amd.CFRK_CANONICAL | cfrk_amd.CFRK_RUNS_ONLY, 100000)
    g.add(reads)
    for call in (lambda: g.query(keys), lambda: g.query_reads(data)):
        with pytest.raises(cfrk_amd.CfrkError) as e:
            call()
        assert e.value.code == CFRK_ERR_STATE
    g = cfrk_amd.GlobalCounter(ctx, 31, cfrk_amd.CFRK_CANONICAL, 100000)
    g.add(reads)
    h = ctx._h
    assert L.cfrk_global_query(h, None, None, 4, vp(out)) == CFRK_ERR_ARG
    assert L.cfrk_global_query(h, vp(keys), None, 4, None) == CFRK_ERR_ARG
    assert L.cfrk_global_query(h, vp(keys), None, -1, vp(out)) == CFRK_ERR_ARG
    assert L.cfrk_global_query(h, None, None, 0, None) == 0
    assert L.cfrk_global_query_device(h, None, None, 4, None) == CFRK_ERR_ARG
    assert L.cfrk_global_query_reads(h, None, None, None, 64, 0, vp(out)) == CFRK_ERR_ARG
    assert L.cfrk_global_query_reads(h, vp(data), None, None, 64, 0, None) == CFRK_ERR_ARG
    assert L.cfrk_global_query_reads(h, vp(data), None, None, -1, 0, vp(out)) == CFRK_ERR_ARG
    assert L.cfrk_global_query_reads(h, None, None, None, 0, 0, None) == 0
    assert L.cfrk_global_query_reads_device(h, None, 64, None) == CFRK_ERR_ARG
    d, o = ctx.alloc(256), ctx.alloc(1024)
    try:
        assert L.cfrk_global_query_reads_device(h, C.c_void_p(d + 1), 64, C.c_void_p(o)) == CFRK_ERR_ALIGN
    finally:
        ctx.free(d); ctx.free(o)
    # layout checked like cfrk_global_add's
    dd, st, ln = refsem.flatten([np.zeros(10, np.int8), np.ones(10, np.int8)])
    st = st.copy(); st[1] += 1
    with pytest.raises(cfrk_amd.CfrkError) as e:
        g.query_reads(dd, st, ln)
    assert e.value.code == -5
    assert len(g.query(np.zeros(0, np.uint64))) == 0


@pytest.mark.parametrize("k", [12, 31, 63])
def test_device_forms_equal_host_forms(ctx, k):
    import cfrk_amd
    data, _, _ = orc.synth_reads(0, 3000, 150, 20000)
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, 100000)
    g.add(data)
    want = _oracle(data, k, True)
    wlo, whi = want[0], want[1]
    rng = np.random.default_rng(k)
    qlo = np.concatenate([wlo, rng.integers(0, 1 << 62, 1000, dtype=np.uint64) & np.uint64((1 << min(2 * k, 64)) - 1)])
    qhi = np.concatenate([whi, np.zeros(1000, np.uint64)])
    host_k = g.query(qlo, qhi)
    host_r = g.query_reads(data)
    n, nN = len(qlo), len(data)
    d_lo, d_hi, d_o = ctx.alloc(n * 8), ctx.alloc(n * 8), ctx.alloc(n * 4)
    d_data, d_or = ctx.alloc(nN + 64), ctx.alloc(nN * 4 + 64)
    try:
        ctx.h2d(d_lo, qlo); ctx.h2d(d_hi, qhi); ctx.h2d(d_data, data)
        g.query_device(d_lo, d_hi, n, d_o)
        g.query_reads_device(d_data, nN, d_or)
        g.query_reads_device(d_data, nN - 5, d_or + 4)          # (an output that is not 16-byte aligned)
        ctx.sync()
        dev_k = np.empty(n, np.uint32); ctx.d2h(dev_k, d_o)
        dev_r = np.empty(nN - 4, np.uint32); ctx.d2h(dev_r, d_or)
    finally:
        for p in (d_lo, d_hi, d_o, d_data, d_or):
            ctx.free(p)
    assert (dev_k == host_k).all()
    assert dev_r[0] == host_r[0]
    short = g.query_reads(data[:nN - 5])
    assert (dev_r[1:] == short).all()


@pytest.mark.parametrize("k", [12, 31, 32, 63])
def test_saturated_key_reads_count_max(ctx, k):
    import cfrk_amd
    two = k > 32
    g = cfrk_amd.GlobalCounter(ctx, k, 0, 1024)
    full = (1 << (2 * k)) - 1
    klo = np.array([5, 5, 77, full & ((1 << 64) - 1)], np.uint64)
    khi = np.array([1 if two else 0] * 2 + [0, full >> 64], np.uint64)
    cnts = np.array([0xF0000000, 0xF0000000, 9, 0xFFFFFFF0], np.uint32)
    for i in range(0, 4, 2):
        d_lo, d_hi, d_cnt = ctx.alloc(16), ctx.alloc(16), ctx.alloc(8)
        ctx.h2d(d_lo, klo[i:i + 2]); ctx.h2d(d_hi, khi[i:i + 2]); ctx.h2d(d_cnt, cnts[i:i + 2])
        g.merge_device(d_lo, d_hi if two else 0, d_cnt, 2)
        ctx.sync()
        ctx.free(d_lo); ctx.free(d_hi); ctx.free(d_cnt)
    got = g.query(klo[1:], khi[1:])                  # (no CFRK_ERR_COUNT_OVERFLOW from queries)
    assert list(got) == [cfrk_amd.CFRK_COUNT_MAX, 9, 0xFFFFFFF0]
    reads = np.full(k + 1, 3, np.int8)               # the all-T key twice
    assert list(g.query_reads(reads)) == [0xFFFFFFF0, 0xFFFFFFF0] + [NONE] * (k - 1)


# ------------------------------------------------------------------ full size, no oracle

def test_query_reads_full_size_invariant(ctx):
    """10^7 reads of configs[1]'s shape, k = 31 canonical, queried with the reads they were counted from: no valid
    window answers 0, valid windows = sum(c), sum(answers) = sum(c^2)"""
    import cfrk_amd
    R, L, k = 10_000_000, 150, 31
    nN = R * (L + 1)
    d = ctx.alloc(nN + 64)
    o = ctx.alloc(nN * 4 + 64)
    try:
        ctx.synth_reads_device(0, R, L, R, d)
        g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, R + 1024)
        g.add_device(d, nN)
        g.query_reads_device(d, nN, o)
        ctx.sync()
        nvalid = zero = total = 0
        step = 1 << 27
        buf = np.empty(step, np.uint32)
        for p in range(0, nN, step):
            m = min(step, nN - p)
            ctx.d2h(buf[:m], o + 4 * p)
            a = buf[:m]
            v = a[a != NONE]
            nvalid += len(v)
            zero += int((v == 0).sum())
            total += int(v.sum(dtype=np.uint64))
    finally:
        ctx.sync()
        ctx.free(d)
        ctx.free(o)
    _, _, cnt = g.export()
    c = cnt.astype(np.uint64)
    assert zero == 0
    assert nvalid == int(c.sum())
    assert total == int((c * c).sum())


# ------------------------------------------------------------------ CLI

def _cli():
    from .conftest import ROOT
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "cfrk_amd", "cfrk")


_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def _query_text(seqs, k, canonical, want):
    """the --query-out format restated: per record its windows' counts, '-' where a window holds a non-ACGT base"""
    lines = []
    for s in seqs:
        data = np.array([_CODE.get(ch, -1) for ch in s.upper()], np.int8)
        ans = _want_reads(data, k, canonical, want)[:max(len(s) - k + 1, 0)]
        lines.append(" ".join("-" if a == NONE else str(int(a)) for a in ans))
    return ("\n".join(lines) + "\n").encode() if lines else b""


@pytest.mark.parametrize("k", [5, 15, 31, 63])
def test_cli_query(tmp_path, k):
    cli = _cli()
    rng = np.random.default_rng(800 + k)
    genome = rng.integers(0, 4, 8000)
    seqs = []
    for _ in range(1500):
        L = int(rng.integers(20, 220))
        a = int(rng.integers(0, len(genome) - L))
        seqs.append("".join("ACGT"[c] for c in genome[a:a + L]))
    fa = tmp_path / "g.fasta"
    fa.write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(seqs)))
    qs = [seqs[3], seqs[10][:k - 1], "", "ACGTNACGT" * 12, seqs[7].lower(), "T" * (k + 3),
          "".join("ACGT"[c] for c in rng.integers(0, 4, 300))]
    qf = tmp_path / "q.fasta"
    qf.write_text("".join(f">q{i}\n{s}\n" for i, s in enumerate(qs)))
    # the oracle's result: the reads as the CLI's native parser gives them
    data, _, _ = refsem.flatten([np.array([_CODE[ch] for ch in s], np.int8) for s in seqs])
    want = _oracle(data, k, True)
    want_txt = _query_text(qs, k, True, want)
    base = [cli, str(fa)]

    def run(out, *extra):
        subprocess.run(base + [str(out), str(k), "--global", "--canonical", "--query", str(qf)] + list(extra),
                       check=True, timeout=300)

    run(tmp_path / "full.txt", "--query-out", str(tmp_path / "q1.txt"), "--binary")
    assert (tmp_path / "q1.txt").read_bytes() == want_txt
    # answers come from the whole result, whatever the output's count range
    run(tmp_path / "f.txt", "--query-out", str(tmp_path / "q2.txt"), "--min-count", "2")
    assert (tmp_path / "q2.txt").read_bytes() == want_txt
    run(tmp_path / "g2.txt", "--query-out", str(tmp_path / "q3.txt"), "--gpus", "2", "--same-device")
    assert (tmp_path / "q3.txt").read_bytes() == want_txt
    # query only: the output path is not created
    for extra in ([], ["--gpus", "2", "--same-device"]):
        (tmp_path / "q4.txt").unlink(missing_ok=True)
        run(tmp_path / "none.txt", "--query-out", str(tmp_path / "q4.txt"), "--query-only", *extra)
        assert (tmp_path / "q4.txt").read_bytes() == want_txt
        assert not (tmp_path / "none.txt").exists()
    # a saved count file, queried without recounting
    subprocess.run([cli, "--query-db", str(tmp_path / "full.txt"), "--query", str(qf), "--query-out",
                    str(tmp_path / "q5.txt")], check=True, timeout=300)
    assert (tmp_path / "q5.txt").read_bytes() == want_txt
    run(tmp_path / "m2.bin", "--query-out", str(tmp_path / "q6.txt"), "--binary", "--min-count", "2")
    subprocess.run([cli, "--query-db", str(tmp_path / "m2.bin"), "--query", str(qf), "--query-out",
                    str(tmp_path / "q7.txt")], check=True, timeout=300)
    wlo, whi, wcnt = want
    keep = wcnt >= 2
    assert (tmp_path / "q7.txt").read_bytes() == _query_text(qs, k, True, (wlo[keep], whi[keep], wcnt[keep]))
