"""GPU: the open-addressing structures behind every global-mode answer -- the HBM table (table_add1 / table_add2), the
query index (qidx_hash_kernel, qidx_ones_kernel) and the probe loops with their unrolled copies (q_find1 / q_find2,
query_reads1/2_kernel, stats_read) -- with keys CRAFTED to collide (tests/hash_craft.py): chains that run off the last
slot and go on at slot 0, clusters of hundreds of keys on a handful of home slots, absent keys that must be walked to
the end of a cluster, two-word keys that differ in one word only, the k = 32 all-T key behind an occupied home, and
thousands of lanes claiming one chain at once.

Every test first holds its assumptions against the product (cfrk_debug_hash_info): the geometry it crafted for, and the
Python hash on its own keys; then its construction (tests.hash_craft.occupied_after: the occupied set of linear probing
does not depend on the insertion order); only then the result.  The reference is a plain dict {(lo, hi): count}; for
reads the window restatement of test_gpu_query.py -- never the library's own queries.  Capacity hint 512 and at most
512 distinct keys give a table and an index of 1024 slots each, so one key set serves both."""
import functools

import numpy as np
import pytest

from . import hash_craft as hc
from . import oracle_lib as orc
from .test_gpu_query import _lookup, _windows
from .test_gpu_read_stats import _assert_rows, _ref_stats

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
HINT = 512
LG = 10                                 # table and index of a job of <= 512 keys with hint 512
LAST = (1 << LG) - 1
# (k, canonical job) of the table tests; two-word keys above 32
A_CASES = [(13, False), (31, False), (32, False), (47, False), (64, False), (31, True)]
KINDS = ["wrap", "cluster", "words", "full", "over"]
SOURCES = ["merge", "hash", "default"]  # hash_merge_kernel / hash_count{1,2}_kernel / the default path's result list


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ key sets (crafted once, shared, never changed)

def _seed(*a):
    return np.random.default_rng(list(a) + [11])


def _cat(parts):
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


@functools.lru_cache(maxsize=None)
def _keys(kind, k, canonical=False, lg=LG):
    """-> (lo, hi): 'wrap' 40 keys homing on the last slot; 'cluster' 400 keys on the last 8 slots; 'words' (k > 32)
    64 keys with one lo + 64 with one hi, all on the last slot; 'full' 512 keys on the last 8 slots (index load
    exactly 0.5); 'over' 513 keys on the last 8 slots of 2^11"""
    two = k > 32
    last = (1 << lg) - 1
    rng = _seed(k, int(canonical), lg, KINDS.index(kind))
    craft = lambda slot, n: hc.keys_homing_on(slot, lg, k, n, canonical=canonical, two_word=two, rng=rng)
    if kind == "wrap":
        lo, hi = craft(last, 40)
    elif kind == "words":
        lo, hi = _cat([hc.same_lo_different_hi(last, lg, k, 64, rng), hc.same_hi_different_lo(last, lg, k, 64, rng)])
    else:
        per = {"cluster": [50] * 8, "full": [64] * 8, "over": [64] * 7 + [65]}[kind]
        lo, hi = _cat([craft(last - 7 + j, n) for j, n in enumerate(per)])
    assert len({(int(l), int(h)) for l, h in zip(lo, hi)}) == len(lo)
    lo.setflags(write=False)
    hi.setflags(write=False)
    return lo, hi


def _counts(n, seed, top=200):
    return np.random.default_rng(seed).integers(1, top + 1, n).astype(np.uint32)


# ------------------------------------------------------------------ assumptions, construction, result

def _assert_hash(lo, hi, two):
    """the Python hash equals the product's on these very keys"""
    import cfrk_amd
    mine = hc.key_hash(lo, hi, two)
    for l, h, m in zip(lo, hi, mine):
        info = cfrk_amd.hash_info(int(l), int(h))
        assert info[3 if two else 2] == int(m), ("slot hash changed", int(l), int(h))


def _assert_construction(kind, lo, hi, two, lg=LG):
    """what the key set was built for, from the probing simulation -> the occupied slots (bool per slot)"""
    homes = hc.home(lo, hi, lg, two)
    occ, disp = hc.occupied_after(homes, lg)
    last = (1 << lg) - 1
    assert occ[0] >= 0 and homes[occ[0]] >= last - 7, "slot 0 is not taken by a key that homes at the table's end"
    if kind in ("wrap", "words"):
        assert (homes == last).all() and sorted(disp.tolist()) == list(range(len(lo)))   # every displacement once
    else:
        bound = {"cluster": 300, "full": 400, "over": 400}[kind]
        assert disp.max() >= bound and hc.forced_displacement(homes, lg) >= bound
    return occ >= 0


def _ref_arrays(ref):
    """dict -> (lo, hi, counts) sorted by (hi, lo), as export() and the oracle order them"""
    items = sorted(ref.items(), key=lambda kv: (kv[0][1], kv[0][0]))
    return (np.array([kv[0][0] for kv in items], np.uint64), np.array([kv[0][1] for kv in items], np.uint64),
            np.array([kv[1] for kv in items], np.uint64))


def _assert_result(g, ref, two, what):
    wlo, whi, wcnt = _ref_arrays(ref)
    lo, hi, cnt = g.export()
    assert len(lo) == len(wlo), (what, "distinct", len(lo), len(wlo), sorted(ref)[:8])
    bad = np.nonzero((lo != wlo) | ((hi != whi) if two else False) | (cnt.astype(np.uint64) != wcnt))[0]
    assert len(bad) == 0, (what, bad[:8], lo[bad[:8]], hi[bad[:8]], cnt[bad[:8]], wlo[bad[:8]], whi[bad[:8]], wcnt[bad[:8]])
    assert g.digest() == orc.digest(wlo, whi, wcnt, two_word=two), what
    nb = 300
    assert (g.histogram(nb) == np.bincount(np.minimum(wcnt, nb - 1).astype(np.int64), minlength=nb).astype(np.uint64)).all(), what


def _merge(ctx, g, lo, hi, cnt, two):
    lo, hi, cnt = (np.ascontiguousarray(lo, np.uint64), np.ascontiguousarray(hi, np.uint64),
                   np.ascontiguousarray(cnt, np.uint32))
    bufs = [ctx.alloc(a.nbytes) for a in (lo, hi, cnt)]
    try:
        for p, a in zip(bufs, (lo, hi, cnt)):
            ctx.h2d(p, a)
        g.merge_device(bufs[0], bufs[1] if two else 0, bufs[2], len(lo))
        ctx.sync()
    finally:
        for p in bufs:
            ctx.free(p)


def _reads_of(lo, hi, cnt, k, rng):
    """key i as a read of exactly k bases, cnt[i] times, shuffled -> (data, start, length)"""
    rows = np.full((len(lo), k + 1), -1, np.int8)
    for i, (l, h) in enumerate(zip(lo, hi)):
        rows[i, :k] = hc.key_to_read(l, h, k)
    rows = rows[rng.permutation(np.repeat(np.arange(len(lo)), cnt.astype(np.int64)))]
    n = len(rows)
    assert n <= 60000
    return rows.reshape(-1), np.arange(n, dtype=np.int64) * (k + 1), np.full(n, k, np.int32)


def _job(ctx, source, k, canonical, lo, hi, cnt, seed):
    """a fresh job that holds exactly {key i: cnt[i]}, filled through `source`; the table geometry is asserted"""
    import cfrk_amd
    two = k > 32
    flags = (cfrk_amd.CFRK_CANONICAL if canonical else 0) | (cfrk_amd.CFRK_FORCE_HASH if source == "hash" else 0)
    g = cfrk_amd.GlobalCounter(ctx, k, flags, HINT)
    assert g.hash_geometry() == (LG, 0), "table sizing rule changed"
    if source == "merge":
        _merge(ctx, g, lo, hi, cnt, two)
    else:
        g.add(*_reads_of(lo, hi, cnt, k, np.random.default_rng(seed)))
    return g


def _with_all_t(k, lo, hi, cnt):
    """k = 32: the all-T key 41 times on top (the table keeps it in a side word, the index as an ordinary entry)"""
    if k != 32:
        return lo, hi, cnt
    return (np.append(lo, np.uint64(hc.ALL_ONES)), np.append(hi, np.uint64(0)), np.append(cnt, np.uint32(41)))


# ------------------------------------------------------------------ A. the table through merge_device

@pytest.mark.parametrize("k,canonical,kind", [(k, c, kind) for k, c in A_CASES for kind in ("wrap", "cluster", "words")
                                              if kind != "words" or k > 32])      # (A3 is two-word only)
def test_table_merge(ctx, k, canonical, kind):
    """A1 wrap / A2 cluster / A3 one-word-shared keys into a fresh job (pairs go straight to hash_merge_kernel), then
    A4: the same keys again in another order with other counts, then a list that holds every key three times.
    include/cfrk_abi.h puts no uniqueness condition on the pairs of cfrk_global_merge_device ("add pre-counted (key,
    count) pairs"), so duplicates inside one list are within the contract: their counts add."""
    two = k > 32
    klo, khi = _keys(kind, k, canonical)
    _assert_hash(klo, khi, two)
    _assert_construction(kind, klo, khi, two)
    lo, hi, c1 = _with_all_t(k, klo, khi, _counts(len(klo), k))
    g = _job(ctx, "merge", k, canonical, lo, hi, c1, 0)
    ref = {(int(l), int(h)): int(c) for l, h, c in zip(lo, hi, c1)}
    _assert_result(g, ref, two, (k, kind, "first merge", lo[:4], hi[:4]))
    rng = np.random.default_rng(k + 5)
    p = rng.permutation(len(lo))
    c2 = _counts(len(lo), k + 1, 1000)
    _merge(ctx, g, lo[p], hi[p], c2[p], two)
    for l, h, c in zip(lo, hi, c2):
        ref[(int(l), int(h))] += int(c)
    _assert_result(g, ref, two, (k, kind, "second merge"))
    p = rng.permutation(np.tile(np.arange(len(lo)), 3))
    c3 = _counts(len(p), k + 2, 50)
    _merge(ctx, g, lo[p], hi[p], c3, two)
    for i, c in zip(p, c3):
        ref[(int(lo[i]), int(hi[i]))] += int(c)
    _assert_result(g, ref, two, (k, kind, "every key three times in one list"))


# ------------------------------------------------------------------ B. table and lists through the counting kernels

@pytest.mark.parametrize("source", ["hash", "default"])
@pytest.mark.parametrize("k,kind", [(k, kind) for k in (13, 31, 32, 47) for kind in ("wrap", "cluster", "words")
                                    if kind != "words" or k > 32])
def test_counting_kernels(ctx, k, source, kind):
    """reads of exactly k bases, key i c_i times (1..200), shuffled: with CFRK_FORCE_HASH tens of thousands of lanes of
    hash_count1/2_kernel claim one chain at the same time; on the default path the result is a list"""
    two = k > 32
    klo, khi = _keys(kind, k)
    _assert_hash(klo, khi, two)
    _assert_construction(kind, klo, khi, two)
    lo, hi, cnt = _with_all_t(k, klo, khi, _counts(len(klo), 3 * k))
    g = _job(ctx, source, k, False, lo, hi, cnt, k)
    ref = {(int(l), int(h)): int(c) for l, h, c in zip(lo, hi, cnt)}
    _assert_result(g, ref, two, (k, source, kind, lo[:4], hi[:4]))


# ------------------------------------------------------------------ C. index build and every lookup form

def _device_query(ctx, g, lo, hi, two):
    out = np.empty(len(lo), np.uint32)
    bufs = [ctx.alloc(max(a.nbytes, 16)) for a in (lo, hi, out)]
    try:
        ctx.h2d(bufs[0], lo)
        ctx.h2d(bufs[1], hi)
        g.query_device(bufs[0], bufs[1] if two else 0, len(lo), bufs[2])
        ctx.sync()
        ctx.d2h(out, bufs[2])
    finally:
        for p in bufs:
            ctx.free(p)
    return out


def _device_reads(ctx, g, data, start, length, threshold):
    import cfrk_amd
    ans = np.empty(len(data), np.uint32)
    rows = np.zeros(len(start), cfrk_amd.READ_STATS_DTYPE)
    arrs = (data, start, length, ans, rows)
    bufs = [ctx.alloc(a.nbytes + 16) for a in arrs]
    try:
        for p, a in zip(bufs[:3], arrs[:3]):
            ctx.h2d(p, a)
        g.query_reads_device(bufs[0], len(data), bufs[3])
        g.read_stats_device(bufs[0], bufs[1], bufs[2], len(data), len(start), threshold, bufs[4])
        ctx.sync()
        ctx.d2h(ans, bufs[3])
        ctx.d2h(rows, bufs[4])
    finally:
        for p in bufs:
            ctx.free(p)
    return ans, rows


def _absent(slot, lg, k, n, canonical, present, rng):
    lo, hi = hc.keys_homing_on(slot, lg, k, n + 8, canonical=canonical, two_word=k > 32, rng=rng)
    keep = [i for i in range(len(lo)) if (int(lo[i]), int(hi[i])) not in present][:n]
    assert len(keep) == n
    return lo[keep], hi[keep]


def _check_lookups(ctx, g, k, canonical, ref, occupied, lg, device_forms, extra_absent=None):
    """query / query_reads / read_stats (host forms; device forms when asked) against the dict, on crafted probes.
    occupied: the index's occupied slots without the all-T entry (bool per slot, from the simulation)."""
    two = k > 32
    n_slots = 1 << lg
    last = n_slots - 1
    rng = _seed(k, lg, int(canonical), 77)
    digest = g.digest()
    plo, phi, pcnt = _ref_arrays(ref)
    want = (plo, phi, pcnt)
    present = set(ref)
    first_empty = next(s for s in range(n_slots) if not occupied[s])          # the cluster wraps: slot 0 is taken
    assert first_empty >= 8 and occupied[last]
    # ---- keys
    groups = [(plo, phi)]
    groups += [_absent(last - 7 + j, lg, k, 25, canonical, present, rng) for j in range(8)]      # 200 on the cluster's homes
    groups += [_absent(s, lg, k, 2, canonical, present, rng) for s in (0, first_empty // 2, first_empty - 1)]
    groups += [_absent(first_empty, lg, k, 2, canonical, present, rng)]       # home = the first empty slot behind it
    if extra_absent is not None:
        groups.append(extra_absent)
    qlo, qhi = _cat(groups)
    _assert_hash(qlo[len(plo):], qhi[len(plo):], two)
    exp = _lookup(want, qlo, qhi)
    assert (exp[:len(plo)] == pcnt).all() and (exp[len(plo):] == 0).all()
    homes = hc.home(qlo[len(plo):], qhi[len(plo):], lg, two)
    n_behind = 25 * int(occupied[last - 7:].sum()) + 6                          # misses that start on an occupied slot ...
    assert n_behind >= 31 and occupied[homes].sum() >= n_behind and (~occupied[homes]).sum() >= 2   # ... on an empty one
    got = g.query(qlo, qhi if two else None)
    assert g.hash_geometry() == (LG, lg), "index sizing rule changed"
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, (k, "query", bad[:8], qlo[bad[:8]], qhi[bad[:8]], got[bad[:8]], exp[bad[:8]])
    if canonical:                                                              # the reverse complement reads the same count
        rc = [hc.revcomp_int(int(h) << 64 | int(l), k) for l, h in zip(plo, phi)]
        rlo = np.array([x & hc.ALL_ONES for x in rc], np.uint64)
        rhi = np.array([x >> 64 for x in rc], np.uint64)
        assert (g.query(rlo, rhi if two else None) == pcnt).all()
    if k < 64:                                                                 # bits at or above 2k: no such k-mer
        top = [(int(h) << 64 | int(l)) | (1 << (2 * k + j % (128 - 2 * k))) for j, (l, h) in enumerate(zip(plo[:64], phi[:64]))]
        tlo = np.array([x & hc.ALL_ONES for x in top], np.uint64)
        thi = np.array([x >> 64 for x in top], np.uint64)
        assert (g.query(tlo, thi) == 0).all()
    if device_forms:
        assert (_device_query(ctx, g, qlo, qhi, two) == exp).all()
    # ---- reads: exactly k bases (present and absent keys); k + 7 bases beginning with a crafted k-mer; an invalid base
    # inside; chains of crafted k-mers with filler of ~120 windows (a 16-lane group, 8 windows per lane: whole batches
    # of QB) and of more than 256 windows (the 64-lane path)
    rd = lambda i: hc.key_to_read(qlo[i], qhi[i], k)
    pick = rng.permutation(len(qlo))
    reads = [rd(i) for i in range(len(qlo))]
    reads += [np.concatenate([rd(i), rng.integers(0, 4, 7).astype(np.int8)]) for i in pick[:300]]
    broken = np.concatenate([rd(pick[0]), rd(pick[1]), rng.integers(0, 4, 7).astype(np.int8)])
    broken[k + 3] = -1
    reads.append(broken)
    for nwin, bad_at in ((120, None), (300, None), (300, 5 * k + 2)):
        parts = []
        while sum(len(p) for p in parts) < nwin + k - 1:
            parts += [rd(int(rng.integers(0, len(qlo)))), rng.integers(0, 4, int(rng.integers(0, 4))).astype(np.int8)]
        r = np.concatenate(parts)[:nwin + k - 1]
        if bad_at is not None:
            r[bad_at] = -1
        reads.append(r)
    if k == 32 and (hc.ALL_ONES, 0) in present:
        reads.append(np.full(32, 3, np.int8))
        reads.append(np.full(45, 3, np.int8))
    from . import refsem
    data, start, length = refsem.flatten(reads)
    wl, wh, valid = _windows(data, k, canonical)
    exp_reads = np.where(valid, _lookup(want, wl, wh), np.uint32(NONE)).astype(np.uint32)
    # the mix the reads were built for: hits, misses behind an occupied home, misses on an empty home, invalid windows
    wh_home = hc.home(wl[valid], wh[valid], lg, two)
    miss = exp_reads[valid] == 0
    assert (~miss).sum() >= len(plo) and (miss & occupied[wh_home]).sum() >= n_behind and (miss & ~occupied[wh_home]).sum() >= 50
    assert (~valid).sum() >= len(reads)
    got = g.query_reads(data, start, length)
    bad = np.nonzero(got != exp_reads)[0]
    assert len(bad) == 0, (k, "query_reads", bad[:8], wl[bad[:8]], wh[bad[:8]], got[bad[:8]], exp_reads[bad[:8]])
    for threshold in (0, 2, 0xFFFFFFFF):
        exp_rows = _ref_stats(data, start, length, k, canonical, want, threshold)
        if threshold == 0:
            w = exp_rows["windows"]
            assert (w == 1).any() and (w == 8).any() and (w == 120).any() and (w == 300).any() and ((w < 300) & (w >= 300 - k)).any()
        _assert_rows(g.read_stats(data, start, length, threshold), exp_rows, (k, "read_stats", threshold))
    if device_forms:
        ans, rows = _device_reads(ctx, g, data, start, length, 2)
        assert (ans == exp_reads).all()
        _assert_rows(rows, _ref_stats(data, start, length, k, canonical, want, 2), (k, "read_stats_device"))
    assert g.digest() == digest, "the queries changed the result"


C_CASES = [(k, False, s) for k in (13, 31, 47) for s in SOURCES] + [(64, False, "merge"), (31, True, "merge")]


@pytest.mark.parametrize("kind", ["wrap", "full"])
@pytest.mark.parametrize("k,canonical,source", C_CASES)
def test_index_and_lookups(ctx, k, canonical, source, kind):
    """'wrap': 40 keys on the last slot, displacements 0 .. 39 exactly once each whatever the order (a key one slot
    behind its home, a key in slot 0, ...); 'full': 512 keys, the index at load exactly 0.5 in one wrapping cluster"""
    two = k > 32
    lo, hi = _keys(kind, k, canonical)
    _assert_hash(lo, hi, two)
    occupied = _assert_construction(kind, lo, hi, two)
    cnt = _counts(len(lo), 7 * k + len(kind))
    g = _job(ctx, source, k, canonical, lo, hi, cnt, k)
    ref = {(int(l), int(h)): int(c) for l, h, c in zip(lo, hi, cnt)}
    _check_lookups(ctx, g, k, canonical, ref, occupied, LG, device_forms=(source == "merge" and kind == "full"))


@pytest.mark.parametrize("k,source", [(13, "merge"), (31, "default"), (47, "merge"), (47, "hash")])
def test_index_of_513_keys_has_2048_slots(ctx, k, source):
    """one key more than 'full': the index doubles; the keys are crafted for THAT geometry (the table keeps 1024)"""
    two = k > 32
    lo, hi = _keys("over", k, False, 11)
    assert len(lo) == 513
    _assert_hash(lo, hi, two)
    occupied = _assert_construction("over", lo, hi, two, 11)
    cnt = _counts(len(lo), 9 * k)
    g = _job(ctx, source, k, False, lo, hi, cnt, k)
    ref = {(int(l), int(h)): int(c) for l, h, c in zip(lo, hi, cnt)}
    _check_lookups(ctx, g, k, False, ref, occupied, 11, device_forms=False)
    _assert_result(g, ref, two, (k, source, "513 keys"))


@pytest.mark.parametrize("k", [47, 64])
@pytest.mark.parametrize("source", ["merge", "hash"])
def test_two_word_lookups_compare_both_words(ctx, k, source):
    """64 keys with one lo and 64 with one hi in ONE chain, every count different; absent keys that share a word with
    present ones (same lo, other hi; same hi, other lo) and home on the same slot must read 0"""
    lo, hi = _keys("words", k)
    _assert_hash(lo, hi, True)
    occupied = _assert_construction("words", lo, hi, True)
    cnt = (np.arange(len(lo)) * 3 + 5).astype(np.uint32)
    g = _job(ctx, source, k, False, lo, hi, cnt, k)
    ref = {(int(l), int(h)): int(c) for l, h, c in zip(lo, hi, cnt)}
    present = set(ref)
    rng = _seed(k, 5)
    hbits = 2 * k - 64
    # same lo as the first group, other hi: scan hi for the last slot; same hi as the second group, other lo: solve
    cand = np.arange(1 << 22, dtype=np.uint64) if hbits >= 22 else np.arange(1 << hbits, dtype=np.uint64)
    cand = cand[hc.home(np.full(len(cand), lo[0], np.uint64), cand, LG, True) == LAST]
    cand = np.array([h for h in cand if (int(lo[0]), int(h)) not in present][:32], np.uint64)
    assert len(cand) == 32
    shift = np.uint64(64 - LG)
    t = (np.uint64(LAST) << shift) | rng.integers(0, 1 << 54, 40, dtype=np.uint64)
    olo = hc.inv_mix(t) ^ hc.mix(hi[-1:])
    olo = np.array([l for l in olo if (int(l), int(hi[-1])) not in present][:32], np.uint64)
    extra = (np.concatenate([np.full(32, lo[0], np.uint64), olo]), np.concatenate([cand, np.full(32, hi[-1], np.uint64)]))
    assert (hc.home(extra[0], extra[1], LG, True) == LAST).all()
    _check_lookups(ctx, g, k, False, ref, occupied, LG, device_forms=False, extra_absent=extra)
    _assert_result(g, ref, True, (k, source, "words"))


# ------------------------------------------------------------------ the k = 32 all-T key behind an occupied home

def _ones_home(lg):
    import cfrk_amd
    h = cfrk_amd.hash_info(hc.ALL_ONES, 0)[2]
    assert h == int(hc.hash1(hc.ALL_ONES)[0])
    return h >> (64 - lg)


def _all_t_job(ctx, source, lg, n_behind):
    """keys on the all-T key's home slot (so that it and n_behind - 1 slots after it are taken by others) plus a
    wrapping cluster at the table's end; lg = 11: 520 keys in all"""
    home = _ones_home(lg)
    rng = _seed(32, lg, n_behind)
    parts = [hc.keys_homing_on(home, lg, 32, n_behind, rng=rng)]
    parts += [hc.keys_homing_on((1 << lg) - 1 - j, lg, 32, 128 if lg == 11 else 25, rng=rng) for j in range(4)]
    lo, hi = _cat(parts)
    _assert_hash(lo, hi, False)
    homes = hc.home(lo, hi, lg, False)
    occ, _ = hc.occupied_after(homes, lg)
    n = 1 << lg
    assert all(occ[(home + j) & (n - 1)] >= 0 for j in range(max(n_behind, 4)))    # home and >= 3 slots after it: others
    cnt = _counts(len(lo), 32 + lg)
    alo, ahi, acnt = _with_all_t(32, lo, hi, cnt)
    g = _job(ctx, source, 32, False, alo, ahi, acnt, lg)
    ref = {(int(l), int(h)): int(c) for l, h, c in zip(alo, ahi, acnt)}
    assert len(ref) >= 513 if lg == 11 else len(ref) <= 512                       # the geometry the keys were crafted for
    return g, ref, occ >= 0, home


def _check_all_t(ctx, g, ref, occupied, lg):
    import cfrk_amd
    _assert_result(g, ref, False, ("all-T", lg))
    ones = np.array([hc.ALL_ONES], np.uint64)
    assert g.query(ones).tolist() == [41]
    assert g.hash_geometry() == (LG, lg)
    t = np.full(32, 3, np.int8)
    data = np.concatenate([t, np.array([-1], np.int8)])
    ans = g.query_reads(data, np.array([0], np.int64), np.array([32], np.int32))
    assert ans[0] == 41 and (ans[1:] == NONE).all()
    row = g.read_stats(data, np.array([0], np.int64), np.array([32], np.int32), 42)[0]
    assert tuple(int(x) for x in row) == (1, 1, 1, 41, 41, 41, 41)
    _check_lookups(ctx, g, 32, False, ref, occupied, lg, device_forms=False)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("lg", [10, 11])
def test_all_t_key_behind_an_occupied_home(ctx, source, lg):
    """qidx_ones_kernel inserts the side word's count after the index build: its home (computed from the hash) and the
    5 slots after it are taken by crafted keys, so it has to probe on; 41 in query, query_reads and read_stats"""
    g, ref, occupied, home = _all_t_job(ctx, source, lg, 6)
    assert occupied[home:home + 6].all() and not occupied[home + 6]
    _check_all_t(ctx, g, ref, occupied, lg)


def test_all_t_key_wraps():
    """The all-T entry can be made to run off the last slot only where its home lies within a few slots of the table's
    end (a chain from its home to the end must fit the <= 511 / <= 1023 other keys of the geometry, and the issue's
    bound is 8 slots).  Its home is fixed by the hash: slot 274 of 1024 and slot 548 of 2048 -- 750 and 1500 slots from
    the end.  It cannot be arranged in either geometry; this test states that and holds the two homes, so a change of
    the hash that makes the sub-case reachable is noticed."""
    homes = {lg: _ones_home(lg) for lg in (10, 11)}
    assert homes == {10: 274, 11: 548}
    assert all((1 << lg) - h > 8 for lg, h in homes.items())
    pytest.skip("the all-T key homes on slot 274 of 1024 / 548 of 2048: no chain from there reaches the wrap")
