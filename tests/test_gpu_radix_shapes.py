"""GPU: radix.hip (global jobs with k <= 16) at every leaf shape, with buffers CRAFTED for its structure
(tests/radix_ref.py, tests/radix_cases.py): both halves of a packed 16-bit counter word, a leaf at 65528 and at 65536
elements (the line between packed counters and the two-pass mode), two-pass leaves with keys at both ends of both
halves, keys that look like pads, RX2's padded tile at its largest, regions and segments of 1 .. 17 elements, level 1
and the leaves laid out again (1, 2 and 3 tiles per region in the scalar RX2), the leaf kernel's result buffer filled
to 704, 705 and past it, several adds into one job (k = 16: alternating with msp.hip), the grid-stride loop of the
k <= 7 kernel, and idx = 13 at k = 13.

Every test first holds its assumptions to the product: cfrk_debug_radix_info's shape for this k and size equals
radix_ref.shape, and after the add the attempts of the layout loop and the re-layouts equal radix_ref.predict; the
construction itself (which leaf holds what, n per leaf, modes) is asserted where the buffer is built, from its bytes.
Only then the result: the exported (key, count) list equals the builder's multiset entry for entry, digest() equals the
oracle's digest of it, and a CFRK_FORCE_HASH job on the same buffer gives the same digest.  Exact everywhere."""
import os

import numpy as np
import pytest

from . import oracle_lib as orc
from . import radix_cases as rc
from . import radix_ref as rr

pytestmark = pytest.mark.gpu

SHAPE_KEYS = ("b1", "b2", "idx", "mul", "inv", "cap1", "cap2", "takes", "direct", "hi8")


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


_GRID = {}


def _grid(ctx, k):
    """the leaf kernel's grid at k on this device: asked of the product after a one-tile add"""
    import cfrk_amd
    if k not in _GRID:
        g = cfrk_amd.GlobalCounter(ctx, k, 0, 1024)
        g.add(np.append(np.zeros(k, np.int8), np.full(8192 - k, -1, np.int8)))
        assert g.export()[2].tolist() == [1]
        _GRID[k] = cfrk_amd.radix_info(k, 8192, ctx)["grid"]
        assert _GRID[k] > 0
    return _GRID[k]


def _flags(b, extra=0):
    import cfrk_amd
    return (cfrk_amd.CFRK_CANONICAL if b.canonical else 0) | extra


def _assert_shape(b):
    import cfrk_amd
    info = cfrk_amd.radix_info(b.k, len(b.data))
    assert {x: info[x] for x in SHAPE_KEYS} == {x: b.sh[x] for x in SHAPE_KEYS} and info["takes"]


def _assert_add(ctx, b, grid=None):
    """what the add did, against the prediction"""
    import cfrk_amd
    info = cfrk_amd.radix_info(b.k, len(b.data), ctx)
    if b.sh["direct"]:
        assert info["attempts"] == 0 and info["grid"] >= 1
        return info
    p = rr.predict(b)
    assert (info["attempts"], info["relaid1"], info["relaid2"]) == (p["attempts"], p["relaid1"], p["relaid2"]), (info, p)
    assert grid is None or info["grid"] == grid
    return info


def _assert_export(g, counts, what):
    keys = np.array(sorted(counts), np.uint64)
    want = np.array([counts[int(x)] for x in keys], np.uint64)
    lo, hi, cnt = g.export()
    assert len(lo) == len(keys), (what, "distinct", len(lo), len(keys))
    bad = np.nonzero((lo != keys) | (cnt.astype(np.uint64) != want))[0]
    assert len(bad) == 0, (what, bad[:8], lo[bad[:8]], cnt[bad[:8]], keys[bad[:8]], want[bad[:8]])
    assert not hi.any()
    assert g.digest() == orc.digest(keys, None, want), what


def _hash_digest(ctx, k, flags, hint, buffers, debug=None):
    """digest after each add of a CFRK_FORCE_HASH job fed the same buffers (a context holds ONE job: call this when the
    job under test has been read out)"""
    import cfrk_amd
    gh = cfrk_amd.GlobalCounter(ctx, k, flags | cfrk_amd.CFRK_FORCE_HASH, hint)
    out = []
    try:
        for i, data in enumerate(buffers):
            if debug is not None:
                gh.set_debug_flags(debug[i])
            gh.add(data)
            out.append(gh.digest())
    finally:
        if debug is not None:
            gh.set_debug_flags(0)
    return out


def _run(ctx, b, grid=None, what="", check=None):
    """assumptions, the add, its course, the result; check(lo, cnt): further assertions on the radix job's export (a
    context holds one job at a time, so they run before the CFRK_FORCE_HASH job begins) -> radix_info after the add"""
    import cfrk_amd
    _assert_shape(b)
    hint = max(4096, 2 * len(b.counts))
    g = cfrk_amd.GlobalCounter(ctx, b.k, _flags(b), hint)
    g.add(b.data)
    info = _assert_add(ctx, b, grid)
    _assert_export(g, b.counts, what)
    if check is not None:
        lo, _, cnt = g.export()
        check(lo, cnt)
    d = g.digest()
    assert _hash_digest(ctx, b.k, _flags(b), hint, [b.data]) == [d], what
    return info


# a ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,canonical", [(13, False), (15, False), (16, False), (13, True)])
def test_a_both_halves_of_a_packed_counter_word(ctx, k, canonical):
    """counters 2c and 2c + 1 of one leaf with counts (1, N), (N, 1), (N, N), counter 0, the last counter and one in
    each half, the leaf at n = 65528 (mode 2, asserted in the construction)"""
    _run(ctx, rc.case_a(k, canonical), what="a")


# b ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n,canonical", [(13, 65528, False), (13, 65536, False), (16, 65528, False), (16, 65536, False),
                                           (16, 65528, True), (16, 65536, True)])
def test_b_the_65536_line(ctx, k, n, canonical):
    """one even counter holds all n elements of its leaf: n = 65528 is counted in packed 16-bit counters, n = 65536
    must take the two-pass mode -- in a 16-bit half the count would carry into the odd neighbour"""
    b = rc.case_b(k, n, canonical)

    def check(lo, cnt):
        assert cnt.tolist() == [n] and b.odd not in lo.tolist()

    _run(ctx, b, what="b", check=check)


# c ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,canonical", [(13, False), (15, False), (16, False), (15, True)])
def test_c_two_pass_leaf_between_packed_leaves(ctx, k, canonical):
    """n >= 65536 with keys at the first and last counter of each half, counts 1 .. 70000; the same workgroup walks a
    packed leaf before it and one after it"""
    grid = _grid(ctx, k)
    _run(ctx, rc.case_c(k, grid, canonical), grid, what="c")


# d ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [4, 7, 8, 10, 12, 13, 15, 16])
def test_d_keys_that_look_like_pads(ctx, k, canonical):
    """level-1 value all ones (k = 12: 0xFFFF, exactly the 16-bit plane; k = 16: 0xFFFFFF and the scrambled key
    0xFFFFFFFF, where a key fills its register), counter all ones, raw and scrambled 0 and 4^k - 1, poly-A / poly-T"""
    _run(ctx, rc.case_d(k, canonical), what="d")


# e ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,canonical", [(8, False), (12, False), (13, False), (12, True)])
def test_e_short_regions_and_segments(ctx, k, canonical):
    """regions of 1, 7, 8, 9, 15, 16, 17 elements under the fixed stride (the partial last vector of the vector RX2, one
    plane at k = 8, both from k = 12) and segments of 1, 7, 8, 9 elements"""
    _run(ctx, rc.case_e_small(k, canonical), what="e-small")


@pytest.mark.parametrize("k,big,canonical", [(10, False, False), (10, True, False), (16, False, False), (16, True, False),
                                             (16, False, True)])
def test_e_the_padded_tile_at_its_largest(ctx, k, big, canonical):
    """one region of exactly 8192 elements, all 2^b2 sub-bins present with counts = 1 mod 8: 8192 + 7 * 2^b2 slots.
    big: under the fixed stride (vector RX2); else after level 1 was laid out again (scalar RX2)"""
    _run(ctx, rc.case_e_tile(k, big, canonical), what="e-tile")


# f ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,size,one_leaf,canonical",
                         [(k, s, False, False) for k in (12, 15, 16) for s in (8192, 8193, 16385)] +
                         [(12, 16385, True, False), (16, 8193, True, True)])
def test_f_level_1_laid_out_again(ctx, k, size, one_leaf, canonical):
    """all keys in one bin, the largest region above cap1: 1, 2 and 3 tiles per region in the scalar RX2; one_leaf: the
    leaves overflow as well (three attempts)"""
    b = rc.case_f(k, size, one_leaf, canonical)
    info = _run(ctx, b, what="f")
    assert info["relaid1"] and info["attempts"] == (3 if one_leaf else 2)


# g ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,canonical", [(12, False), (13, False), (13, True)])
def test_g_the_result_buffer(ctx, k, canonical):
    """successive leaves of one workgroup with (300, 404), (300, 405), (704, 1), (705), (10, 705, 10), (0, 704, 0, 1)
    distinct keys: the buffer filled to exactly 704, the flush before 705, the direct route, a direct leaf between
    buffered ones.  (A workgroup walks nleaf / grid leaves: two at k = 12 on 256 CUs, so the patterns of three and four
    leaves run at k = 13 only; the construction asserts that at least four patterns fit.)"""
    grid = _grid(ctx, k)
    b = rc.case_g(k, grid, canonical)
    assert k != 13 or len(b.patterns) == len(rc.PATTERNS) or (1 << (b.sh["b1"] + b.sh["b2"])) // grid < 4
    _run(ctx, b, grid, what="g")


# h ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,canonical", [(7, False), (12, False), (15, False), (12, True)])
def test_h_three_adds_accumulate(ctx, k, canonical):
    import cfrk_amd
    adds = rc.case_h(k, canonical)
    g = cfrk_amd.GlobalCounter(ctx, k, _flags(adds[0]), 4096)
    total, digests = {}, []
    for b in adds:
        _assert_shape(b)
        g.add(b.data)
        _assert_add(ctx, b)
        for key, c in b.counts.items():
            total[key] = total.get(key, 0) + c
        _assert_export(g, total, "h")
        digests.append(g.digest())
    assert len(total) < sum(len(b.counts) for b in adds)          # (the sets overlap)
    assert _hash_digest(ctx, k, _flags(adds[0]), 4096, [b.data for b in adds]) == digests


def test_h_k16_adds_alternate_between_radix_and_msp(ctx):
    """three adds into one k = 16 job, the second kept away from radix.hip (CFRK_DEBUG_NO_RADIX16): msp.hip's records
    exist after the second add only; the export after each add equals the running multiset"""
    import cfrk_amd
    adds = rc.case_h(16)
    g = cfrk_amd.GlobalCounter(ctx, 16, 0, 4096)
    total, digests = {}, []
    debug = [0, cfrk_amd.CFRK_DEBUG_NO_RADIX16, 0]
    try:
        for i, b in enumerate(adds):
            _assert_shape(b)
            g.set_debug_flags(debug[i])
            g.add(b.data)
            rec = g.msp_info()["l2_records"]
            assert (rec != 0) == (i == 1), (i, rec)
            if i != 1:
                _assert_add(ctx, b)
            for key, c in b.counts.items():
                total[key] = total.get(key, 0) + c
            _assert_export(g, total, f"h16 add {i}")
            digests.append(g.digest())
    finally:
        g.set_debug_flags(0)
    assert _hash_digest(ctx, 16, 0, 4096, [b.data for b in adds], debug) == digests


# i ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,canonical", [(1, False), (4, False), (7, False), (4, True)])
def test_i_the_direct_kernels_grid_stride_loop(ctx, k, canonical):
    """20 MB of random codes, 1 % invalid: more than 8 * CUs tiles of 8192 bytes, so every workgroup of the k <= 7
    kernel goes round its loop more than once (asserted from the grid the product reports)"""
    import cfrk_amd
    nN = 20 * (1 << 20)
    rng = np.random.default_rng(k)
    data = rng.integers(0, 4, nN, dtype=np.int8)
    data[rng.random(nN) < 0.01] = -1
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL if canonical else 0, 1 << 15)
    g.add(data)
    info = cfrk_amd.radix_info(k, nN, ctx)
    assert info["direct"] and (nN + 8191) // 8192 > info["grid"] >= 1
    wlo, whi, wcnt = orc.global_count(data, k, orc.ORC_CANONICAL if canonical else 0, threads=8)
    lo, hi, cnt = g.export()
    assert len(lo) == len(wlo) and (lo == wlo).all() and (cnt.astype(np.uint64) == wcnt).all()
    d = g.digest()
    assert d == orc.digest(wlo, whi, wcnt)
    assert _hash_digest(ctx, k, cfrk_amd.CFRK_CANONICAL if canonical else 0, 1 << 15, [data]) == [d]


# j ------------------------------------------------------------------------------------------------------------
J_K, J_L, J_G = 13, 150, 1_000_000


def _j_size():
    """(reads, bytes): the smallest whole number of 150-base reads above the last size that still chooses idx = 14"""
    lo_n, hi_n = 1, 1 << 40
    while hi_n - lo_n > 1:                                    # bisection on the reference
        mid = (lo_n + hi_n) // 2
        lo_n, hi_n = (mid, hi_n) if rr.shape(J_K, mid)["idx"] == 14 else (lo_n, mid)
    R = lo_n // (J_L + 1) + 1
    return R, R * (J_L + 1)


@pytest.fixture(scope="module")
def j_reads(ctx):
    """the reads of case j, generated on the device, as the host sees them (shared by both strands, never changed)"""
    R, nN = _j_size()
    d = ctx.alloc(nN + 64)
    try:
        ctx.synth_reads_device(0, R, J_L, J_G, d)
        host = np.empty(nN, np.int8)
        ctx.d2h(host, d)
    finally:
        ctx.free(d)
    host.setflags(write=False)
    return host


@pytest.mark.parametrize("canonical", [False, True])
def test_j_idx_13_at_k13(ctx, j_reads, canonical):
    """the smallest whole number of 150-base reads above the batch size from which the host chooses 2^13 keys per leaf
    and 32-bit counters at k = 13 (b2 = 5): that instantiation against the threaded oracle, entry for entry.  The add's
    course is predicted from the buffer's bytes like everywhere else (radix_ref.survey: regions, segments, bounds of n per
    leaf; the regions are two RX2 tiles long, so n is bounded, not exact -- predict() refuses if that left the
    re-layouts open).  Most of this test's time is the oracle."""
    import cfrk_amd
    k = J_K
    R, nN = _j_size()
    threads = max(1, min(64, len(os.sched_getaffinity(0))))
    assert rr.shape(k, nN)["idx"] == 13 and rr.shape(k, nN - (J_L + 1))["idx"] == 14
    info = cfrk_amd.radix_info(k, nN)
    assert {x: info[x] for x in SHAPE_KEYS} == {x: rr.shape(k, nN)[x] for x in SHAPE_KEYS}
    assert (info["idx"], info["b2"]) == (13, 5) and info["takes"]
    b = rr.survey(j_reads, k, canonical, threads=min(threads, 16))
    p = rr.predict(b)
    assert set(p["mode"].values()) == {0} and len(p["mode"]) == 1 << 13         # every leaf holds keys, 32-bit counters
    flags = cfrk_amd.CFRK_CANONICAL if canonical else 0
    g = cfrk_amd.GlobalCounter(ctx, k, flags, 4 * J_G)
    g.add(j_reads)
    after = cfrk_amd.radix_info(k, nN, ctx)
    assert (after["attempts"], after["relaid1"], after["relaid2"]) == (p["attempts"], p["relaid1"], p["relaid2"]), (after, p)
    lo, hi, cnt = g.export()
    gd = g.digest()
    wlo, whi, wcnt = orc.global_count(j_reads, k, orc.ORC_CANONICAL if canonical else 0, threads=threads)
    assert int(wcnt.sum()) == R * (J_L - k + 1)
    assert len(lo) == len(wlo) and (lo == wlo).all() and (cnt.astype(np.uint64) == wcnt).all()
    assert gd == orc.digest(wlo, whi, wcnt)
    assert _hash_digest(ctx, k, flags, 4 * J_G, [j_reads]) == [gd]
