"""GPU: spectral error correction (cfrk_global_correct_reads / _device, GlobalCounter.correct_reads) held to the
plain-Python rule of tests/correct_ref.py: data_out and the fix rows are EQUAL, never close, through the host form and
the device form, and the job's digest is the same before and after.  The job counts a small random genome twice, so
every genome window is solid at min_count 2; the query reads are pieces of it with planted substitutions at the edges
between the head, interior and tail cases, at the seams of the lanes, the size classes, the long path's chunks and its
rounds.  At small k chance-solid alternatives abound: the device has to agree with the reference there too, whatever the
rule makes of them.  The counts of a (k, strand rule) are computed once and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

from . import correct_ref as cr
from .test_gpu_filter import _Guarded, _upload

pytestmark = pytest.mark.gpu

CFRK_ERR_ARG, CFRK_ERR_STATE, CFRK_ERR_LAYOUT = -1, -4, -5
KS = [5, 12, 13, 21, 31, 32, 33, 47, 64]
GENOME = 9400                                            # room for a read of 9000 windows at k = 64


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ inputs (built once, shared, never changed)

@functools.lru_cache(maxsize=None)
def _genome():
    g = np.random.default_rng(2207).integers(0, 4, GENOME).astype(np.int8)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _counted():
    """the counted set: the genome twice, as two reads"""
    g = _genome()
    return cr.flatten([g, g])


@functools.lru_cache(maxsize=None)
def _counts(k, canonical):
    return cr.count_reads(*_counted(), k, canonical)


def _job(ctx, k, canonical, extra=None):
    import cfrk_amd
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL if canonical else 0, 1 << 16)
    g.add(*_counted())
    if extra is not None:
        g.add(*extra)
    return g


def _piece(a, L):
    return _genome()[a:a + L].copy()


def _sub(r, positions, rng):
    for p in positions:
        r = cr.substitute(r, p, rng)
    return r


def _device(ctx, g, data, start, length, mn, skew=0, with_fix=True):
    nN, nS = len(data), len(start)
    d_data, d_start, d_length = _upload(ctx, data, skew), _upload(ctx, start), _upload(ctx, length)
    out, fix = _Guarded(ctx, nN, 3), _Guarded(ctx, nS * 8)
    try:
        g.correct_reads_device(d_data + skew, d_start, d_length, nN, nS, mn, out.ptr, fix.ptr if with_fix else None)
        ctx.sync()
        return out.fetch(nN, np.int8), fix.fetch(nS * 8 if with_fix else 0, cr.FIX_DTYPE)
    finally:
        ctx.sync()
        for p in (d_data, d_start, d_length):
            ctx.free(p)
        out.free()
        fix.free()


def _assert_same(got, want, what):
    data, fix = got
    wdata, wfix = want
    bad = np.nonzero(data != wdata)[0]
    assert len(bad) == 0, (what, "data_out differs at bytes", bad[:10], data[bad[:10]], wdata[bad[:10]])
    bad = np.nonzero((fix["fixed"] != wfix["fixed"]) | (fix["left"] != wfix["left"]))[0]
    assert len(bad) == 0, (what, "fix rows differ at reads", bad[:10], fix[bad[:10]], wfix[bad[:10]])


def _check(ctx, g, reads, k, canonical, counts, mn, what, skew=1):
    """both forms against the reference; the digest unchanged; -> the reference's (data_out, fix)"""
    data, start, length = cr.flatten(reads)
    want = cr.correct(data, start, length, k, canonical, counts, mn)
    before = g.digest()
    _assert_same(g.correct_reads(data, start, length, mn), want, (what, "host form"))
    _assert_same(_device(ctx, g, data, start, length, mn, skew), want, (what, "device form"))
    assert g.digest() == before, what
    return want


# ------------------------------------------------------------------ every k, both strand rules: lengths and positions

def _edge_reads(k, rng):
    """reads of the lengths around k and 2k (2k + 1 is the first at which an interior run can exist) and 150 bases, clean
    and with one substitution at each edge between the head, interior and tail cases; then pairs of substitutions k - 1,
    k (one merged run, left alone) and k + 1 (two runs) apart"""
    reads = []
    for L in sorted({k - 1, k, k + 1, 2 * k - 1, 2 * k, 2 * k + 1, 150, 3 * k + 2}):
        if L < 1:
            continue
        a = int(rng.integers(0, GENOME - L))
        reads.append(_piece(a, L))
        for p in sorted({0, 1, k - 2, k - 1, k, L - k - 1, L - k, L - k + 1, L - 2, L - 1}):
            if 0 <= p < L:
                reads.append(_sub(_piece(a, L), [p], rng))
    L = 4 * k + 9
    for d in (k - 1, k, k + 1):
        for p in (0, 3, k, k + 2, L - d - 1, L - d - 4):
            if d >= 1 and 0 <= p and p + d < L:
                reads.append(_sub(_piece(int(rng.integers(0, GENOME - L)), L), [p, p + d], rng))
    return reads


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", KS)
def test_lengths_and_error_positions(ctx, k, canonical):
    rng = np.random.default_rng([k, 1])
    reads = _edge_reads(k, rng)
    g = _job(ctx, k, canonical)
    # (at k = 5 every 5-mer occurs in the genome many times: the threshold goes to the mean count, so that weak and solid
    # windows both occur)
    mn = 2 if 4 ** k > 4 * GENOME else 2 * GENOME * (2 if canonical else 1) // 4 ** k
    _, fix = _check(ctx, g, reads, k, canonical, _counts(k, canonical), mn, (k, canonical))
    if k >= 21:
        assert fix["fixed"].sum() > 40 and fix["left"].sum() > 6, "the input exercises neither outcome"
    else:
        assert fix["left"].sum() > 6


@pytest.mark.parametrize("k,canonical", [(12, True), (31, True), (33, False), (64, True)])
def test_class_seams_and_lane_seams(ctx, k, canonical):
    """reads of 256 / 257 and 2048 / 2049 windows (the seams between the three launches); a 16-lane read with an error
    at every position in turn and 64-lane reads whose runs begin in one lane's stretch and end in the next"""
    rng = np.random.default_rng([k, 2])
    reads = []
    for W in (256, 257, 2048, 2049):
        L = W + k - 1
        for rep in range(2):
            a = int(rng.integers(0, GENOME - L))
            step = k + 2 + rep * 7
            pos = list(range(int(rng.integers(0, k)), L, step)) + [L - 1]
            reads.append(_sub(_piece(a, L), sorted(set(pos)), rng))
        reads.append(_piece(int(rng.integers(0, GENOME - L)), L))
    L = 129 + k                                              # 130 windows: per = 9 at G = 16
    a = int(rng.integers(0, GENOME - L))
    reads += [_sub(_piece(a, L), [p], rng) for p in range(L)]
    for W in (1000, 1024, 700):                              # per = 16, 16 and 11 at G = 64
        L, per = W + k - 1, -(-W // 64)
        for off in (0, 1, per - 1):
            a = int(rng.integers(0, GENOME - L))
            pos = [p for p in range(k - 1 + off, L, per * ((k + 1) // per + 1)) if p < L]   # run starts a = p - k + 1 on the seams
            reads.append(_sub(_piece(a, L), pos, rng))
    g = _job(ctx, k, canonical)
    _, fix = _check(ctx, g, reads, k, canonical, _counts(k, canonical), 2, (k, canonical))
    if k >= 21:
        assert fix["fixed"].sum() > 300


@pytest.mark.parametrize("k,canonical", [(12, False), (31, True), (47, False)])
def test_long_read(ctx, k, canonical):
    """one read of about 9000 windows: runs that straddle the windows 32 j (the chunks of the threads), 8191 / 8192 (the
    seam of a round) and the k + 1 windows before it whose run starts wait for the next round; a pair too close"""
    rng = np.random.default_rng([k, 3])
    W = 9000
    L = W + k - 1
    pos = set(range(5, 8000, 2 * k + 11))                    # (an odd step: the runs meet every residue modulo 32)
    pos |= {8192 - k - 3 + k - 1, 8192 + k + 20, 8192 + 3 * k + 30, L - 1, L - 2 * k - 5}
    pos |= {8600, 8600 + k - 1}
    reads = [_sub(_piece(7, L), sorted(pos), rng)]
    for p in (8191, 8192, 8190 + k, 8191 + k, 8192 - k - 2 + k - 1, 8192 - k - 1 + k - 1, 0, L - 1):
        reads.append(_sub(_piece(11, L), [p], rng))
    reads.append(_piece(3, L))
    g = _job(ctx, k, canonical)
    _, fix = _check(ctx, g, reads, k, canonical, _counts(k, canonical), 2, (k, canonical))
    if k >= 21:
        assert fix["fixed"][0] > 60 and fix["left"][0] >= 1 and (fix["fixed"][1:-1] == 1).all()
        assert tuple(fix[-1]) == (0, 0)


# ------------------------------------------------------------------ the outcomes that leave a run alone

def test_ambiguity_no_base_and_invalid_neighbours(ctx):
    k, canonical, L = 31, True, 150
    rng = np.random.default_rng(4)
    g0 = _genome()
    m = 5000
    variant = _piece(m - 100, 200)
    variant[100] = (int(variant[100]) + 1) & 3               # the job holds two variants of the locus m ...
    extra = cr.flatten([variant, variant])
    counts = cr.count_reads(*extra, k, canonical, dict(_counts(k, canonical)))
    third = _piece(m - 70, L)
    third[70] = (int(g0[m]) + 2) & 3                         # ... and the read carries a third base there
    outside = rng.integers(0, 4, L).astype(np.int8)          # no base passes: a read from outside the genome,
    chimera = np.concatenate([_piece(100, 75), rng.integers(0, 4, 75).astype(np.int8)])
    lone = _piece(300, L)                                    # an interior error whose true base is the only way back,
    lone[60] = (int(lone[60]) + 1) & 3
    n_right, n_left, n_far = lone.copy(), lone.copy(), lone.copy()
    n_right[60 + k] = 4                                      # invalid windows [61, 91] abut the run [30, 60] behind it,
    n_left[60 - k] = -1                                      # invalid windows [-1, 29] abut it in front,
    n_far[60 + k + 1] = 4                                    # one solid window between: attempted
    reads = [third, outside, chimera, lone, n_right, n_left, n_far]
    g = _job(ctx, k, canonical, extra)
    data_out, fix = _check(ctx, g, reads, k, canonical, counts, 2, "outcomes")
    data, start, _ = cr.flatten(reads)
    assert fix.tolist() == [(0, 1), (0, 1), (0, 1), (1, 0), (0, 1), (0, 1), (1, 0)]
    changed = np.nonzero(data_out != data)[0].tolist()
    assert changed == [int(start[3]) + 60, int(start[6]) + 60]
    assert data_out[changed[0]] == g0[360]


@pytest.mark.parametrize("k,canonical", [(12, True), (31, False), (64, True)])
def test_min_count_extremes(ctx, k, canonical):
    rng = np.random.default_rng([k, 5])
    reads = _edge_reads(k, rng)[::3] + [rng.integers(0, 4, 200).astype(np.int8), _sub(_piece(50, 2300 + k), [9, 900, 2200], rng)]
    reads[1][len(reads[1]) // 2] = 4
    data, start, length = cr.flatten(reads)
    g = _job(ctx, k, canonical)
    counts = _counts(k, canonical)
    data0, fix0 = _check(ctx, g, reads, k, canonical, counts, 0, (k, "min_count 0"))
    assert (data0 == data).all() and not fix0["fixed"].any() and not fix0["left"].any()      # the identity
    _check(ctx, g, reads, k, canonical, counts, 1, (k, "min_count 1"))                        # weak means absent
    data1, fix1 = _check(ctx, g, reads, k, canonical, counts, 0xFFFFFFFF, (k, "min_count 2^32 - 1"))
    assert (data1 == data).all() and not fix1["fixed"].any()                                  # every valid window weak
    runs = [len(cr.weak_runs(cr.window_classes(r.tolist(), k, canonical, counts, 0xFFFFFFFF))) if len(r) >= k else 0 for r in reads]
    assert fix1["left"].tolist() == runs and sum(runs) > len(reads) // 2
    _check(ctx, g, reads, k, canonical, counts, 3, (k, "min_count 3"))                        # nothing is solid: counts are 2


# ------------------------------------------------------------------ the buffers

def test_buffer_rules(ctx):
    """bytes between and behind the reads and terminators of any value are copied verbatim; a read whose range does not
    lie inside [0, nN) gets {0, 0}; d_fix = NULL; nS = 0 with nN > 0 copies; no alignment requirement"""
    k, canonical = 31, True
    rng = np.random.default_rng(6)
    counts = _counts(k, canonical)
    g = _job(ctx, k, canonical)
    reads = [_sub(_piece(int(rng.integers(0, 9000)), 150), [int(rng.integers(0, 150))], rng) for _ in range(40)]
    gap = 7
    nN = sum(len(r) + gap for r in reads) + 13
    data = rng.integers(-128, 128, nN).astype(np.int8)       # (what lies between the reads: any bytes, bases too)
    start = np.zeros(len(reads), np.int64)
    at = 5
    for i, r in enumerate(reads):
        start[i] = at
        data[at:at + len(r)] = r
        data[at + len(r)] = (-1, 4, 127, -128)[i % 4]
        at += len(r) + gap
    length = np.full(len(reads), 150, np.int32)
    bad = {3: (nN - 10, 100), 5: (-5, 100), 6: (nN + 7, 50), 20: (0, -3), 21: (int(start[21]), 0x7FFFFFFF),
           30: (-(1 << 62), 150), 31: ((1 << 62), 150), 39: (nN - 20, k + 25)}
    for i, (s, L) in bad.items():
        start[i], length[i] = s, L
    want = cr.correct(data, start, length, k, canonical, counts, 2)
    assert want[1]["fixed"].sum() >= 30 and all(tuple(want[1][i]) == (0, 0) for i in bad)
    before = g.digest()
    for skew in (0, 1, 2, 7):
        _assert_same(_device(ctx, g, data, start, length, 2, skew), want, ("gaps", skew))
    got = _device(ctx, g, data, start, length, 2, 5, with_fix=False)                         # d_fix = NULL
    assert (got[0] == want[0]).all()
    # nS = 0 with nN > 0 copies (both forms)
    d_data = _upload(ctx, data)
    out = _Guarded(ctx, nN, 1)
    try:
        g.correct_reads_device(d_data, 0, 0, nN, 0, 2, out.ptr, 0)
        ctx.sync()
        assert (out.fetch(nN, np.int8) == data).all()
    finally:
        ctx.sync()
        ctx.free(d_data)
        out.free()
    copy, rows = g.correct_reads(data, np.zeros(0, np.int64), np.zeros(0, np.int32), 2)
    assert (copy == data).all() and len(rows) == 0
    assert g.digest() == before


def test_errors(ctx):
    import cfrk_amd
    L = cfrk_amd.load_library()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    data, start, length = cr.flatten([np.zeros(40, np.int8), np.ones(40, np.int8)])
    out = np.zeros_like(data)
    fix = np.zeros(2, cfrk_amd.READ_FIX_DTYPE)
    args = lambda h: (h, vp(data), vp(start), vp(length), len(data), 2, 2, vp(out), vp(fix))
    fresh = cfrk_amd.Context(0)
    try:
        assert L.cfrk_global_correct_reads(*args(fresh._h)) == CFRK_ERR_STATE              # before begin
        assert L.cfrk_global_correct_reads_device(fresh._h, None, None, None, 82, 2, 2, None, None) == CFRK_ERR_STATE
    finally:
        fresh.close()
    g = cfrk_amd.GlobalCounter(ctx, 31, cfrk_amd.CFRK_CANONICAL | cfrk_amd.CFRK_RUNS_ONLY, 100000)
    g.add(*_counted())
    with pytest.raises(cfrk_amd.CfrkError) as e:
        g.correct_reads(data, start, length, 2)
    assert e.value.code == CFRK_ERR_STATE
    g = _job(ctx, 31, True)
    h = ctx._h
    assert L.cfrk_global_correct_reads(*args(h)) == 0
    assert L.cfrk_global_correct_reads(h, vp(data), vp(start), vp(length), len(data), 2, 2, vp(out), None) == 0   # fix may be NULL
    for drop in range(4):                                           # data, start, length, data_out NULL in turn
        a = [vp(data), vp(start), vp(length), vp(out)]
        a[drop] = None
        assert L.cfrk_global_correct_reads(h, a[0], a[1], a[2], len(data), 2, 2, a[3], vp(fix)) == CFRK_ERR_ARG
        assert L.cfrk_global_correct_reads_device(h, a[0], a[1], a[2], len(data), 2, 2, a[3], vp(fix)) == CFRK_ERR_ARG
    assert L.cfrk_global_correct_reads(h, vp(data), None, None, len(data), 0, 2, None, None) == CFRK_ERR_ARG    # data_out, nN > 0
    assert L.cfrk_global_correct_reads_device(h, vp(data), None, None, len(data), 0, 2, None, None) == CFRK_ERR_ARG
    for nN, nS in ((-1, 2), (len(data), -1)):
        assert L.cfrk_global_correct_reads(h, vp(data), vp(start), vp(length), nN, nS, 2, vp(out), vp(fix)) == CFRK_ERR_ARG
        assert L.cfrk_global_correct_reads_device(h, vp(data), vp(start), vp(length), nN, nS, 2, vp(out), vp(fix)) == CFRK_ERR_ARG
    assert L.cfrk_global_correct_reads(h, None, None, None, 0, 0, 2, None, None) == 0           # nothing at all is fine
    assert L.cfrk_global_correct_reads_device(h, None, None, None, 0, 0, 2, None, None) == 0
    bad = start.copy(); bad[1] += 1                                 # layout checked like cfrk_global_add's
    with pytest.raises(cfrk_amd.CfrkError) as e:
        g.correct_reads(data, bad, length, 2)
    assert e.value.code == CFRK_ERR_LAYOUT
    with pytest.raises(ValueError):
        g.correct_reads(data, start, length, 1 << 32)
    assert g.correct_reads(data, start, length, 0)[1].tolist() == [(0, 0), (0, 0)]      # the job is still usable


# ------------------------------------------------------------------ one mixed batch

@pytest.mark.parametrize("k,canonical", [(31, True), (47, False), (12, True)])
def test_mixed_batch(ctx, k, canonical):
    """about 2000 reads of all three size classes in a shuffled order, both strands under the canonical rule, with
    random substitutions at 1 % per base and a few invalid codes: the three launches skip each other's reads"""
    rng = np.random.default_rng([k, 7])
    lens = [150] * 1700 + [int(x) for x in rng.integers(1, 2 * k, 60)] + [int(x) for x in rng.integers(257 + k, 2048 + k, 200)] + \
           [k + 254, k + 255, k + 256, k + 2046, k + 2047, k + 2048] * 2 + [int(x) for x in rng.integers(2049 + k, 3500, 8)]
    lens = [lens[i] for i in rng.permutation(len(lens))]
    reads = []
    for j, L in enumerate(lens):
        r = _piece(int(rng.integers(0, GENOME - L)), L)
        if canonical and rng.integers(0, 2):
            r = cr.revcomp(r)
        r = _sub(r, np.nonzero(rng.random(L) < 0.01)[0].tolist(), rng)
        if j % 17 == 3:
            r[int(rng.integers(0, L))] = -1 if j % 2 else 4
        reads.append(r)
    g = _job(ctx, k, canonical)
    _, fix = _check(ctx, g, reads, k, canonical, _counts(k, canonical), 2, (k, canonical), skew=3)
    if k >= 21:
        assert fix["fixed"].sum() > 1500 and fix["left"].sum() > 300
