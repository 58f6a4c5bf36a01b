"""GPU: per-read abundance statistics against a finished global result (cfrk_global_read_stats / _device): all seven
fields against numpy over tests.oracle_lib.global_count on a k grid, query reads that differ from the counted ones,
thresholds, both lane-group widths and the long-read path, every counting path behind the index, a saturated key,
errors, the job's life cycle, out-of-range reads in the device form, and the CLI's --query-stats / --stats-below.
The window restatement (_windows, _lookup) is test_gpu_query.py's; the library's own query_reads is never the
reference."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from . import oracle_lib as orc
from . import refsem
from .test_gpu_query import _CODE, _cli, _grid_reads, _lookup, _oracle, _random_reads, _windows

pytestmark = pytest.mark.gpu

CFRK_ERR_ARG, CFRK_ERR_STATE, CFRK_ERR_LAYOUT = -1, -4, -5
COUNT_MAX = 0xFFFFFFFE
FIELDS = ("windows", "present", "below", "min", "median", "max", "sum")
KS = [5, 12, 13, 21, 31, 32, 33, 47, 64]


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


def _ref_stats(data, start, length, k, canonical, want, threshold):
    """numpy reference: the valid windows of every read, their oracle counts, and the seven fields"""
    import cfrk_amd
    lo, hi, valid = _windows(data, k, canonical)
    cnt = _lookup(want, lo, hi)
    out = np.zeros(len(start), cfrk_amd.READ_STATS_DTYPE)
    for i, (s, L) in enumerate(zip(start, length)):
        m = max(int(L) - k + 1, 0)
        c = np.sort(cnt[s:s + m][valid[s:s + m]]).astype(np.uint64)
        if len(c) == 0:
            continue
        out[i] = (len(c), int((c >= 1).sum()), int((c < threshold).sum()), int(c[0]), int(c[(len(c) - 1) // 2]),
                  int(c[-1]), int(c.sum()))
    return out


def _assert_rows(got, exp, what=""):
    assert got.dtype == exp.dtype and len(got) == len(exp)
    for f in FIELDS:
        bad = np.nonzero(got[f] != exp[f])[0]
        assert len(bad) == 0, (what, f, bad[:10], got[bad[:10]], exp[bad[:10]])


def _unflatten(data, start, length):
    return [data[s:s + L].copy() for s, L in zip(start, length)]


def _stats_reads(k, seed=0):
    """test_gpu_query's grid mix plus: reads of exactly CFRK_STATS_FAST_WINDOWS and one more window, reads between the
    16-lane and the 64-lane capacity, long reads (random with a repeated stretch, a homopolymer), ties, both parities"""
    import cfrk_amd
    rng = np.random.default_rng(4200 + k + seed)
    reads = _unflatten(*_grid_reads(k))
    F = cfrk_amd.CFRK_STATS_FAST_WINDOWS
    genome = rng.integers(0, 4, 6000).astype(np.int8)
    for nwin in (F, F + 1, 256, 257, 255, 1000, 1001):
        L = nwin + k - 1
        a = int(rng.integers(0, len(genome) - min(L, 3000)))
        r = np.concatenate([genome[a:a + min(L, 3000)], rng.integers(0, 4, max(L - 3000, 0)).astype(np.int8)])
        assert len(r) == L
        reads.append(r)
    rep = rng.integers(0, 4, 5000).astype(np.int8)
    long_read = np.concatenate([rep, rng.integers(0, 4, 12000).astype(np.int8), rep, genome[:1500]])
    long_read[7000] = -1                                         # an invalid code inside a long read
    assert len(long_read) >= 20000
    reads.append(long_read)
    reads.append(np.full(3000, 1, np.int8))                      # long homopolymer: every window ties
    reads.append(np.full(k + 6, 2, np.int8))                     # 7 windows, all equal
    reads.append(np.full(k + 7, 2, np.int8))                     # 8 windows, all equal
    reads.append(genome[100:100 + k + 10].copy())                # 11 windows
    reads.append(genome[100:100 + k + 11].copy())                # 12 windows
    return refsem.flatten(reads)


# ------------------------------------------------------------------ parity on the k grid

@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("canonical", [False, True])
def test_read_stats_vs_oracle(ctx, k, canonical):
    import cfrk_amd
    data, start, length = _stats_reads(k)
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL if canonical else 0, 0)
    g.add(data, start, length)
    want = _oracle(data, k, canonical)
    exp = _ref_stats(data, start, length, k, canonical, want, 2)
    # the mix holds what it was built for
    F = cfrk_amd.CFRK_STATS_FAST_WINDOWS
    w = exp["windows"]
    assert (w == 0).any() and (w == F).any() and (w == F + 1).any() and (w > 10000).any()
    assert ((w > 256) & (w < F)).any() and ((w > 0) & (w <= 256)).any()
    mixed = exp["min"] != exp["max"]
    assert (mixed & (w % 2 == 0)).any() and (mixed & (w % 2 == 1)).any()
    assert ((w > 1) & ~mixed).any()
    got = g.read_stats(data, start, length, 2)
    _assert_rows(got, exp, (k, canonical))
    assert g.digest() == orc.digest(*want, two_word=k > 32)


@pytest.mark.parametrize("k", [12, 31, 47])
def test_query_reads_that_differ_from_the_counted_reads(ctx, k):
    import cfrk_amd
    data, start, length = _grid_reads(k)
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, 0)
    g.add(data, start, length)
    want = _oracle(data, k, True)
    rng = np.random.default_rng(77 + k)
    counted = _unflatten(data, start, length)
    other = _random_reads(rng, 200, 1, 400, 0.01)
    other += [np.concatenate([counted[310 + j][:90], rng.integers(0, 4, 80).astype(np.int8)]) for j in range(40)]
    other.append(rng.integers(0, 4, 30000).astype(np.int8))     # a long read, nearly all of it absent for k > 12
    qd, qs, ql = refsem.flatten(other)
    exp = _ref_stats(qd, qs, ql, k, True, want, 2)
    # the reference itself holds rows with absent windows, and rows with both present and absent ones
    assert (exp["present"] < exp["windows"]).any()
    assert ((exp["windows"] > 0) & (exp["min"] == 0)).any()
    assert ((exp["present"] > 0) & (exp["present"] < exp["windows"])).any()
    _assert_rows(g.read_stats(qd, qs, ql, 2), exp, k)


@pytest.mark.parametrize("k", [12, 31, 47])
def test_thresholds(ctx, k):
    import cfrk_amd
    data, start, length = _stats_reads(k, seed=1)
    g = cfrk_amd.GlobalCounter(ctx, k, 0, 0)
    g.add(data, start, length)
    want = _oracle(data, k, False)
    rng = np.random.default_rng(k)
    qd, qs, ql = refsem.flatten(_unflatten(data, start, length)[::3] + _random_reads(rng, 100, 1, 300, 0.02))
    for t in (0, 1, 2, 0xFFFFFFFF):
        exp = _ref_stats(qd, qs, ql, k, False, want, t)
        if t == 0:
            assert (exp["below"] == 0).all()
        if t == 0xFFFFFFFF:
            assert (exp["below"] == exp["windows"]).all()
        _assert_rows(g.read_stats(qd, qs, ql, t), exp, (k, t))
    assert len(g.read_stats(qd[:0], qs[:0], ql[:0], 3)) == 0      # nS = 0 is fine


# ------------------------------------------------------------------ host and device forms, lane-group widths, bounds

def _device_stats(ctx, g, data, start, length, threshold, skew=0, fill=0xAB):
    """the device form on buffers of its own; data placed `skew` bytes off a 16-byte boundary, the output pre-filled"""
    import cfrk_amd
    nN, nS = len(data), len(start)
    d_data, d_start, d_length = ctx.alloc(nN + 64), ctx.alloc(max(nS, 1) * 8), ctx.alloc(max(nS, 1) * 4)
    d_out = ctx.alloc(max(nS, 1) * 32)
    out = np.full(nS * 32, fill, np.uint8)
    try:
        if nN:
            ctx.h2d(d_data + skew, data)
        if nS:
            ctx.h2d(d_start, start); ctx.h2d(d_length, length); ctx.h2d(d_out, out)
        g.read_stats_device(d_data + skew, d_start, d_length, nN, nS, threshold, d_out)
        ctx.sync()
        if nS:
            ctx.d2h(out, d_out)
    finally:
        ctx.sync()
        for p in (d_data, d_start, d_length, d_out):
            ctx.free(p)
    return out.view(cfrk_amd.READ_STATS_DTYPE)


@pytest.mark.parametrize("k", [12, 31, 63])
def test_device_form_equals_host_form(ctx, k):
    import cfrk_amd
    data, start, length = _stats_reads(k, seed=2)
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, 0)
    g.add(data, start, length)
    host = g.read_stats(data, start, length, 3)
    _assert_rows(host, _ref_stats(data, start, length, k, True, _oracle(data, k, True), 3), k)
    for skew in (0, 1, 7):                                       # no alignment requirement on d_data
        _assert_rows(_device_stats(ctx, g, data, start, length, 3, skew), host, (k, skew))


@pytest.mark.parametrize("k", [21, 40])
def test_both_lane_group_widths(ctx, k):
    """a short-read batch (every read within the 16-lane group's 256 windows) and a long-read batch (every read above
    it, within the 64-lane group's capacity): by construction each runs through one width only"""
    import cfrk_amd
    rng = np.random.default_rng(500 + k)
    genome = rng.integers(0, 4, 50000).astype(np.int8)

    def sample(n, lo, hi):
        reads = []
        for L in rng.integers(lo, hi, n):
            a = int(rng.integers(0, len(genome) - int(L)))
            r = genome[a:a + int(L)].copy()
            r[rng.random(int(L)) < 0.005] = -1
            reads.append(r)
        return refsem.flatten(reads)

    short = sample(3000, 100, 200)
    long_ = sample(400, 256 + k, cfrk_amd.CFRK_STATS_FAST_WINDOWS + k - 1)
    assert (short[2] - k + 1 <= 256).all()
    assert (long_[2] - k + 1 > 256).all() and (long_[2] - k + 1 <= cfrk_amd.CFRK_STATS_FAST_WINDOWS).all()
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, 0)
    g.add(*short)
    g.add(*long_)
    want = _oracle(np.concatenate([short[0], long_[0]]), k, True)
    for batch in (short, long_):
        exp = _ref_stats(*batch, k, True, want, 4)
        assert (exp["min"] != exp["max"]).any()
        _assert_rows(g.read_stats(*batch, 4), exp, k)


def test_device_form_out_of_range_reads_get_zero_rows(ctx):
    """start / length are not checked by the device form: a read that does not lie inside [0, nN) gets a zero row, its
    neighbours their own (bounds by construction: nothing outside the buffers is touched)"""
    import cfrk_amd
    k = 21
    data, start, length = _grid_reads(k)
    g = cfrk_amd.GlobalCounter(ctx, k, 0, 0)
    g.add(data, start, length)
    exp = _ref_stats(data, start, length, k, False, _oracle(data, k, False), 2)
    st, ln = start.copy(), length.copy()
    nN = len(data)
    bad = {3: (-5, 100), 10: (nN + 7, 50), 11: (nN - 10, 100), 50: (0, -3), 51: (int(start[51]), 0x7FFFFFFF),
           120: (-(1 << 62), 150), 121: ((1 << 62), 150), 300: (nN, 30), len(st) - 1: (nN - 20, 21 + 5)}
    for i, (s, L) in bad.items():
        st[i], ln[i] = s, L
    for i in bad:
        exp[i] = (0,) * 7
    assert (exp["windows"] > 0).sum() > 400                      # (the neighbours have rows of their own)
    got = _device_stats(ctx, g, data, st, ln, 2)
    _assert_rows(got, exp)


# ------------------------------------------------------------------ every counting path behind the index

def _path_reads(seed):
    rng = np.random.default_rng(seed)
    reads = _random_reads(rng, 2000, 1, 300)
    genome = rng.integers(0, 4, 5000).astype(np.int8)
    for _ in range(1000):
        a = int(rng.integers(0, len(genome) - 150))
        reads.append(genome[a:a + 150].copy())
    reads.append(np.full(200, 0, np.int8))
    return refsem.flatten(reads)


@pytest.mark.parametrize("k, path", [(13, "radix"), (16, "radix"), (16, "partitioned"), (31, "partitioned"),
                                     (47, "partitioned"), (13, "hash"), (31, "hash"), (47, "hash")])
def test_every_counting_path_gives_the_same_stats(ctx, k, path):
    import cfrk_amd
    data, start, length = _path_reads(1600 + k)
    flags = cfrk_amd.CFRK_CANONICAL | (cfrk_amd.CFRK_FORCE_HASH if path == "hash" else 0)
    g = cfrk_amd.GlobalCounter(ctx, k, flags, 1 << 20)
    if k == 16 and path == "partitioned":
        g.set_debug_flags(cfrk_amd.CFRK_DEBUG_NO_RADIX16)
    try:
        g.add(data, start, length)
        if path == "partitioned" and k <= 32:               # (the one-word partitioned path reports its records)
            assert g.msp_info()["l2_records"] > 0
        exp = _ref_stats(data, start, length, k, True, _oracle(data, k, True), 2)
        _assert_rows(g.read_stats(data, start, length, 2), exp, (k, path))
    finally:
        g.set_debug_flags(0)


@pytest.mark.parametrize("k", [12, 31, 63])
def test_read_stats_on_a_merged_job(ctx, k):
    import cfrk_amd
    data, start, length = orc.synth_reads(0, 3000, 150, 20000)
    want = _oracle(data, k, True)
    wlo, whi, wcnt = want
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, 100000)
    cnt32 = wcnt.astype(np.uint32)
    d_lo, d_hi, d_cnt = ctx.alloc(wlo.nbytes), ctx.alloc(whi.nbytes), ctx.alloc(cnt32.nbytes)
    try:
        ctx.h2d(d_lo, wlo); ctx.h2d(d_hi, whi); ctx.h2d(d_cnt, cnt32)
        g.merge_device(d_lo, d_hi if k > 32 else 0, d_cnt, len(wlo))
        ctx.sync()
    finally:
        ctx.free(d_lo); ctx.free(d_hi); ctx.free(d_cnt)
    _assert_rows(g.read_stats(data, start, length, 2), _ref_stats(data, start, length, k, True, want, 2), k)


@pytest.mark.parametrize("k", [12, 31, 32, 63])
def test_saturated_key(ctx, k):
    """the construction of test_gpu_saturation.py: pre-counted pairs whose sum passes 2^32 - 2.  The median reads
    CFRK_COUNT_MAX, the sum adds it, and no overflow error comes back"""
    import cfrk_amd
    two = k > 32
    g = cfrk_amd.GlobalCounter(ctx, k, 0, 1024)
    full = (1 << (2 * k)) - 1
    klo = np.array([full & ((1 << 64) - 1), 5], np.uint64)
    khi = np.array([full >> 64, 0], np.uint64)
    for cnts in ([0xF0000000, 9], [0xF0000000, 1]):
        d_lo, d_hi, d_cnt = ctx.alloc(16), ctx.alloc(16), ctx.alloc(8)
        ctx.h2d(d_lo, klo); ctx.h2d(d_hi, khi); ctx.h2d(d_cnt, np.array(cnts, np.uint32))
        g.merge_device(d_lo, d_hi if two else 0, d_cnt, 2)
        ctx.sync()
        ctx.free(d_lo); ctx.free(d_hi); ctx.free(d_cnt)
    five = np.array([(5 >> (2 * (k - 1 - j))) & 3 if 2 * (k - 1 - j) < 8 else 0 for j in range(k)], np.int8)   # key 5
    reads = [np.full(k + 2, 3, np.int8),                                   # the all-T key three times
             np.concatenate([np.full(k + 1, 3, np.int8), [0]]).astype(np.int8),   # twice, then an absent k-mer
             np.concatenate([five, np.full(k, 3, np.int8)]).astype(np.int8)]
    data, start, length = refsem.flatten(reads)
    want = (np.array([5, klo[0]], np.uint64), np.array([0, khi[0]], np.uint64), np.array([10, 1 << 33], np.uint64))
    exp = _ref_stats(data, start, length, k, False, want, 11)
    assert tuple(exp[0]) == (3, 3, 0, COUNT_MAX, COUNT_MAX, COUNT_MAX, 3 * COUNT_MAX)
    assert tuple(exp[1]) == (3, 2, 1, 0, COUNT_MAX, COUNT_MAX, 2 * COUNT_MAX)
    assert exp[2]["min"] == 0 and exp[2]["max"] == COUNT_MAX and exp[2]["present"] == 2 and exp[2]["below"] == k
    _assert_rows(g.read_stats(data, start, length, 11), exp, k)       # (no CFRK_ERR_COUNT_OVERFLOW)


# ------------------------------------------------------------------ errors, life cycle

def test_read_stats_errors(ctx):
    import cfrk_amd
    L = cfrk_amd.load_library()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    data, start, length = refsem.flatten([np.zeros(40, np.int8), np.ones(40, np.int8)])
    out = np.zeros(2, cfrk_amd.READ_STATS_DTYPE)
    host_args = lambda h: (h, vp(data), vp(start), vp(length), len(data), 2, 0, vp(out))
    fresh = cfrk_amd.Context(0)
    try:
        assert L.cfrk_global_read_stats(*host_args(fresh._h)) == CFRK_ERR_STATE
        assert L.cfrk_global_read_stats_device(fresh._h, None, None, None, 82, 2, 0, None) == CFRK_ERR_STATE
    finally:
        fresh.close()
    reads, _, _ = orc.synth_reads(0, 2000, 150, 20000)
    g = cfrk_amd.GlobalCounter(ctx, 31, cfrk_amd.CFRK_CANONICAL | cfrk_amd.CFRK_RUNS_ONLY, 100000)
    g.add(reads)
    with pytest.raises(cfrk_amd.CfrkError) as e:
        g.read_stats(data, start, length)
    assert e.value.code == CFRK_ERR_STATE
    g = cfrk_amd.GlobalCounter(ctx, 31, cfrk_amd.CFRK_CANONICAL, 100000)
    g.add(reads)
    h = ctx._h
    assert L.cfrk_global_read_stats(*host_args(h)) == 0
    for drop in range(4):                                           # each pointer NULL in turn
        a = [vp(data), vp(start), vp(length), vp(out)]
        a[drop] = None
        assert L.cfrk_global_read_stats(h, a[0], a[1], a[2], len(data), 2, 0, a[3]) == CFRK_ERR_ARG
        assert L.cfrk_global_read_stats_device(h, a[0], a[1], a[2], len(data), 2, 0, a[3]) == CFRK_ERR_ARG
    assert L.cfrk_global_read_stats(h, vp(data), vp(start), vp(length), -1, 2, 0, vp(out)) == CFRK_ERR_ARG
    assert L.cfrk_global_read_stats(h, vp(data), vp(start), vp(length), len(data), -1, 0, vp(out)) == CFRK_ERR_ARG
    assert L.cfrk_global_read_stats_device(h, None, None, None, -1, 0, 0, None) == CFRK_ERR_ARG
    assert L.cfrk_global_read_stats_device(h, None, None, None, 10, -2, 0, None) == CFRK_ERR_ARG
    assert L.cfrk_global_read_stats(h, None, None, None, 0, 0, 0, None) == 0
    assert L.cfrk_global_read_stats_device(h, None, None, None, 0, 0, 0, None) == 0
    bad = start.copy(); bad[1] += 1                                 # layout checked like cfrk_global_add's
    with pytest.raises(cfrk_amd.CfrkError) as e:
        g.read_stats(data, bad, length)
    assert e.value.code == CFRK_ERR_LAYOUT
    assert g.read_stats(data, start, length)["windows"].tolist() == [10, 10]      # the job is still usable


@pytest.mark.parametrize("k", [12, 31, 63])
def test_read_stats_leave_the_result_untouched_and_reuse_the_index(ctx, k):
    import cfrk_amd
    data, start, length = orc.synth_reads(0, 4000, 150, 20000)
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, 100000)
    g.add(data)
    want = _oracle(data, k, True)
    before = (g.digest(), g.histogram(300), g.export())
    exp = _ref_stats(data, start, length, k, True, want, 2)
    _assert_rows(g.read_stats(data, start, length, 2), exp, k)
    held = ctx.device_bytes()
    _assert_rows(g.read_stats(data, start, length, 2), exp, k)        # the second call: same index, nothing new allocated
    assert ctx.device_bytes() == held
    # queries and stats share the index: the windows' counts are what the reference says
    lo, hi, valid = _windows(data, k, True)
    assert (g.query_reads(data)[valid] == _lookup(want, lo, hi)[valid]).all()
    assert ctx.device_bytes() >= held
    after = (g.digest(), g.histogram(300), g.export())
    assert before[0] == after[0] and (before[1] == after[1]).all()
    assert all((a == b).all() for a, b in zip(before[2], after[2]))
    # an add changes the result: the next call sees it
    g.add(data)
    exp2 = _ref_stats(data, start, length, k, True, (want[0], want[1], want[2] * 2), 2)
    _assert_rows(g.read_stats(data, start, length, 2), exp2, k)


# ------------------------------------------------------------------ CLI

def _stats_text(rows):
    from .conftest import ROOT
    L = C.CDLL(os.path.join(ROOT, "cfrk_amd", "libcfrk_host.so"))
    L.cfrk_host_format_read_stats.argtypes = [C.c_void_p, C.c_int64, C.c_char_p, C.c_size_t]
    L.cfrk_host_format_read_stats.restype = C.c_size_t
    p = rows.ctypes.data_as(C.c_void_p) if len(rows) else None
    n = L.cfrk_host_format_read_stats(p, len(rows), None, 0)
    buf = C.create_string_buffer(n + 1)
    assert L.cfrk_host_format_read_stats(p, len(rows), buf, n) == n
    return buf.raw[:n]


@pytest.mark.parametrize("k", [9, 31, 63])
def test_cli_query_stats(tmp_path, k):
    cli = _cli()
    rng = np.random.default_rng(8800 + k)
    genome = rng.integers(0, 4, 8000)
    seqs = []
    for _ in range(1500):
        L = int(rng.integers(20, 220))
        a = int(rng.integers(0, len(genome) - L))
        seqs.append("".join("ACGT"[c] for c in genome[a:a + L]))
    fa = tmp_path / "g.fasta"
    fa.write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(seqs)))
    qs = [seqs[3], seqs[10][:k - 1], "", "ACGTNACGT" * 12, seqs[7].lower(), "T" * (k + 3),
          "".join("ACGT"[c] for c in rng.integers(0, 4, 300)),
          "".join("ACGT"[c] for c in genome[:3000]), seqs[5] + "N" + seqs[6]]
    qf = tmp_path / "q.fasta"
    qf.write_text("".join(f">q{i}\n{s}\n" for i, s in enumerate(qs)))
    data, _, _ = refsem.flatten([np.array([_CODE[ch] for ch in s], np.int8) for s in seqs])
    want = _oracle(data, k, True)
    qd, qst, qln = refsem.flatten([np.array([_CODE.get(ch, -1) for ch in s.upper()], np.int8) for s in qs])
    want_txt = _stats_text(_ref_stats(qd, qst, qln, k, True, want, 2))
    assert want_txt.count(b"\n") == len(qs)
    base = [cli, str(fa)]
    sf, none = tmp_path / "s1.txt", tmp_path / "none.txt"
    subprocess.run(base + [str(none), str(k), "--global", "--canonical", "--query", str(qf), "--query-stats", str(sf),
                           "--stats-below", "2", "--query-only"], check=True, timeout=300)
    assert sf.read_bytes() == want_txt
    assert not none.exists()
    # with --query-out as well, and the counts written in the binary form
    s2, q2, full = tmp_path / "s2.txt", tmp_path / "q2.txt", tmp_path / "full.bin"
    subprocess.run(base + [str(full), str(k), "--global", "--canonical", "--binary", "--query", str(qf), "--query-stats",
                           str(s2), "--stats-below", "2", "--query-out", str(q2)], check=True, timeout=300)
    assert s2.read_bytes() == want_txt and q2.exists() and full.exists()
    # the saved count file, queried without recounting
    s3 = tmp_path / "s3.txt"
    subprocess.run([cli, "--query-db", str(full), "--query", str(qf), "--query-stats", str(s3), "--stats-below", "2"],
                   check=True, timeout=300)
    assert s3.read_bytes() == want_txt
    # the default threshold is 0
    s4 = tmp_path / "s4.txt"
    subprocess.run([cli, "--query-db", str(full), "--query", str(qf), "--query-stats", str(s4)], check=True, timeout=300)
    assert s4.read_bytes() == _stats_text(_ref_stats(qd, qst, qln, k, True, want, 0))
