"""GPU: the device forms with reads, text bytes and output bytes at offsets of 2^31 and 2^32 and more.

Part one -- few reads, far away.  One device buffer of N = 2^32 + 2^20 bytes is filled by the device generator (R = N //
151 reads of 150 bases from a genome of 10^5 bases) and a job per k in {12, 31, 47} counts its first 20 000 reads (dense,
one-word and two-word index).  A set of about 2 000 (start, length) entries (tests/far_ref.pick_reads) picks reads on
both sides of 2^31 and 2^32, at both ends of the buffer, 2 000 at random above 2^31, three ranges that lie across the
generator's terminators (1 400 bases: the 64-lane class; 6 000 and 40 000 bases: the long class, the last one with more
than 4 x 8192 windows, so that the correction kernel's ring of four rounds wraps) and four entries without a result
(start >= N, start + length > N, a negative start, length 0).  About 300 single bases of the buffer are patched first so
that weak windows exist; the patch is undone when the module ends.  The bytes of every entry are fetched with one d2h at
d_data + start, the plain references (normalize_ref, filter_ref, correct_ref, pair_ref, text_out_ref, the C oracle) run on
those bytes with the job's exported counts, and every row must be equal.  Every device form is called with nN = N.

Part two -- whole buffers past 4 GiB: the read query into 4 N bytes, the sketch against the merge of five pieces, the
select over all R reads, a FASTQ text of more than 2^32 bytes through parser, index and emitter (the emitter must give
back the text), a FASTA text whose parsed data pass 2^32, and the three branches that only a text of 2^31 bytes or more
can take (a record, a quality line, a header line of 2^31 bytes).  The oracle of the tiled texts is tests/far_ref.py,
which tests/test_far_offsets_cpu.py holds equal to the plain references without a GPU.

Out of scope: the host forms at these sizes (they stage into the same kernels, and a second 4 GiB host array per call
buys nothing), the CLI at these sizes, and cfrk_global_add* at these sizes (the full-size digest tests of
tests/test_gpu_parity.py cover it).

Two things the ABI fixes shape the tests.  cfrk_per_read_sparse_device gives undefined rows to reads whose ranges
overlap and takes 12 bytes of pool memory per byte of nN (include/cfrk_abi.h), so the set goes through it in layers of
ranges that do not overlap, on a context of its own that is closed afterwards (about 52 GB for the duration of that
test; every other test stays below 24 GiB).  cfrk_per_read_dense_device is defined on the struct-read layout and
documents no result for a range outside the buffer: its call takes the composite ranges lengthened to the next
terminator and leaves the four entries without a result out (test_per_read_dense_device_k4 says why).  The jobs count
through the HBM table (CFRK_FORCE_HASH): the index the device forms look up in is the same, and the partitioned
paths' pools would take the three contexts and the read query's 5 N bytes past 24 GiB."""
import collections
import ctypes as C

import numpy as np
import pytest

from . import correct_ref as cr
from . import far_ref as far
from . import fastq_ref as fq
from . import filter_ref as fr
from . import ingest_cases as ic
from . import normalize_ref as nr
from . import oracle_lib as orc
from . import pair_ref as pr
from . import text_out_ref as tr
from .test_gpu_query import _want_reads

pytestmark = pytest.mark.gpu

CFRK_ERR_LAYOUT, CFRK_ERR_SMALL_BUF = -5, -9
COUNT_MAX = 0xFFFFFFFE
QUERY_NONE = 0xFFFFFFFF
N, L = far.FAR_N, 150
R = N // (L + 1)
GENOME = 100000
COUNTED = 20000
JOBS = ((12, True), (31, False), (47, True))       # (k, canonical): dense, one-word and two-word index
CHUNK = 1 << 28
MIB = 1 << 20


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype}{got.shape} against {want.dtype}{want.shape}"
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got.reshape(-1) != want.reshape(-1))[0])
        raise AssertionError(f"{what}: {int((got != want).sum())} differ, the first at {i}: {got.reshape(-1)[i]} against {want.reshape(-1)[i]}")


def _down(ctx, ptr, n, dtype):
    out = np.empty(n, dtype)
    if n:
        ctx.d2h(out, ptr)
    return out


def _up(ctx, arr):
    arr = np.ascontiguousarray(arr)
    p = ctx.alloc(max(arr.nbytes, 16))
    if arr.nbytes:
        ctx.h2d(p, arr)
    return p


class _Bufs:
    """device buffers that are freed together"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def alloc(self, nbytes):
        self.ptrs.append(self.ctx.alloc(max(int(nbytes), 16)))
        return self.ptrs[-1]

    def up(self, arr):
        self.ptrs.append(_up(self.ctx, arr))
        return self.ptrs[-1]

    def free(self):
        while self.ptrs:
            self.ctx.free(self.ptrs.pop())


def _flags(canonical):
    import cfrk_amd
    return cfrk_amd.CFRK_CANONICAL if canonical else 0


# ------------------------------------------------------------------ fixtures of part one

@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


class _Far:
    pass


@pytest.fixture(scope="module")
def buf(ctx):
    """the generator's buffer with its start / length arrays, about 300 bases patched (and put back at the end)"""
    F = _Far()
    F.d_data, F.d_start, F.d_length = ctx.alloc(N), ctx.alloc(R * 8), ctx.alloc(R * 4)
    try:
        ctx.synth_reads_device(0, R, L, GENOME, F.d_data, F.d_start, F.d_length)
        ctx.h2d(F.d_data + R * (L + 1), np.full(N - R * (L + 1), -1, np.int8))
        F.start, F.length = far.pick_reads(N, R, L, 7)
        rng = np.random.default_rng(11)
        plain = np.flatnonzero((F.length == L) & (F.start >= 1 << 31) & (F.start % (L + 1) == 0) & (F.start + L <= N))
        at = [int(F.start[i]) + int(rng.integers(0, L)) for i in rng.choice(plain, 280, replace=False)]
        # and inside the composite ranges, on bases (not terminators); in the longest one also behind its window 4 * 8192
        for s, n in far.COMPOSITES:
            at += [int(p) for p in s + rng.integers(0, n, 8) if p % (L + 1) != L]
        s, n = far.COMPOSITES[2]
        at += [int(p) for p in s + rng.integers(4 * 8192 + 100, n, 10) if p % (L + 1) != L]
        F.patched = {}
        one = np.empty(1, np.int8)
        for p in sorted(set(at)):
            ctx.d2h(one, F.d_data + p)
            F.patched[p] = int(one[0])
            assert 0 <= F.patched[p] <= 3
            ctx.h2d(F.d_data + p, np.array([(F.patched[p] + 1 + int(rng.integers(0, 3))) & 3], np.int8))
        yield F
        for p, c in F.patched.items():
            ctx.h2d(F.d_data + p, np.array([c], np.int8))
    finally:
        for p in (F.d_data, F.d_start, F.d_length):
            ctx.free(p)


def _fetch(ctx, d_data, a, b):
    """bytes [a, b) of the buffer; what lies outside [0, N) reads -1"""
    out = np.full(b - a, -1, np.int8)
    lo, hi = max(a, 0), min(b, N)
    if lo < hi:
        part = np.empty(hi - lo, np.int8)
        ctx.d2h(part, d_data + lo)
        out[lo - a:hi - a] = part
    return out


class _Set:
    pass


@pytest.fixture(scope="module")
def reads(ctx, buf):
    """the read set: its arrays on the device, and on the host the bytes of every entry, fetched at d_data + start, laid
    out as a small struct-read buffer of their own for the references (an entry without a result: no bytes)"""
    S = _Set()
    S.start, S.length, S.n = buf.start, buf.length, len(buf.start)
    S.valid = (S.start >= 0) & (S.start + S.length.astype(np.int64) <= N) & (S.length > 0)
    assert (~S.valid).sum() == 4
    S.bytes = [_fetch(ctx, buf.d_data, int(s), int(s) + int(n)) if v else np.zeros(0, np.int8)
               for s, n, v in zip(S.start, S.length, S.valid)]
    S.ldata, S.lstart, S.llength = cr.flatten(S.bytes)
    S.d_start, S.d_length = _up(ctx, S.start), _up(ctx, S.length)
    yield S
    ctx.free(S.d_start)
    ctx.free(S.d_length)


class _Job:
    pass


@pytest.fixture(scope="module")
def jobs(buf):
    """a context and a job per k over reads [0, 20 000), exported once: as arrays and as the references' dict"""
    import cfrk_amd
    out = {}
    try:
        for k, canonical in JOBS:
            J = _Job()
            J.k, J.canonical = k, canonical
            J.ctx = cfrk_amd.Context(0)
            out[k] = J
            # (counted through the HBM table: the partitioned paths' pools, a GiB and more per context, would take the
            #  three jobs and the read query's 5 N bytes past 24 GiB; the counting paths are not under test here)
            J.g = cfrk_amd.GlobalCounter(J.ctx, k, _flags(canonical) | cfrk_amd.CFRK_FORCE_HASH, 1 << 20)
            J.g.add_device(buf.d_data, COUNTED * (L + 1))
            J.want = J.g.export()
            lo, hi, cnt = J.want
            J.counts = {int(a) | (int(b) << 64): int(c) for a, b, c in zip(lo.tolist(), hi.tolist(), cnt.tolist())}
            assert len(J.counts) > GENOME // 2
        yield out
    finally:
        for J in out.values():
            J.ctx.close()


def _window_counts(S, J):
    """(count, valid) of the window at every byte of the set's own buffer"""
    return fr.window_counts(S.ldata, J.k, J.canonical, J.want)


# ------------------------------------------------------------------ part one: one device form per test

def _layers(S):
    """the entries in groups whose ranges (terminator included) do not overlap; an entry without a range goes anywhere"""
    layers, ends = [], []
    for i in np.argsort(S.start, kind="stable"):
        if not S.valid[i]:
            continue
        for j, e in enumerate(ends):
            if e <= S.start[i]:
                break
        else:
            layers.append([])
            ends.append(0)
            j = len(ends) - 1
        layers[j].append(int(i))
        ends[j] = int(S.start[i]) + int(S.length[i]) + 1
    layers[0] += [int(i) for i in np.flatnonzero(~S.valid)]
    return [np.array(sorted(x), np.int64) for x in layers]


def test_per_read_sparse_device(buf, reads):
    """k = 12 canonical and k = 31 forward, on one context of its own: its pool (12 bytes per byte of nN) is taken once
    and given back when the context closes"""
    import cfrk_amd
    S = reads
    layers = _layers(S)
    assert sum(len(x) for x in layers) == S.n and 2 <= len(layers) <= 4
    sctx = cfrk_amd.Context(0)
    B = _Bufs(sctx)
    try:
        for (k, canonical), layer in ((kc, layer) for kc in ((12, True), (31, False)) for layer in layers):
            nS = len(layer)
            d_s, d_l, d_rp = B.up(S.start[layer]), B.up(S.length[layer]), B.alloc((nS + 1) * 8)
            args = (buf.d_data, d_s, d_l, N, nS, k, _flags(canonical), d_rp)
            with pytest.raises(cfrk_amd.CfrkError) as e:
                sctx.per_read_sparse_device(*args, 0, 0, 0)
            assert e.value.code == CFRK_ERR_SMALL_BUF
            nnz = e.value.nnz
            d_k, d_c = B.alloc(nnz * 8), B.alloc(nnz * 4)
            assert sctx.per_read_sparse_device(*args, d_k, d_c, nnz) == nnz
            row_ptr, keys, counts = _down(sctx, d_rp, nS + 1, np.int64), _down(sctx, d_k, nnz, np.uint64), _down(sctx, d_c, nnz, np.uint32)
            rows = [sorted(collections.Counter(nr.read_keys(S.bytes[i], 0, len(S.bytes[i]), k, canonical)).items()) for i in layer]
            w_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
            _same(row_ptr, w_ptr, f"k={k} row_ptr")
            _same(keys, np.array([x for r in rows for x, _ in r], np.uint64), f"k={k} keys")
            _same(counts, np.array([c for r in rows for _, c in r], np.uint32), f"k={k} counts")
            assert all(w_ptr[j] == w_ptr[j + 1] for j, i in enumerate(layer) if not S.valid[i])
            B.free()
    finally:
        B.free()
        sctx.close()


def test_per_read_dense_device_k4(ctx, buf, reads):
    """Native mode.  The dense form is defined on the struct-read layout, where a terminator (or the buffer's end) lies
    behind every read: the reference's kernel visits that byte as a window start too, the product does not, and they
    agree because no window begins on a terminator.  So for this call the composite ranges are lengthened to the next
    terminator of the generator (they lie across as many terminators as before and stay in their size classes), and the
    four entries without a range in the layout are left out.  A window of the read's last k - 1 positions takes in the
    bytes behind the read: the set's bytes are fetched again with those."""
    k, S = 4, reads
    take = np.flatnonzero(S.valid)
    length = S.length[take].copy()
    ends = S.start[take] + length
    inside = ends < R * (L + 1)
    length[inside] += ((L - ends[inside]) % (L + 1)).astype(np.int32)
    assert (length >= S.length[take]).all() and ((length != S.length[take]).sum() == 3)
    assert (((S.start[take] + length)[inside] % (L + 1)) == L).all()
    pieces = [_fetch(ctx, buf.d_data, int(s), int(s) + int(n) + k - 1) for s, n in zip(S.start[take], length)]
    ldata = np.concatenate(pieces + [np.full(8, -1, np.int8)])
    lstart = np.concatenate([[0], np.cumsum([len(p) for p in pieces])[:-1]]).astype(np.int64)
    want = orc.per_read_dense(ldata, lstart, length, k, 0)
    B = _Bufs(ctx)
    try:
        d_s, d_l, d_f = B.up(S.start[take]), B.up(length), B.alloc(len(take) * 4 ** k * 4)
        vp = C.c_void_p
        ctx.check(ctx._L.cfrk_per_read_dense_device(ctx._h, vp(buf.d_data), vp(d_s), vp(d_l), N, len(take), k, 0, vp(d_f)),
                  "cfrk_per_read_dense_device")
        got = _down(ctx, d_f, len(take) * 4 ** k, np.int32).reshape(len(take), 4 ** k)
    finally:
        B.free()
    _same(got, want.reshape(got.shape).astype(np.int32), "dense rows")
    assert got.sum() > 0.9 * (length.astype(np.int64).sum() - (k - 1) * len(take))


def _stats_want(S, J, threshold):
    import cfrk_amd
    counts, valid = _window_counts(S, J)
    out = np.zeros(S.n, cfrk_amd.READ_STATS_DTYPE)
    for i in range(S.n):
        m = max(int(S.llength[i]) - J.k + 1, 0)
        s = int(S.lstart[i])
        c = np.sort(counts[s:s + m][valid[s:s + m]].astype(np.uint64))
        if len(c):
            out[i] = (len(c), (c >= 1).sum(), (c < threshold).sum(), c[0], c[(len(c) - 1) // 2], c[-1], c.sum())
    return out


@pytest.mark.parametrize("k", [12, 31, 47])
def test_read_stats_device(buf, reads, jobs, k):
    import cfrk_amd
    S, J = reads, jobs[k]
    d_out = J.ctx.alloc(S.n * 32)
    try:
        for threshold in (2, 12):
            J.g.read_stats_device(buf.d_data, S.d_start, S.d_length, N, S.n, threshold, d_out)
            got = _down(J.ctx, d_out, S.n, cfrk_amd.READ_STATS_DTYPE)
            want = _stats_want(S, J, threshold)
            _same(got, want, f"k={k} threshold={threshold}")
            assert (want["windows"][~S.valid] == 0).all() and 0 < (want["below"] > 0).sum() < S.n
    finally:
        J.ctx.free(d_out)


def _spans_want(S, J, min_count, mode):
    counts, valid = _window_counts(S, J)
    return fr.ref_spans(S.ldata, S.lstart, S.llength, J.k, min_count, COUNT_MAX, mode, counts, valid)


@pytest.mark.parametrize("k", [12, 31, 47])
def test_read_spans_device(buf, reads, jobs, k):
    import cfrk_amd
    S, J = reads, jobs[k]
    d_out = J.ctx.alloc(S.n * 8)
    try:
        for mode in (cfrk_amd.CFRK_SPAN_PREFIX, cfrk_amd.CFRK_SPAN_LONGEST):
            J.g.read_spans_device(buf.d_data, S.d_start, S.d_length, N, S.n, 2, COUNT_MAX, mode, d_out)
            got = _down(J.ctx, d_out, S.n, cfrk_amd.READ_SPAN_DTYPE)
            want = _spans_want(S, J, 2, mode)
            _same(got, want.astype(cfrk_amd.READ_SPAN_DTYPE), f"k={k} mode={mode}")
            assert (want["length"][~S.valid] == 0).all()
            trimmed = (want["length"] < S.length) & S.valid
            assert 100 < trimmed.sum() < S.n - 100, "the patched bases cut spans short, most reads are whole"
    finally:
        J.ctx.free(d_out)


@pytest.mark.parametrize("k", [12, 31, 47])
def test_correct_reads_device(buf, reads, jobs, k):
    """every read sees the input buffer, so the reads of the set that overlap (the composite ranges and the generator's
    reads under them) are corrected independently and data_out holds the union of their fixes; the reference's fixes of
    two overlapping reads never name one byte with two different bases (asserted: a property of the set, not of the
    code under test)"""
    S, J, mn = reads, jobs[k], 3
    fix_want = np.zeros(S.n, cr.FIX_DTYPE)
    fixes = {}
    for i in np.flatnonzero(S.valid):
        codes = S.bytes[i].tolist()
        out, f, l = cr.correct_codes(codes, k, J.canonical, J.counts, mn)
        fix_want[i] = (f, l)
        for p, (a, b) in enumerate(zip(codes, out)):
            if a != b:
                assert fixes.setdefault(int(S.start[i]) + p, b) == b
    assert len(fixes) > 100 and fix_want["left"].sum() > 0
    long_i = int(np.flatnonzero(S.length == far.COMPOSITES[2][1])[0])
    assert any(p - far.COMPOSITES[2][0] > 4 * 8192 for p in fixes), "a fix behind the long read's fourth round"
    assert fix_want[long_i]["fixed"] > 0

    def expect(a, b):
        want = _fetch(J.ctx, buf.d_data, a, b)
        for p, c in fixes.items():
            if a <= p < b:
                want[p - a] = c
        return want

    d_out, d_fix = J.ctx.alloc(N), J.ctx.alloc(S.n * 8)
    try:
        J.g.correct_reads_device(buf.d_data, S.d_start, S.d_length, N, S.n, mn, d_out, d_fix)
        _same(_down(J.ctx, d_fix, S.n, cr.FIX_DTYPE), fix_want, f"k={k} fix rows")
        for i in np.flatnonzero(S.valid):
            a, b = int(S.start[i]), int(S.start[i]) + int(S.length[i])
            got = _down(J.ctx, d_out + a, b - a, np.int8)
            want = S.bytes[i].copy()
            for p in range(a, b):
                if p in fixes:
                    want[p - a] = fixes[p]
            _same(got, want, f"k={k} read {i} at {a}")
        for mid in (1 << 31, 1 << 32, N - MIB // 2):
            a = mid - MIB // 2
            _same(_down(J.ctx, d_out + a, MIB, np.int8), expect(a, a + MIB), f"k={k} data_out[{a} .. +1 MiB)")
    finally:
        J.ctx.free(d_out)
        J.ctx.free(d_fix)


@pytest.fixture(scope="module")
def set_keys(reads):
    return {k: nr.all_read_keys(reads.ldata, reads.lstart, reads.llength, k, canonical) for k, canonical in JOBS[1:]}


@pytest.mark.parametrize("batch", [64, 2048])
@pytest.mark.parametrize("k", [31, 47])
def test_normalize_device_and_pairs(buf, reads, jobs, set_keys, k, batch):
    """a fresh job over the same 20 000 reads per call (the call adds what it keeps); the set in consecutive twos for
    the paired calls"""
    import cfrk_amd
    S, J = reads, jobs[k]
    # the median count of the job's keys (30-fold coverage by reads of 150 - k + 1 windows; a forward key sees one
    # strand): about half of the set's reads lie below it
    cutoff = 22 if J.canonical else 12
    nctx = cfrk_amd.Context(0)
    d_keep = nctx.alloc(S.n)
    try:
        for mode in (None, cfrk_amd.CFRK_PAIR_BOTH, cfrk_amd.CFRK_PAIR_EITHER):
            g = cfrk_amd.GlobalCounter(nctx, k, _flags(J.canonical), 1 << 20)
            g.add_device(buf.d_data, COUNTED * (L + 1))
            nctx.h2d(d_keep, np.full(S.n, 7, np.uint8))
            if mode is None:
                n_kept = g.normalize_device(buf.d_data, S.d_start, S.d_length, N, S.n, cutoff, d_keep, batch)
                keep, w_kept, counts = nr.normalize_keys(set_keys[k], cutoff, batch, dict(J.counts))
            else:
                n_kept = g.normalize_pairs_device(buf.d_data, S.d_start, S.d_length, N, S.n, cutoff, d_keep, batch, mode)
                keep, w_kept, counts = pr.normalize_pairs_keys(set_keys[k], cutoff, batch, mode, dict(J.counts))
            what = f"k={k} batch={batch} mode={mode}"
            _same(_down(nctx, d_keep, S.n, np.uint8), keep, what + " keep")
            assert n_kept == w_kept and 50 < w_kept < S.n - 50, what
            for got, want, name in zip(g.export(), nr.export_arrays(counts), ("lo", "hi", "count")):
                _same(got, want, f"{what} export {name}")
    finally:
        nctx.free(d_keep)
        nctx.close()


# ------------------------------------------------------------------ part two: whole buffers

def test_query_reads_device_whole_buffer(buf, jobs):
    """4 N bytes of counts; checked at both seams, at the end and in 64 blocks of 4 096 windows above 2^31"""
    rng = np.random.default_rng(3)
    ranges = [((1 << 31) - (1 << 16), (1 << 31) + (1 << 16)), ((1 << 32) - (1 << 16), (1 << 32) + (1 << 16)), (N - (1 << 16), N)]
    ranges += [(int(a), int(a) + 4096) for a in rng.integers(1 << 31, N - 4096, 64)]
    J0 = jobs[JOBS[0][0]]
    d_out = J0.ctx.alloc(4 * N)
    try:
        for k, _ in JOBS:
            J = jobs[k]
            J.ctx.h2d(d_out + 4 * (N - 64), np.zeros(64, np.uint32))
            J.g.query_reads_device(buf.d_data, N, d_out)
            for a, b in ranges:
                data = _fetch(J.ctx, buf.d_data, a, min(b + k - 1, N))
                want = _want_reads(data, k, J.canonical, J.want)[:b - a]
                _same(_down(J.ctx, d_out + 4 * a, b - a, np.uint32), want, f"k={k} counts[{a}:{b}]")
                if b == N:
                    assert (want[-(k - 1):] == QUERY_NONE).all()
                else:
                    assert (want != QUERY_NONE).sum() > (b - a) // 2
            J.ctx.sync()
    finally:
        J0.ctx.free(d_out)


@pytest.mark.parametrize("k,canonical", [(21, True), (47, False)])
def test_distinct_sketch_device_whole_buffer(ctx, buf, k, canonical):
    """The registers over N bytes equal the maximum-merge of the sketches of five consecutive pieces, each cut at a read
    boundary (a multiple of 16 reads, for the 16-byte alignment the call asks for), shorter than 2^31 bytes and taken at
    d_data + offset, so that each piece's call sees small offsets only.  The pieces are the code under test as well, at
    sizes tests/test_gpu_sketch.py already pins to tests/sketch_ref.py.  The generator writes no invalid base, so the
    windows are R (150 - k + 1) by its rule."""
    import cfrk_amd
    cuts = [(R * j // 5) // 16 * 16 * (L + 1) for j in range(5)] + [N]
    assert all(0 < b - a < 1 << 31 and a % 16 == 0 for a, b in zip(cuts, cuts[1:]))
    zero = np.zeros(cfrk_amd.CFRK_SKETCH_REGS, np.uint8)
    d_regs = ctx.alloc(cfrk_amd.CFRK_SKETCH_REGS)
    try:
        ctx.h2d(d_regs, zero)
        windows = ctx.distinct_sketch_device(buf.d_data, N, k, _flags(canonical), d_regs)
        whole = _down(ctx, d_regs, len(zero), np.uint8)
        merged, total = zero.copy(), 0
        for a, b in zip(cuts, cuts[1:]):
            ctx.h2d(d_regs, zero)
            total += ctx.distinct_sketch_device(buf.d_data + a, b - a, k, _flags(canonical), d_regs)
            cfrk_amd.sketch_merge(merged, _down(ctx, d_regs, len(zero), np.uint8))
    finally:
        ctx.free(d_regs)
    assert windows == total == R * (L - k + 1)
    _same(whole, merged, "registers")
    # both strands of the genome (canonical: one key for the two), and at most k new keys per patched base; five standard
    # errors of the estimate are 4 %
    distinct = GENOME if canonical else 2 * GENOME
    assert 0.95 * distinct < cfrk_amd.sketch_estimate(whole) < 1.05 * (distinct + k * len(buf.patched))


def _select_all(ctx, buf, keep, spans, period):
    """cfrk_reads_select_device over all R reads -> checked whole against the (R, 151) matrix of the input: the kept
    bytes of the matrix in row-major order ARE data_out.  keep and spans repeat every `period` reads."""
    import cfrk_amd
    B = _Bufs(ctx)
    try:
        d_keep = B.up(keep) if keep is not None else 0
        d_span = B.up(spans) if spans is not None else 0
        w_start, w_length, w_index, w_nN, w_nS = far.select_expect(np.arange(R, dtype=np.int64) * (L + 1), np.full(R, L, np.int32),
                                                                   keep, spans, 0, N)
        d_data_out, d_so, d_lo, d_io = B.alloc(w_nN), B.alloc(w_nS * 8), B.alloc(w_nS * 4), B.alloc(w_nS * 8)
        got = ctx.select_reads_device(buf.d_data, buf.d_start, buf.d_length, N, R, d_span, d_keep, 0, d_data_out, w_nN, d_so, d_lo, d_io, w_nS)
        assert got == (w_nN, w_nS)
        _same(_down(ctx, d_so, w_nS, np.int64), w_start, "start_out")
        _same(_down(ctx, d_lo, w_nS, np.int32), w_length, "length_out")
        _same(_down(ctx, d_io, w_nS, np.int64), w_index, "index_out")
        out = _down(ctx, d_data_out, w_nN, np.int8)
        assert (out[w_start + w_length] == -1).all(), "every output read ends on a terminator"
        # keep and spans repeat every `period` reads, so the expected bytes of `period` reads are the same slices of
        # their rows all along: a few hundred strided copies per chunk instead of a mask over every byte
        keep_p = np.ones(period, np.uint8) if keep is None else keep[:period]
        off_p = np.zeros(period, np.int64) if spans is None else spans["offset"][:period].astype(np.int64)
        n_p = np.full(period, L, np.int64) if spans is None else spans["length"][:period].astype(np.int64)
        whole = R // period * period
        if keep is not None:
            assert (keep[:whole].reshape(-1, period) == keep_p).all()
        if spans is not None:
            assert (spans[:whole].reshape(-1, period) == spans[:period]).all()
        width = int(((n_p + 1) * (keep_p != 0)).sum())
        per_chunk, pos = max((1 << 21) // period, 1), 0
        for r0 in range(0, R, per_chunk * period):
            r1 = min(r0 + per_chunk * period, R)
            block = _down(ctx, buf.d_data + r0 * (L + 1), (r1 - r0) * (L + 1), np.int8)
            m = (r1 - r0) // period
            rows3 = block[:m * period * (L + 1)].reshape(m, period, L + 1)
            want = np.empty((m, width), np.int8)
            o = 0
            for r in np.flatnonzero(keep_p):
                a, n = int(off_p[r]), int(n_p[r])
                want[:, o:o + n] = rows3[:, r, a:a + n]
                want[:, o + n] = rows3[:, r, L]
                o += n + 1
            assert o == width
            _same(out[pos:pos + want.size], want.reshape(-1), f"data_out for reads [{r0}, {r0 + m * period})")
            pos += want.size
            for r in range(r0 + m * period, r1):                  # the last reads, fewer than a period
                if keep_p[(r - r0) % period]:
                    a, n = int(off_p[(r - r0) % period]), int(n_p[(r - r0) % period])
                    row = block[(r - r0) * (L + 1):(r - r0 + 1) * (L + 1)]
                    _same(out[pos:pos + n + 1], np.concatenate([row[a:a + n], row[L:]]), f"data_out for read {r}")
                    pos += n + 1
        assert pos == w_nN
        return w_nN
    finally:
        B.free()


def test_select_reads_device_all_reads_dropped_and_trimmed(ctx, buf):
    """every 97th read dropped, 10 bases trimmed off every 5th (3 in front, 7 behind).  The output is 0.977 N bytes: it
    passes 2^31 and ends short of 2^32 -- the next test's output passes 2^32."""
    import cfrk_amd
    keep = (np.arange(R) % 97 != 0).astype(np.uint8)
    spans = np.zeros(R, cfrk_amd.READ_SPAN_DTYPE)
    spans["length"] = L
    spans["offset"][::5], spans["length"][::5] = 3, L - 10
    assert _select_all(ctx, buf, keep, spans, 97 * 5) > 1 << 31


def test_select_reads_device_all_reads_output_past_4gib(ctx, buf):
    """every read kept whole (no keep array, no spans): the output is the R reads, R * 151 = N - 36 bytes"""
    assert _select_all(ctx, buf, None, None, 1) == R * (L + 1) > 1 << 32


# ------------------------------------------------------------------ the FASTQ text of more than 2^32 bytes

FASTQ_LENGTHS = (150, 1, 37, 150, 400, 2, 3000, 211, 16, 150, 15, 17, 150, 93, 150, 150, 333, 64, 150, 3000, 150, 7, 150, 299)


class _Text:
    pass


@pytest.fixture(scope="module")
def fastq_text(ctx):
    T = _Text()
    T.block = far.fastq_block(5, FASTQ_LENGTHS)
    assert len(FASTQ_LENGTHS) % 2 == 0 and len(T.block) % 2 == 1
    T.reps = -(-N // len(T.block))
    T.nbytes = T.reps * len(T.block)
    T.host = far.tiled_text(T.block, T.reps)
    T.d_text = ctx.alloc(T.nbytes)
    try:
        ctx.h2d(T.d_text, T.host)
        T.rows = far.tiled_index_expect(tr.index_ref(T.block, tr.TEXT_FASTQ), len(T.block), T.reps)
        yield T
    finally:
        ctx.free(T.d_text)
        T.host = None


def _parse_whole(ctx, call, want, what):
    """call(d_data, cap_data, d_start, d_length, cap_reads) -> (nN, nS) against want = far_ref's five; the position arrays
    whole, data whole in chunks.  Returns the buffers (the caller frees them)."""
    w_start, w_length, w_nN, w_nS, data_range = want
    B = _Bufs(ctx)
    try:
        d_data, d_start, d_length = B.alloc(w_nN), B.alloc(w_nS * 8), B.alloc(w_nS * 4)
        assert call(d_data, w_nN, d_start, d_length, w_nS) == (w_nN, w_nS), what
        _same(_down(ctx, d_start, w_nS, np.int64), w_start, what + " start")
        _same(_down(ctx, d_length, w_nS, np.int32), w_length, what + " length")
        for a in range(0, w_nN, CHUNK):
            b = min(a + CHUNK, w_nN)
            _same(_down(ctx, d_data + a, b - a, np.int8), data_range(a, b), f"{what} data[{a}:{b}]")
    except BaseException:
        B.free()
        raise
    return B, d_data, d_start, d_length


def test_fastq_text_parse_index_and_emit_round_trip(ctx, fastq_text):
    """parse (min_qual 0) and index are checked whole against far_ref; the emitter, given all reads with whole spans,
    must write the input text back byte for byte: its oracle is the text itself"""
    import cfrk_amd
    T = fastq_text
    want = far.tiled_fastq_expect(T.block, fq.parse(T.block, 0)[1:], T.reps)
    assert T.nbytes >= N
    B, d_data, d_start, d_length = _parse_whole(ctx, lambda *a: ctx.parse_fastq_device(T.d_text, T.nbytes, 0, *a), want, "min_qual 0")
    try:
        nS = want[3]
        d_rec = B.alloc(nS * 24)
        assert ctx.index_text_device(T.d_text, T.nbytes, cfrk_amd.CFRK_TEXT_FASTQ, d_rec, nS) == nS
        _same(_down(ctx, d_rec, nS, cfrk_amd.TEXT_RECORD_DTYPE), T.rows.astype(cfrk_amd.TEXT_RECORD_DTYPE), "index rows")
        assert T.rows["head_off"][-1] > 1 << 32 and T.rows["qual_off"][-1] > 1 << 32
        d_out = B.alloc(T.nbytes)
        got = ctx.emit_reads_device(d_data, d_start, d_length, want[2], nS, 0, 0, 0, T.d_text, T.nbytes, d_rec, cfrk_amd.CFRK_TEXT_FASTQ,
                                    d_out, T.nbytes)
        assert got == (T.nbytes, nS)
        for a in range(0, T.nbytes, CHUNK):
            b = min(a + CHUNK, T.nbytes)
            _same(_down(ctx, d_out + a, b - a, np.uint8), T.host[a:b], f"emitted text[{a}:{b}]")
    finally:
        B.free()


def test_fastq_text_min_qual_20(ctx, fastq_text):
    T = fastq_text
    masked = fq.parse(T.block, 20)[1:]
    assert (masked[0] == -1).sum() > 2 * len(FASTQ_LENGTHS)
    want = far.tiled_fastq_expect(T.block, masked, T.reps)
    B = _parse_whole(ctx, lambda *a: ctx.parse_fastq_device(T.d_text, T.nbytes, 20, *a), want, "min_qual 20")[0]
    B.free()


def _far_rows(T, lengths):
    """for every length a record of the text whose header begins at or above 2^32 -- one with as many bases where the
    text has such records (150), any other otherwise"""
    first = int(np.searchsorted(T.rows["head_off"], 1 << 32))
    far_rows = T.rows[first:]
    assert len(far_rows) > 1000
    by_len = {}
    for j, q in enumerate(far_rows["qual_len"][:20 * len(FASTQ_LENGTHS)].tolist()):
        by_len.setdefault(q, []).append(j)
    pick, used = [], collections.Counter()
    for n in lengths.tolist():
        cand = by_len.get(n) or by_len[max(by_len)]
        pick.append(cand[used[n] % len(cand)])
        used[n] += 1
    return far_rows[np.array(pick)], first


def test_select_and_emit_device_far_reads_far_records(buf, reads, jobs, fastq_text):
    """the set's reads selected and emitted with the spans of the span test (k = 31, longest run, min_count 2) and keep
    bytes from them; the emitter's records lie in the text at 2^32 and above.  The outputs are small and checked whole"""
    import cfrk_amd
    S, J, T = reads, jobs[31], fastq_text
    ctx = J.ctx
    spans = _spans_want(S, J, 2, cfrk_amd.CFRK_SPAN_LONGEST).astype(cfrk_amd.READ_SPAN_DTYPE)
    keep = ((spans["length"] > 0) & (np.arange(S.n) % 7 != 3)).astype(np.uint8)
    keep[~S.valid] = 1                                     # (the calls drop them by their ranges)
    min_len = 40
    rec, _ = _far_rows(T, S.length)
    base = int(rec["head_off"].min()) // len(T.block) * len(T.block)
    span = int((rec["qual_off"] + rec["qual_len"]).max()) + 1 - base
    ltext = T.host[base:base + span].tobytes()
    lrec = rec.copy()
    lrec["head_off"] -= base
    lrec["qual_off"] -= base
    lkeep = keep.copy()
    lkeep[~S.valid] = 0
    B = _Bufs(ctx)
    try:
        d_span, d_keep, d_rec = B.up(spans), B.up(keep), B.up(rec.astype(cfrk_amd.TEXT_RECORD_DTYPE))
        # select
        w_data, w_start, w_length, w_index = fr.ref_select(S.ldata, S.lstart, S.llength, spans, lkeep, min_len)
        e_start, e_length, e_index, e_nN, e_nS = far.select_expect(S.start, S.length, keep, spans, min_len, N)
        _same(e_index, w_index, "far_ref.select_expect against filter_ref")
        assert 1000 < e_nS < S.n - 100
        d_do, d_so, d_lo, d_io = B.alloc(e_nN), B.alloc(e_nS * 8), B.alloc(e_nS * 4), B.alloc(e_nS * 8)
        assert ctx.select_reads_device(buf.d_data, S.d_start, S.d_length, N, S.n, d_span, d_keep, min_len, d_do, e_nN, d_so, d_lo, d_io,
                                       e_nS) == (e_nN, e_nS)
        _same(_down(ctx, d_so, e_nS, np.int64), w_start, "start_out")
        _same(_down(ctx, d_lo, e_nS, np.int32), w_length, "length_out")
        _same(_down(ctx, d_io, e_nS, np.int64), w_index, "index_out")
        _same(_down(ctx, d_do, e_nN, np.int8), w_data, "data_out")
        # emit, both formats
        for fmt in (cfrk_amd.CFRK_TEXT_FASTA, cfrk_amd.CFRK_TEXT_FASTQ):
            w_text, w_idx = tr.emit_ref(S.ldata, S.lstart, S.llength, ltext, lrec, spans, lkeep, min_len, fmt)
            assert len(w_idx) > 1000
            args = (buf.d_data, S.d_start, S.d_length, N, S.n, d_span, d_keep, min_len, T.d_text, T.nbytes, d_rec, fmt)
            with pytest.raises(cfrk_amd.CfrkError) as e:
                ctx.emit_reads_device(*args, 0, 0)
            assert e.value.code == CFRK_ERR_SMALL_BUF and (e.value.nbytes, e.value.nS) == (len(w_text), len(w_idx))
            d_out = B.alloc(len(w_text))
            assert ctx.emit_reads_device(*args, d_out, len(w_text)) == (len(w_text), len(w_idx))
            assert _down(ctx, d_out, len(w_text), np.uint8).tobytes() == w_text, f"emitted text, format {fmt}"
    finally:
        B.free()


def test_check_pairs_device_far_records(ctx, fastq_text):
    """500 interleaved pairs whose records lie at 2^32 and above (the text has about 1 400 records there); two of them get
    unequal names by a one-byte patch of the text (undone at the end)"""
    import cfrk_amd
    T = fastq_text
    first = int(np.searchsorted(T.rows["head_off"], 1 << 32))
    first += first % 2
    rec = T.rows[first:first + 1000]
    assert len(rec) == 1000 and rec["head_off"][0] >= 1 << 32
    base = int(rec["head_off"][0])
    local = bytearray(T.host[base:int(rec["qual_off"][-1] + rec["qual_len"][-1]) + 1].tobytes())
    lrec = rec.copy()
    lrec["head_off"] -= base
    lrec["qual_off"] -= base
    assert pr.check_pairs(local, lrec[0::2], local, lrec[1::2]) == (-1, 0)
    d_rec = _up(ctx, rec.astype(cfrk_amd.TEXT_RECORD_DTYPE))
    args = (len(rec) // 2, 2, T.d_text, T.nbytes, d_rec, T.d_text, T.nbytes, d_rec + 24)
    patched = [int(rec["head_off"][2 * j + side]) + 2 for j, side in ((413, 0), (207, 1))]
    try:
        assert ctx.check_pairs_device(*args) == (-1, 0)
        for p in patched:
            assert chr(local[p - base]).isdigit()
            local[p - base] = ord("Z")
            ctx.h2d(T.d_text + p, np.array([ord("Z")], np.uint8))
        assert pr.check_pairs(local, lrec[0::2], local, lrec[1::2]) == (207, 2)
        assert ctx.check_pairs_device(*args) == (207, 2)
    finally:
        for p in patched:
            ctx.h2d(T.d_text + p, T.host[p:p + 1])
        ctx.free(d_rec)


# ------------------------------------------------------------------ the FASTA text whose parsed data pass 2^32

def test_fasta_text_parsed_data_past_4gib(ctx):
    import cfrk_amd
    block = far.fasta_block(3, 200)
    rc, parse = ic.host_parse(block, ic.NATIVE)
    assert rc == 0
    reps = -(-N // len(parse[0]))
    nbytes = reps * len(block)
    assert N <= reps * len(parse[0]) and nbytes < 1.08 * N
    host = far.tiled_text(block, reps)
    d_text = ctx.alloc(nbytes)
    B = None
    try:
        ctx.h2d(d_text, host)
        host = None
        want = far.tiled_fasta_expect(block, parse, reps)
        B, d_data, d_start, d_length = _parse_whole(ctx, lambda *a: ctx.parse_fasta_device(d_text, nbytes, 0, *a), want, "native")
        B.free()
        nS = want[3]
        d_rec = B.alloc(nS * 24)
        assert ctx.index_text_device(d_text, nbytes, cfrk_amd.CFRK_TEXT_FASTA, d_rec, nS) == nS
        rows = far.tiled_index_expect(tr.index_ref(block, tr.TEXT_FASTA), len(block), reps)
        _same(_down(ctx, d_rec, nS, cfrk_amd.TEXT_RECORD_DTYPE), rows.astype(cfrk_amd.TEXT_RECORD_DTYPE), "index rows")
        B.free()
        # compat mode on a prefix of whole blocks of 2^31 + 2^20 bytes or more
        rc, cparse = ic.host_parse(block, ic.COMPAT)
        assert rc == 0
        creps = -(-((1 << 31) + MIB) // len(block))
        cwant = far.tiled_fasta_expect(block, cparse, creps)
        B = _parse_whole(ctx, lambda *a: ctx.parse_fasta_device(d_text, creps * len(block), cfrk_amd.CFRK_COMPAT, *a), cwant, "compat")[0]
    finally:
        if B is not None:
            B.free()
        ctx.free(d_text)


# ------------------------------------------------------------------ the branches behind nbytes > 2^31 - 1

def _long_text(ctx, head, fill, n_fill, tail):
    """head + n_fill bytes of `fill` + tail on the device -> (d_text, nbytes); never a Python string of that size"""
    nbytes = len(head) + n_fill + len(tail)
    host = np.full(nbytes, ord(fill), np.uint8)
    host[:len(head)] = np.frombuffer(head, np.uint8)
    host[nbytes - len(tail):] = np.frombuffer(tail, np.uint8)
    d_text = ctx.alloc(nbytes)
    try:
        ctx.h2d(d_text, host)
    except BaseException:
        ctx.free(d_text)
        raise
    return d_text, nbytes


def test_fasta_record_of_2_to_31_bases_is_refused_and_one_base_less_is_parsed(ctx):
    import cfrk_amd
    tail = b"\n>r1\nACGT\n>r2\nGG\n"
    for n_bases, ok in ((1 << 31, False), ((1 << 31) - 1, True)):
        d_text, nbytes = _long_text(ctx, b">r0\n", "C", n_bases, tail)
        B = _Bufs(ctx)
        try:
            nN, nS = n_bases + 1 + 5 + 3, 3
            d_data, d_start, d_length = B.alloc(nN), B.alloc(nS * 8), B.alloc(nS * 4)
            call = lambda: ctx.parse_fasta_device(d_text, nbytes, 0, d_data, nN, d_start, d_length, nS)
            if not ok:
                with pytest.raises(cfrk_amd.CfrkError) as e:
                    call()
                assert e.value.code == CFRK_ERR_LAYOUT and "record 0 " in str(e.value) and "2^31 - 1" in str(e.value)
                continue
            assert call() == (nN, nS)
            _same(_down(ctx, d_start, nS, np.int64), np.array([0, n_bases + 1, n_bases + 6], np.int64), "start")
            _same(_down(ctx, d_length, nS, np.int32), np.array([n_bases, 4, 2], np.int32), "length")
            assert n_bases == 2 ** 31 - 1
            _same(_down(ctx, d_data, 4096, np.int8), np.full(4096, 1, np.int8), "the record's first codes")
            end = np.concatenate([np.full(4096, 1, np.int8), np.array([-1, 0, 1, 2, 3, -1, 2, 2, -1], np.int8)])
            _same(_down(ctx, d_data + nN - len(end), len(end), np.int8), end, "the last codes")
        finally:
            B.free()
            ctx.free(d_text)


def test_fastq_record_of_2_to_31_bases_is_refused(ctx):
    import cfrk_amd
    n = 1 << 31
    head, mid = b"@r0\n", b"\n+\n"
    nbytes = len(head) + n + len(mid) + n + 1
    host = np.full(nbytes, ord("G"), np.uint8)
    host[:len(head)] = np.frombuffer(head, np.uint8)
    host[len(head) + n:len(head) + n + len(mid)] = np.frombuffer(mid, np.uint8)
    host[len(head) + n + len(mid):] = ord("I")
    host[-1] = 10
    d_text = ctx.alloc(nbytes)
    B = _Bufs(ctx)
    try:
        ctx.h2d(d_text, host)
        host = None
        d_data, d_start, d_length = B.alloc(n + 1), B.alloc(8), B.alloc(4)
        with pytest.raises(cfrk_amd.CfrkError) as e:
            ctx.parse_fastq_device(d_text, nbytes, 0, d_data, n + 1, d_start, d_length, 1)
        assert e.value.code == CFRK_ERR_LAYOUT and "record 0 " in str(e.value) and "2^31 - 1" in str(e.value)
    finally:
        B.free()
        ctx.free(d_text)


def test_text_index_header_line_of_2_to_31_bytes_is_refused_and_one_byte_less_is_exact(ctx):
    import cfrk_amd
    head, tail = b">a\nACGT\n>", b"\nACGT\n>c\nTT\n"
    for n_line, ok in ((1 << 31, False), ((1 << 31) - 1, True)):
        d_text, nbytes = _long_text(ctx, head, "h", n_line - 1, tail)
        d_rec = ctx.alloc(3 * 24)
        try:
            call = lambda: ctx.index_text_device(d_text, nbytes, cfrk_amd.CFRK_TEXT_FASTA, d_rec, 3)
            if not ok:
                with pytest.raises(cfrk_amd.CfrkError) as e:
                    call()
                assert e.value.code == CFRK_ERR_LAYOUT and "record 1 " in str(e.value)
                continue
            assert call() == 3
            at = len(head) - 1
            want = np.array([(0, -1, 2, 0), (at, -1, n_line, 0), (at + n_line + 1 + 5, -1, 2, 0)], cfrk_amd.TEXT_RECORD_DTYPE)
            _same(_down(ctx, d_rec, 3, cfrk_amd.TEXT_RECORD_DTYPE), want, "rows")
        finally:
            ctx.free(d_rec)
            ctx.free(d_text)
