"""GPU: the read filter against a finished global result -- solid spans (cfrk_global_read_spans / _device) against numpy
over tests.oracle_lib.global_count on a k grid, both modes, four threshold settings, lane seams at every residue modulo
64, the long-read path, out-of-range reads, errors; the select (cfrk_reads_select / _device) against plain array
slicing: every length class around the copy's tile, every mutual misalignment, the seams of the output tiles and of the
tile scan, capacities, guard bytes; then the chain text -> parse -> count -> spans -> select -> second count on the
device, and the CLI's --filter-out.  The references are tests/filter_ref.py; the library's own calls are never the
reference."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from . import filter_ref as fr
from . import oracle_lib as orc
from . import refsem
from .test_gpu_query import _CODE, _cli, _oracle

pytestmark = pytest.mark.gpu

CFRK_ERR_ARG, CFRK_ERR_STATE, CFRK_ERR_LAYOUT, CFRK_ERR_SMALL_BUF = -1, -4, -5, -9
COUNT_MAX = 0xFFFFFFFE
KS = [5, 12, 13, 21, 31, 32, 33, 47, 64]
GUARD = 64
TIE_RUN = 40


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


class _Guarded:
    """a device array of n bytes, `skew` bytes off a 64-byte boundary, with guard bytes of 0xA5 on both sides"""

    def __init__(self, ctx, n, skew=0):
        self.ctx, self.n, self.lo = ctx, n, GUARD + skew
        self.total = self.lo + n + GUARD
        self.base = ctx.alloc(self.total)
        ctx.h2d(self.base, np.full(self.total, 0xA5, np.uint8))
        self.ptr = self.base + self.lo

    def fetch(self, used, dtype=np.uint8):
        """the first `used` bytes as dtype; everything else must still be 0xA5"""
        whole = np.empty(self.total, np.uint8)
        self.ctx.d2h(whole, self.base)
        assert (whole[:self.lo] == 0xA5).all(), "bytes in front of the array were written"
        assert (whole[self.lo + used:] == 0xA5).all(), "bytes behind the used part were written"
        return whole[self.lo:self.lo + used].copy().view(dtype)

    def free(self):
        self.ctx.free(self.base)


def _upload(ctx, arr, skew=0):
    arr = np.ascontiguousarray(arr)
    p = ctx.alloc(arr.nbytes + 64 + skew)
    if arr.nbytes:
        ctx.h2d(p + skew, arr)
    return p


# ------------------------------------------------------------------ spans: the mix

def _counted_reads(k):
    """the counted set: a small genome as one read (every genome window occurs), reads at a few x coverage, and some
    of them twice more, so that counts 1, 2 and more all occur"""
    rng = np.random.default_rng(9100 + k)
    genome = rng.integers(0, 4, 6000).astype(np.int8)
    reads = [genome.copy()]
    for _ in range(120):
        a = int(rng.integers(0, len(genome) - 150))
        reads.append(genome[a:a + 150].copy())
    reads += [r.copy() for r in reads[1:31]] + [r.copy() for r in reads[1:11]]
    return genome, refsem.flatten(reads)


def _sub(r, p):
    r[p] = (r[p] + 1) % 4


def _query_reads(k, genome):
    """-> (data, start, length, marks): reads that differ from the counted ones; marks name the reads built for one thing"""
    import cfrk_amd
    rng = np.random.default_rng(9200 + k)
    F = cfrk_amd.CFRK_SPANS_FAST_WINDOWS
    reads, marks = [], {}
    for nwin in (0, 1, 15, 16, 17, 255, 256, 257, 1000, F, F + 1):
        L = nwin + k - 1
        a = int(rng.integers(0, len(genome) - L))
        r = genome[a:a + L].copy()
        for p in rng.integers(0, max(L, 1), 3 if L > 40 else 0):
            _sub(r, int(p))
        reads.append(r)
    marks["above_fast"] = len(reads) - 1
    long_read = np.concatenate([genome, rng.integers(0, 4, 8000).astype(np.int8), genome])
    long_read[3000] = long_read[7000] = -1                       # invalid codes inside a long read
    assert len(long_read) >= 20000
    marks["long"] = len(reads)
    reads.append(long_read)
    reads.append(np.full(300, 1, np.int8))                       # a homopolymer
    # the first window of a solid run at residue r, its last window at residue (r + 70) % 64: every residue at either end
    marks["seam0"] = len(reads)
    for r_ in range(64):
        L = r_ + 70 + 2 * k                                      # windows 0 .. r_ + 70 + k
        a = int(rng.integers(0, len(genome) - L))
        r = genome[a:a + L].copy()
        if r_ > 0:
            _sub(r, r_ - 1)                                      # kills the windows r_ - k .. r_ - 1
        _sub(r, r_ + 70 + k)                                     # kills the windows from r_ + 71 on
        reads.append(r)
    # two runs of TIE_RUN windows with k dead windows between them
    a = int(rng.integers(0, len(genome) - 400))
    r = genome[a:a + 2 * TIE_RUN + 2 * k - 1].copy()
    _sub(r, TIE_RUN + k - 1)
    marks["tie"] = len(reads)
    reads.append(r)
    marks["whole"] = len(reads)
    reads.append(genome[1000:1000 + 180 + k].copy())             # a run that is the whole read
    r = genome[2000:2000 + 100 + k].copy()
    _sub(r, k)                                                   # window 0 solid, window 1 not
    marks["w0_then_gap"] = len(reads)
    reads.append(r)
    r = genome[2500:2500 + 100 + k].copy()
    _sub(r, 0)                                                   # window 0 not solid
    marks["w0_dead"] = len(reads)
    reads.append(r)
    return refsem.flatten(reads) + (marks,)


def _assert_spans(got, exp, what=""):
    assert got.dtype == exp.dtype and len(got) == len(exp)
    for f in ("offset", "length"):
        bad = np.nonzero(got[f] != exp[f])[0]
        assert len(bad) == 0, (what, f, bad[:10], got[bad[:10]], exp[bad[:10]])


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("canonical", [False, True])
def test_read_spans_vs_oracle(ctx, k, canonical):
    """both modes and the four threshold settings against one job and one set of oracle counts"""
    import cfrk_amd
    genome, (cdata, cstart, clength) = _counted_reads(k)
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL if canonical else 0, 0)
    g.add(cdata, cstart, clength)
    want = _oracle(cdata, k, canonical)
    qd, qs, ql, marks = _query_reads(k, genome)
    counts, valid = fr.window_counts(qd, k, canonical, want)
    largest = int(want[2].max())
    assert largest >= 3 and (k < 12 or ((want[2] == 1).any() and (want[2] == 2).any()))
    exact = k >= 21      # (a substituted window is absent from the counted set: 4^k is far above its 10^4 windows)
    F = cfrk_amd.CFRK_SPANS_FAST_WINDOWS
    nwin = np.maximum(ql.astype(np.int64) - k + 1, 0)
    for mode in (cfrk_amd.CFRK_SPAN_LONGEST, cfrk_amd.CFRK_SPAN_PREFIX):
        for mn, mx in ((1, COUNT_MAX), (2, COUNT_MAX), (0, COUNT_MAX), (1, largest - 1)):
            exp = fr.ref_spans(qd, qs, ql, k, mn, mx, mode, counts, valid)
            if (mn, mx) == (1, COUNT_MAX):
                # the expected spans hold what the mix was built for
                assert (exp["length"] == 0).any() and ((exp["length"] == ql) & (ql > 0)).any()
                assert tuple(exp[marks["whole"]]) == (0, int(ql[marks["whole"]]))
                assert (exp["length"][nwin > F] > 0).any()
                if exact:
                    assert tuple(exp[marks["w0_then_gap"]]) == ((0, k) if mode == cfrk_amd.CFRK_SPAN_PREFIX else (k + 1, 99))
                    assert tuple(exp[marks["tie"]]) == (0, TIE_RUN + k - 1)
                    if mode == cfrk_amd.CFRK_SPAN_LONGEST:
                        seam = exp[marks["seam0"]:marks["seam0"] + 64]
                        assert seam["offset"].tolist() == list(range(64)) and (seam["length"] == 71 + k - 1).all()
                        assert ((exp["offset"] > 0) & (exp["offset"] + exp["length"] < ql)).any()      # interior spans
                        assert exp[marks["long"]]["offset"] > 0 and exp[marks["long"]]["length"] > F
                    else:
                        assert tuple(exp[marks["w0_dead"]]) == (0, 0)
            if mn == 0:
                assert (exp["length"][nwin > 0] > 0).sum() > len(ql) - 5       # every valid window is solid
            got = g.read_spans(qd, qs, ql, mn, mx, mode)
            _assert_spans(got, exp, (k, canonical, mode, mn, mx))
    none = g.read_spans(qd, qs, ql, 3, 2)                            # min_count > max_count: none solid, not an error
    assert (none["offset"] == 0).all() and (none["length"] == 0).all()
    assert g.digest() == orc.digest(*want, two_word=k > 32)


def _device_spans(ctx, g, data, start, length, mn, mx, mode, skew=0):
    nN, nS = len(data), len(start)
    d_data, d_start, d_length = _upload(ctx, data, skew), _upload(ctx, start), _upload(ctx, length)
    out = _Guarded(ctx, nS * 8)
    try:
        g.read_spans_device(d_data + skew, d_start, d_length, nN, nS, mn, mx, mode, out.ptr)
        ctx.sync()
        return out.fetch(nS * 8, fr.SPAN_DTYPE)
    finally:
        ctx.sync()
        for p in (d_data, d_start, d_length):
            ctx.free(p)
        out.free()


@pytest.mark.parametrize("k", [12, 31, 63])
def test_device_form_equals_host_form_and_guards_out_of_range_reads(ctx, k):
    import cfrk_amd
    genome, (cdata, cstart, clength) = _counted_reads(k)
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, 0)
    g.add(cdata, cstart, clength)
    want = _oracle(cdata, k, True)
    qd, qs, ql, _ = _query_reads(k, genome)
    counts, valid = fr.window_counts(qd, k, True, want)
    for mode in (cfrk_amd.CFRK_SPAN_LONGEST, cfrk_amd.CFRK_SPAN_PREFIX):
        exp = fr.ref_spans(qd, qs, ql, k, 2, COUNT_MAX, mode, counts, valid)
        for skew in (0, 1, 7):                                       # no alignment requirement on d_data
            _assert_spans(_device_spans(ctx, g, qd, qs, ql, 2, COUNT_MAX, mode, skew), exp, (k, mode, skew))
    # one read range past nN, one negative start (and a few more): {0, 0}, the neighbours their own, the guards intact
    exp = fr.ref_spans(qd, qs, ql, k, 1, COUNT_MAX, cfrk_amd.CFRK_SPAN_LONGEST, counts, valid)
    st, ln = qs.copy(), ql.copy()
    nN = len(qd)
    bad = {2: (nN - 10, 100), 5: (-5, 100), 6: (nN + 7, 50), 20: (0, -3), 21: (int(qs[21]), 0x7FFFFFFF),
           30: (-(1 << 62), 150), 31: ((1 << 62), 150), len(st) - 1: (nN - 20, k + 25)}
    for i, (s, L) in bad.items():
        st[i], ln[i] = s, L
        exp[i] = (0, 0)
    assert (exp["length"] > 0).sum() > 60
    _assert_spans(_device_spans(ctx, g, qd, st, ln, 1, COUNT_MAX, cfrk_amd.CFRK_SPAN_LONGEST), exp)


def test_read_spans_errors(ctx):
    import cfrk_amd
    L = cfrk_amd.load_library()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    data, start, length = refsem.flatten([np.zeros(40, np.int8), np.ones(40, np.int8)])
    out = np.zeros(2, cfrk_amd.READ_SPAN_DTYPE)
    args = lambda h, mode=1: (h, vp(data), vp(start), vp(length), len(data), 2, 1, COUNT_MAX, mode, vp(out))
    fresh = cfrk_amd.Context(0)
    try:
        assert L.cfrk_global_read_spans(*args(fresh._h)) == CFRK_ERR_STATE          # before begin
        assert L.cfrk_global_read_spans_device(fresh._h, None, None, None, 82, 2, 1, 2, 1, None) == CFRK_ERR_STATE
    finally:
        fresh.close()
    reads, _, _ = orc.synth_reads(0, 2000, 150, 20000)
    g = cfrk_amd.GlobalCounter(ctx, 31, cfrk_amd.CFRK_CANONICAL | cfrk_amd.CFRK_RUNS_ONLY, 100000)
    g.add(reads)
    with pytest.raises(cfrk_amd.CfrkError) as e:
        g.read_spans(data, start, length)
    assert e.value.code == CFRK_ERR_STATE
    g = cfrk_amd.GlobalCounter(ctx, 31, cfrk_amd.CFRK_CANONICAL, 100000)
    g.add(reads)
    h = ctx._h
    assert L.cfrk_global_read_spans(*args(h)) == 0
    for mode in (2, -1):
        assert L.cfrk_global_read_spans(*args(h, mode)) == CFRK_ERR_ARG
        assert L.cfrk_global_read_spans_device(*args(h, mode)) == CFRK_ERR_ARG
    for drop in range(4):                                           # each pointer NULL in turn
        a = [vp(data), vp(start), vp(length), vp(out)]
        a[drop] = None
        assert L.cfrk_global_read_spans(h, a[0], a[1], a[2], len(data), 2, 1, 2, 1, a[3]) == CFRK_ERR_ARG
        assert L.cfrk_global_read_spans_device(h, a[0], a[1], a[2], len(data), 2, 1, 2, 1, a[3]) == CFRK_ERR_ARG
    assert L.cfrk_global_read_spans(h, vp(data), vp(start), vp(length), -1, 2, 1, 2, 1, vp(out)) == CFRK_ERR_ARG
    assert L.cfrk_global_read_spans(h, vp(data), vp(start), vp(length), len(data), -1, 1, 2, 1, vp(out)) == CFRK_ERR_ARG
    assert L.cfrk_global_read_spans(h, None, None, None, 0, 0, 1, 2, 1, None) == 0              # nS = 0 is fine
    assert L.cfrk_global_read_spans_device(h, None, None, None, 0, 0, 1, 2, 0, None) == 0
    bad = start.copy(); bad[1] += 1                                 # layout checked like cfrk_global_add's
    with pytest.raises(cfrk_amd.CfrkError) as e:
        g.read_spans(data, bad, length)
    assert e.value.code == CFRK_ERR_LAYOUT
    assert g.read_spans(data, start, length, 0)["length"].tolist() == [40, 40]       # the job is still usable


# ------------------------------------------------------------------ select

def _device_select(ctx, data, start, length, spans=None, keep=None, min_len=0, index=True, cap_data=None, cap_reads=None,
                   skew_in=0, skew_out=0, sizes_only=False):
    """the device form on guarded arrays of its own -> (nN, nS, data, start, length, index or None).  A CfrkError is
    passed on after the check that nothing was written."""
    import cfrk_amd
    nN, nS = len(data), len(start)
    cap_data = nN if cap_data is None else cap_data
    cap_reads = nS if cap_reads is None else cap_reads
    ins = [_upload(ctx, data, skew_in), _upload(ctx, start), _upload(ctx, length)]
    d_span = _upload(ctx, spans) if spans is not None else 0
    d_keep = _upload(ctx, np.ascontiguousarray(keep, np.uint8)) if keep is not None else 0
    o_data, o_start = _Guarded(ctx, cap_data, skew_out), _Guarded(ctx, cap_reads * 8)
    o_length, o_index = _Guarded(ctx, cap_reads * 4), _Guarded(ctx, cap_reads * 8)
    outs = (o_data, o_start, o_length, o_index)
    try:
        try:
            if sizes_only:
                n, s = ctx.select_reads_device(ins[0] + skew_in, ins[1], ins[2], nN, nS, d_span, d_keep, min_len, 0, 0, 0, 0, 0, 0)
            else:
                n, s = ctx.select_reads_device(ins[0] + skew_in, ins[1], ins[2], nN, nS, d_span, d_keep, min_len, o_data.ptr,
                                               cap_data, o_start.ptr, o_length.ptr, o_index.ptr if index else 0, cap_reads)
        except cfrk_amd.CfrkError:
            ctx.sync()
            for o in outs:
                o.fetch(0)                                       # nothing written
            raise
        ctx.sync()
        if sizes_only:
            for o in outs:
                o.fetch(0)
            return n, s
        return (n, s, o_data.fetch(n, np.int8), o_start.fetch(s * 8, np.int64), o_length.fetch(s * 4, np.int32),
                o_index.fetch(s * 8 if index else 0, np.int64))
    finally:
        ctx.sync()
        for p in ins + [d_span, d_keep]:
            if p:
                ctx.free(p)
        for o in outs:
            o.free()


def _assert_select(got, exp, what=""):
    n, s, d, st, ln, ix = got
    ed, est, eln, eix = exp
    assert (n, s) == (len(ed), len(est)), (what, n, s, len(ed), len(est))
    assert (st == est).all() and (ln == eln).all(), what
    if len(ix) or not len(eix):
        assert (ix == eix).all(), what
    bad = np.nonzero(d != ed)[0]
    assert len(bad) == 0, (what, bad[:10], d[bad[:10]], ed[bad[:10]])


def _select_mix(seed=0):
    """every length class around the copy's tile, span offsets of every residue mod 4, spans that end at the read's end"""
    import cfrk_amd
    T = cfrk_amd.CFRK_SELECT_TILE_BYTES
    rng = np.random.default_rng(300 + seed)
    lens = [0, 1, 3, 4, 5, 150, T - 1, T, T + 1, 5 * T] + [int(x) for x in rng.integers(0, 300, 60)]
    order = rng.permutation(len(lens))
    reads = [rng.integers(-1, 4, lens[i]).astype(np.int8) for i in order]
    data, start, length = refsem.flatten(reads)
    spans = np.zeros(len(reads), fr.SPAN_DTYPE)
    for i, L in enumerate(length):
        off = min(i % 4, int(L))
        spans[i] = (off, int(L) - off if i % 3 else (int(L) - off) // 2)
    assert set(spans["offset"][length >= 3] % 4) == {0, 1, 2, 3}
    assert ((spans["offset"] + spans["length"] == length) & (length > 4)).any()
    keep = rng.random(len(reads)) < 0.7
    return data, start, length, spans, keep


@pytest.mark.parametrize("min_len", [0, 1, 21])
def test_select_vs_numpy(ctx, min_len):
    import cfrk_amd
    data, start, length, spans, keep = _select_mix(min_len)
    for sp, kp, skews in ((spans, keep, (0, 0)), (spans, None, (1, 3)), (None, keep, (2, 5)), (None, None, (3, 0)), (spans, keep, (0, 9))):
        exp = fr.ref_select(data, start, length, sp, kp, min_len)
        assert 0 < len(exp[1]) < len(start) or (kp is None and min_len == 0)
        what = (min_len, sp is not None, kp is not None, skews)
        _assert_select(_device_select(ctx, data, start, length, sp, kp, min_len, skew_in=skews[0], skew_out=skews[1]), exp, what)
        d, s, l, i = ctx.select_reads(data, start, length, sp, kp, min_len)                     # the host form
        _assert_select((len(d), len(s), d, s, l, i), exp, ("host",) + what)
    exp = fr.ref_select(data, start, length, spans, keep, min_len)
    got = _device_select(ctx, data, start, length, spans, keep, min_len, index=False)           # d_index_out NULL
    assert len(got[5]) == 0
    _assert_select(got, exp, "no index")
    with pytest.raises(cfrk_amd.CfrkError) as e:                    # the sizes-only call: sizes complete, nothing written
        _device_select(ctx, data, start, length, spans, keep, min_len, sizes_only=True)
    assert e.value.code == CFRK_ERR_SMALL_BUF and (e.value.nN, e.value.nS) == (len(exp[0]), len(exp[1]))


def test_select_nothing_kept_and_no_reads(ctx):
    import cfrk_amd
    data, start, length, spans, keep = _select_mix()
    none = np.zeros(len(start), bool)
    got = _device_select(ctx, data, start, length, spans, none, 0)
    assert got[:2] == (0, 0) and all(len(a) == 0 for a in got[2:])
    got = _device_select(ctx, data, start, length, None, None, 0x7FFFFFFF)       # min_len above every read
    assert got[:2] == (0, 0)
    assert all(len(a) == 0 for a in ctx.select_reads(data, start, length, spans, none))
    e = np.zeros(0, np.int8)
    assert _device_select(ctx, e, e.astype(np.int64), e.astype(np.int32))[:2] == (0, 0)          # nS = 0
    assert all(len(a) == 0 for a in ctx.select_reads(e, e.astype(np.int64), e.astype(np.int32)))
    with pytest.raises(cfrk_amd.CfrkError) as err:
        ctx.select_reads(data, start, length, min_len=-1)
    assert err.value.code == CFRK_ERR_ARG


def test_select_small_buffers_report_the_sizes_and_write_nothing(ctx):
    import cfrk_amd
    data, start, length, spans, keep = _select_mix(7)
    exp = fr.ref_select(data, start, length, spans, keep, 1)
    nN, nS = len(exp[0]), len(exp[1])
    for caps in ((nN - 1, nS), (nN, nS - 1)):                      # by one byte, by one read
        with pytest.raises(cfrk_amd.CfrkError) as e:
            _device_select(ctx, data, start, length, spans, keep, 1, cap_data=caps[0], cap_reads=caps[1])
        assert e.value.code == CFRK_ERR_SMALL_BUF and (e.value.nN, e.value.nS) == (nN, nS)
    _assert_select(_device_select(ctx, data, start, length, spans, keep, 1, cap_data=nN, cap_reads=nS), exp)   # exactly enough


def test_select_output_tile_seams(ctx):
    """a kept read that ends exactly on an output-tile boundary and the next one beginning on it; tiles that hold
    nothing but terminators (empty reads kept with min_len = 0)"""
    import cfrk_amd
    T = cfrk_amd.CFRK_SELECT_TILE_BYTES
    rng = np.random.default_rng(11)
    lens = [T - 1, 150, T - 152, 7, 2 * T - 9, 300] + [0] * (2 * T + 77) + [150] * 109 + [33]
    reads = [rng.integers(0, 4, L).astype(np.int8) for L in lens]
    data, start, length = refsem.flatten(reads)
    assert start[1] == T and start[3] == 2 * T and start[5] == 4 * T            # reads that begin on a tile boundary
    exp = fr.ref_select(data, start, length)
    assert (exp[0] == data).all()
    for skew in (0, 3):
        _assert_select(_device_select(ctx, data, start, length, skew_in=skew, skew_out=(skew * 5) % 16), exp, skew)
    # trimmed so that the seam falls behind a kept span: spans of T - 1 bases out of longer reads
    reads = [rng.integers(0, 4, T + 40).astype(np.int8) for _ in range(5)]
    data, start, length = refsem.flatten(reads)
    spans = np.array([(i + 1, T - 1) for i in range(5)], fr.SPAN_DTYPE)
    exp = fr.ref_select(data, start, length, spans)
    assert exp[1].tolist() == [i * T for i in range(5)]
    _assert_select(_device_select(ctx, data, start, length, spans), exp)


def test_select_more_read_tiles_than_a_scan_block(ctx):
    """more than CFRK_SELECT_SCAN_TILES tiles of reads AND of output bytes: the one-workgroup scan walks a second block"""
    import cfrk_amd
    T, R, S = cfrk_amd.CFRK_SELECT_TILE_BYTES, cfrk_amd.CFRK_SELECT_TILE_READS, cfrk_amd.CFRK_SELECT_SCAN_TILES
    rng = np.random.default_rng(12)
    nS = S * R + 300
    length = rng.integers(60, 101, nS).astype(np.int32)
    start = np.concatenate([[0], np.cumsum(length.astype(np.int64) + 1)[:-1]]).astype(np.int64)
    nN = int(start[-1]) + int(length[-1]) + 1
    data = rng.integers(0, 4, nN).astype(np.int8)
    data[start + length] = -1
    keep = rng.random(nS) < 0.9
    ed = data[np.repeat(keep, length.astype(np.int64) + 1)]
    eln = length[keep]
    est = np.concatenate([[0], np.cumsum(eln.astype(np.int64) + 1)[:-1]]).astype(np.int64)
    assert len(ed) > S * T and nS > S * R
    _assert_select(_device_select(ctx, data, start, length, None, keep), (ed, est, eln, np.nonzero(keep)[0]))


def test_select_drops_bad_spans_on_the_device_and_refuses_them_on_the_host(ctx):
    import cfrk_amd
    data, start, length, spans, keep = _select_mix(3)
    nN = len(data)
    big = int(np.argmax(length))
    bad_spans = spans.copy()
    i_neg, i_long, i_neglen = [int(i) for i in np.nonzero(length > 20)[0][:3]]
    bad_spans[i_neg] = (-1, 5)                                      # a negative offset
    bad_spans[i_long] = (2, int(length[i_long]))                    # longer than its read
    bad_spans[i_neglen] = (0, -4)
    exp = fr.ref_select(data, start, length, bad_spans, None, 0)
    assert not set(exp[3].tolist()) & {i_neg, i_long, i_neglen}
    _assert_select(_device_select(ctx, data, start, length, bad_spans), exp, "bad spans")
    for i in (i_neg, i_long, i_neglen):                             # the host form names the read
        one = spans.copy()
        one[i] = bad_spans[i]
        with pytest.raises(cfrk_amd.CfrkError, match=r"read %d: span" % i) as e:
            ctx.select_reads(data, start, length, one)
        assert e.value.code == CFRK_ERR_LAYOUT
    # read ranges outside [0, nN): dropped, nothing outside the buffers is touched (the guards are checked)
    st, ln = start.copy(), length.copy()
    out_of_range = {0: (-3, 10), 4: (nN - 5, 50), 9: (nN + 100, 4), 12: (0, -1), 13: (1 << 62, 10), big: (int(start[big]), 0x7FFFFFFF)}
    sp = spans.copy()
    for i, (s, L) in out_of_range.items():
        st[i], ln[i] = s, L
        sp[i] = (0, 0)                                             # (a span that would lie inside: the range alone drops it)
    good = np.ones(len(st), bool)
    good[list(out_of_range)] = False
    exp = fr.ref_select(data, np.where(good, st, 0), np.where(good, ln, 0), sp, good, 0)
    _assert_select(_device_select(ctx, data, st, ln, sp), exp, "ranges")
    with pytest.raises(cfrk_amd.CfrkError) as e:                    # the host form checks the layout
        ctx.select_reads(data, st, ln, sp)
    assert e.value.code == CFRK_ERR_LAYOUT


# ------------------------------------------------------------------ end to end

def _noisy_reads(rng, genome, n, lo, hi, p_err):
    reads = []
    for _ in range(n):
        L = int(rng.integers(lo, hi))
        a = int(rng.integers(0, len(genome) - L))
        r = genome[a:a + L].copy()
        for p in np.nonzero(rng.random(L) < p_err)[0]:
            _sub(r, int(p))
        reads.append(r)
    return reads


def test_text_to_second_count_on_the_device(ctx):
    """parse_fasta_device -> count at k = 21 -> read_spans_device -> select_reads_device -> a second job's add_device on
    the selected buffers at k = 15: its digest is the oracle's count of the numpy-trimmed reads"""
    import cfrk_amd
    k1, k2 = 21, 15
    rng = np.random.default_rng(77)
    genome = rng.integers(0, 4, 20000).astype(np.int8)
    reads = _noisy_reads(rng, genome, 1500, 80, 200, 0.01)
    reads += [rng.integers(0, 4, int(L)).astype(np.int8) for L in rng.integers(30, 200, 60)]      # not from the genome
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    text = "".join(">r%d\n%s\n" % (i, "".join("ACGT"[c] for c in r)) for i, r in enumerate(reads)).encode()
    data, start, length = refsem.flatten(reads)
    want = _oracle(data, k1, True)
    counts, valid = fr.window_counts(data, k1, True, want)
    spans = fr.ref_spans(data, start, length, k1, 2, COUNT_MAX, fr.SPAN_LONGEST, counts, valid)
    ed, est, eln, eix = fr.ref_select(data, start, length, spans, None, k1)
    assert 0 < len(est) < len(start) and (eln < length[eix]).any()      # some reads dropped, some trimmed
    nb = len(text)
    d_text = _upload(ctx, np.frombuffer(text, np.uint8))
    d_data, d_start, d_length = ctx.alloc(nb + 16), ctx.alloc(nb * 4 + 8), ctx.alloc(nb * 2 + 4)
    d_span = ctx.alloc(len(start) * 8)
    o_data, o_start, o_length = ctx.alloc(nb + 16), ctx.alloc(len(start) * 8), ctx.alloc(len(start) * 4)
    try:
        nN, nS = ctx.parse_fasta_device(d_text, nb, 0, d_data, nb, d_start, d_length, (nb + 1) // 2)
        assert (nN, nS) == (len(data), len(start))
        g = cfrk_amd.GlobalCounter(ctx, k1, cfrk_amd.CFRK_CANONICAL, 0)
        g.add_device(d_data, nN)
        g.read_spans_device(d_data, d_start, d_length, nN, nS, 2, COUNT_MAX, cfrk_amd.CFRK_SPAN_LONGEST, d_span)
        n2, s2 = ctx.select_reads_device(d_data, d_start, d_length, nN, nS, d_span, 0, k1, o_data, nN, o_start, o_length, 0, nS)
        assert (n2, s2) == (len(ed), len(est))
        assert g.digest() == orc.digest(*want, two_word=False)
        g2 = cfrk_amd.GlobalCounter(ctx, k2, cfrk_amd.CFRK_CANONICAL, 0)
        g2.add_device(o_data, n2)
        assert g2.digest() == orc.digest(*_oracle(ed, k2, True), two_word=False)
    finally:
        ctx.sync()
        for p in (d_text, d_data, d_start, d_length, d_span, o_data, o_start, o_length):
            ctx.free(p)


def test_cli_filter_out(tmp_path):
    from .test_gpu_read_stats import _ref_stats
    cli = _cli()
    k = 21
    rng = np.random.default_rng(8811)
    genome = rng.integers(0, 4, 8000).astype(np.int8)
    creads = _noisy_reads(rng, genome, 1200, 60, 220, 0.0)
    fa = tmp_path / "g.fasta"
    fa.write_text("".join(">r%d\n%s\n" % (i, "".join("ACGT"[c] for c in r)) for i, r in enumerate(creads)))
    qs = ["".join("ACGT"[c] for c in r) for r in _noisy_reads(rng, genome, 300, 30, 260, 0.01)]
    qs += ["", "ACGT", qs[0][:k - 1], qs[1][:40] + "N" + qs[1][40:], qs[2].lower(), "T" * (k + 30),
           "".join("ACGT"[c] for c in genome[:3000])]
    qf = tmp_path / "q.fasta"
    qf.write_text("".join(">q%d\n%s\n" % (i, s) for i, s in enumerate(qs)))
    cdata, _, _ = refsem.flatten(creads)
    want = _oracle(cdata, k, True)
    qd, qst, qln = refsem.flatten([np.array([_CODE.get(ch, -1) for ch in s.upper()], np.int8) for s in qs])
    counts, valid = fr.window_counts(qd, k, True, want)
    med = _ref_stats(qd, qst, qln, k, True, want, 0)["median"]

    def text(mode, mn=2, mx=COUNT_MAX, min_len=k, max_median=None):
        spans = None if mode is None else fr.ref_spans(qd, qst, qln, k, mn, mx, mode, counts, valid)
        keep = None if max_median is None else med <= max_median
        return fr.fasta_text(*fr.ref_select(qd, qst, qln, spans, keep, min_len))

    base = [cli, str(fa)]
    glob = ["--global", "--canonical"]
    plain, full = tmp_path / "plain.cfrk", tmp_path / "full.bin"
    subprocess.run(base + [str(plain), str(k)] + glob, check=True, timeout=300)
    subprocess.run(base + [str(full), str(k)] + glob + ["--binary"], check=True, timeout=300)
    longest = text(fr.SPAN_LONGEST)
    assert 0 < longest.count(b">") < len(qs)
    f1, o1 = tmp_path / "f1.fa", tmp_path / "o1.cfrk"
    subprocess.run(base + [str(o1), str(k)] + glob + ["--query", str(qf), "--filter-out", str(f1)], check=True, timeout=300)
    assert f1.read_bytes() == longest
    assert o1.read_bytes() == plain.read_bytes()                      # the count output is that of a run without the option
    f2, none = tmp_path / "f2.fa", tmp_path / "none.cfrk"
    subprocess.run(base + [str(none), str(k)] + glob + ["--query", str(qf), "--filter-out", str(f2), "--filter-trim", "prefix",
                                                        "--filter-min-count", "1", "--query-only"], check=True, timeout=300)
    assert f2.read_bytes() == text(fr.SPAN_PREFIX, mn=1) and not none.exists()
    db = [cli, "--query-db", str(full), "--query", str(qf)]
    f3 = tmp_path / "f3.fa"
    subprocess.run(db + ["--filter-out", str(f3)], check=True, timeout=300)
    assert f3.read_bytes() == longest
    mm = int(np.median(med[med > 0]))
    f4 = tmp_path / "f4.fa"
    subprocess.run(db + ["--filter-out", str(f4), "--filter-max-median", str(mm), "--filter-trim", "prefix"], check=True, timeout=300)
    want4 = text(fr.SPAN_PREFIX, max_median=mm)
    assert f4.read_bytes() == want4 and want4 != text(fr.SPAN_PREFIX)
    f5 = tmp_path / "f5.fa"
    subprocess.run(db + ["--filter-out", str(f5), "--filter-trim", "none", "--filter-min-len", "0", "--filter-max-median", str(mm),
                         "--filter-max-count", "3"], check=True, timeout=300)
    assert f5.read_bytes() == text(None, min_len=0, max_median=mm)
