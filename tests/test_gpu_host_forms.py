"""GPU: every host form of the C ABI against its _device form on buffers from Context.alloc -- the same result exactly,
the same refusal of a bad start/length table (code and text) from every form that checks one, the same result again
right after that refusal on the same context, and for the measure-then-emit forms the same CFRK_ERR_SMALL_BUF sizes at a
capacity one below the need.  The smallest input that reaches every part: four reads of 0, 5, 40 and 300 bases, a job at
k = 5 and one at k = 33 (two-word keys), a FASTA and a FASTQ text of four records.  What the features compute is checked
against references elsewhere (test_gpu_query / _read_stats / _filter / _sparse / _sketch / _ingest / _fastq); this file
holds the two forms of a pair to each other.  cfrk_per_read_dense takes a table but has never checked it, and
cfrk_global_query and the parsers take none: they appear in the equality test only."""
import ctypes as C

import numpy as np
import pytest

from . import refsem

pytestmark = pytest.mark.gpu

CFRK_ERR_LAYOUT, CFRK_ERR_SMALL_BUF = -5, -9
LENGTHS = (0, 5, 40, 300)
KS = (5, 33)
FASTA = b">r0\nACGTA\n>r1 two lines\nACGTACGTAC\nGGTTAACC\n>r2\nTTTT\n>r3\nACGTNACGTTGCA\n"
FASTQ = b"@r0\nACGTA\n+\nIIIII\n@r1\nACGTACGTACGGTTAACC\n+r1\nIIIIIIIII#IIIIIIII\n@r2\nTTTT\n+\n!!II\n@r3\nACGTNACGTTGCA\n+\nIIIIIIIIIIIII\n"


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def reads():
    rng = np.random.default_rng(1600)
    rs = [rng.integers(0, 4, n).astype(np.int8) for n in LENGTHS]
    rs[3][100] = -1                     # an invalid base inside a read
    rs[3][200:240] = rs[2]              # the short read occurs in the long one: counts above 1
    return refsem.flatten(rs)


class _Dev:
    """device buffers of one test, freed at its end"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def room(self, nbytes):
        self.ptrs.append(self.ctx.alloc(nbytes + 64))
        return self.ptrs[-1]

    def up(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.room(arr.nbytes)
        if arr.nbytes:
            self.ctx.h2d(p, arr)
        return p

    def down(self, p, n, dtype):
        out = np.empty(n, dtype)
        if n:
            self.ctx.d2h(out, p)
        else:
            self.ctx.sync()
        return out

    def free(self):
        for p in self.ptrs:
            self.ctx.free(p)


@pytest.fixture
def dev(ctx):
    d = _Dev(ctx)
    yield d
    d.free()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _spans_keep(length):
    import cfrk_amd
    spans = np.zeros(len(length), cfrk_amd.READ_SPAN_DTYPE)
    spans["offset"], spans["length"] = (0, 1, 0, 10), (0, 3, 40, 200)
    return spans, np.array([1, 1, 0, 1], np.uint8)


# ---- the pairs: host(g, ctx, k, data, start, length) and device(g, ctx, k, dev, data, start, length) -> tuple of arrays.
# g: the job the form works on (None where it needs none).

def _export(g):
    return g.export()


def h_add(g, ctx, k, data, start, length):
    g.add(data, start, length)
    return _export(g)


def d_add(g, ctx, k, dev, data, start, length):
    g.add_device(dev.up(data), len(data))
    return _export(g)


def h_query_reads(g, ctx, k, data, start, length):
    return (g.query_reads(data, start, length),)


def d_query_reads(g, ctx, k, dev, data, start, length):
    out = dev.room(len(data) * 4)
    g.query_reads_device(dev.up(data), len(data), out)
    return (dev.down(out, len(data), np.uint32),)


def h_read_stats(g, ctx, k, data, start, length):
    return (g.read_stats(data, start, length, 2),)


def d_read_stats(g, ctx, k, dev, data, start, length):
    import cfrk_amd
    out = dev.room(len(length) * 32)
    g.read_stats_device(dev.up(data), dev.up(start), dev.up(length), len(data), len(length), 2, out)
    return (dev.down(out, len(length), cfrk_amd.READ_STATS_DTYPE),)


def h_read_spans(g, ctx, k, data, start, length):
    return (g.read_spans(data, start, length, 1, 1),)


def d_read_spans(g, ctx, k, dev, data, start, length):
    import cfrk_amd
    out = dev.room(len(length) * 8)
    g.read_spans_device(dev.up(data), dev.up(start), dev.up(length), len(data), len(length), 1, 1, cfrk_amd.CFRK_SPAN_LONGEST, out)
    return (dev.down(out, len(length), cfrk_amd.READ_SPAN_DTYPE),)


def _select_host_raw(ctx, data, start, length, cap_data, cap_reads):
    """-> (rc, nN', nS', arrays of exactly the capacities)"""
    spans, keep = _spans_keep(length)
    o = (np.empty(cap_data, np.int8), np.empty(cap_reads, np.int64), np.empty(cap_reads, np.int32), np.empty(cap_reads, np.int64))
    nN, nS = C.c_int64(-1), C.c_int64(-1)
    rc = ctx._L.cfrk_reads_select(ctx._h, _ptr(data), _ptr(start), _ptr(length), len(data), len(length), _ptr(spans), _ptr(keep), 1,
                                  _ptr(o[0]), cap_data, _ptr(o[1]), _ptr(o[2]), _ptr(o[3]), cap_reads, C.byref(nN), C.byref(nS))
    return rc, nN.value, nS.value, o


def _select_dev_raw(ctx, dev, data, start, length, cap_data, cap_reads):
    import cfrk_amd
    spans, keep = _spans_keep(length)
    o = (dev.room(cap_data), dev.room(cap_reads * 8), dev.room(cap_reads * 4), dev.room(cap_reads * 8))
    try:
        nN, nS = ctx.select_reads_device(dev.up(data), dev.up(start), dev.up(length), len(data), len(length), dev.up(spans), dev.up(keep), 1,
                                         o[0], cap_data, o[1], o[2], o[3], cap_reads)
    except cfrk_amd.CfrkError as e:
        return e.code, e.nN, e.nS, None
    return 0, nN, nS, (dev.down(o[0], nN, np.int8), dev.down(o[1], nS, np.int64), dev.down(o[2], nS, np.int32), dev.down(o[3], nS, np.int64))


def h_select(g, ctx, k, data, start, length):
    spans, keep = _spans_keep(length)
    return ctx.select_reads(data, start, length, spans, keep, 1)


def d_select(g, ctx, k, dev, data, start, length):
    rc, nN, nS, _ = _select_dev_raw(ctx, dev, data, start, length, 0, 0)
    assert rc == CFRK_ERR_SMALL_BUF
    rc, _, _, out = _select_dev_raw(ctx, dev, data, start, length, nN, nS)
    assert rc == 0
    return out


def h_sparse(g, ctx, k, data, start, length):
    return ctx.per_read_sparse(data, start, length, 5)


def d_sparse(g, ctx, k, dev, data, start, length):
    import cfrk_amd
    nS = len(length)
    args = (dev.up(data), dev.up(start), dev.up(length), len(data), nS, 5, 0, dev.room((nS + 1) * 8))
    with pytest.raises(cfrk_amd.CfrkError) as e:
        ctx.per_read_sparse_device(*args, 0, 0, 0)
    assert e.value.code == CFRK_ERR_SMALL_BUF
    nnz = e.value.nnz
    keys, counts = dev.room(nnz * 8), dev.room(nnz * 4)
    assert ctx.per_read_sparse_device(*args, keys, counts, nnz) == nnz
    return dev.down(args[7], nS + 1, np.int64), dev.down(keys, nnz, np.uint64), dev.down(counts, nnz, np.uint32)


def h_sketch(g, ctx, k, data, start, length):
    regs, windows = ctx.distinct_sketch(data, k, 0, start, length)
    return regs, np.array([windows])


def d_sketch(g, ctx, k, dev, data, start, length):
    import cfrk_amd
    regs = dev.up(np.zeros(cfrk_amd.CFRK_SKETCH_REGS, np.uint8))
    windows = ctx.distinct_sketch_device(dev.up(data), len(data), k, 0, regs)
    return dev.down(regs, cfrk_amd.CFRK_SKETCH_REGS, np.uint8), np.array([windows])


def h_dense(g, ctx, k, data, start, length):
    return (ctx.per_read_dense(data, start, length, 5, 0),)


def d_dense(g, ctx, k, dev, data, start, length):
    nS = len(length)
    out = dev.room(nS * 1024 * 4)
    ctx.check(ctx._L.cfrk_per_read_dense_device(ctx._h, dev.up(data), dev.up(start), dev.up(length), len(data), nS, 5, 0, out),
              "cfrk_per_read_dense_device")
    return (dev.down(out, nS * 1024, np.int32).reshape(nS, 1024),)


def _keys(g, data, k):
    """keys to look up: counted ones, and ones with the last base changed (inside the key range, most of them absent)"""
    lo, hi, _ = g.export()
    return np.concatenate([lo[::2], lo[::3] ^ np.uint64(1)]), np.concatenate([hi[::2], hi[::3]])


def h_query(g, ctx, k, data, start, length):
    lo, hi = _keys(g, data, k)
    return (g.query(lo, hi if k > 32 else None),)


def d_query(g, ctx, k, dev, data, start, length):
    lo, hi = _keys(g, data, k)
    out = dev.room(len(lo) * 4)
    g.query_device(dev.up(lo), dev.up(hi) if k > 32 else 0, len(lo), out)
    return (dev.down(out, len(lo), np.uint32),)


# name -> (host, device, job: None / "empty" / "counted", checks a table)
FORMS = {
    "global_add": (h_add, d_add, "empty", True),
    "global_query_reads": (h_query_reads, d_query_reads, "counted", True),
    "global_read_stats": (h_read_stats, d_read_stats, "counted", True),
    "global_read_spans": (h_read_spans, d_read_spans, "counted", True),
    "reads_select": (h_select, d_select, None, True),
    "per_read_sparse": (h_sparse, d_sparse, None, True),
    "distinct_sketch": (h_sketch, d_sketch, None, True),
    "per_read_dense": (h_dense, d_dense, None, False),
    "global_query": (h_query, d_query, "counted", False),
}
TABLE_FORMS = [n for n, f in FORMS.items() if f[3]]


def _job(ctx, kind, k, reads):
    import cfrk_amd
    if kind is None:
        return None
    g = cfrk_amd.GlobalCounter(ctx, k, 0, 1 << 12)
    if kind == "counted":
        g.add(*reads)
    return g


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and (x.tobytes() == y.tobytes())


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", list(FORMS))
def test_host_form_equals_device_form(ctx, dev, reads, name, k):
    host, device, kind, _ = FORMS[name]
    got = host(_job(ctx, kind, k, reads), ctx, k, *reads)
    want = device(_job(ctx, kind, k, reads), ctx, k, dev, *reads)
    _same(got, want)
    assert sum(x.size for x in want) > 0


@pytest.mark.parametrize("k", KS)
def test_bad_table_is_refused_alike_and_the_next_call_is_right(ctx, dev, reads, k):
    import cfrk_amd
    data, start, length = reads
    bad = start.copy()
    bad[1] += 1
    texts = {}
    for name in TABLE_FORMS:
        host, device, kind, _ = FORMS[name]
        want = device(_job(ctx, kind, k, reads), ctx, k, dev, *reads)
        g = _job(ctx, kind, k, reads)
        with pytest.raises(cfrk_amd.CfrkError) as e:
            host(g, ctx, k, data, bad, length)
        assert e.value.code == CFRK_ERR_LAYOUT, name
        texts[name] = ctx._L.cfrk_last_error(ctx._h).decode()
        _same(host(g, ctx, k, data, start, length), want)      # the same job, the same pool: nothing of the refused call is left
    assert set(texts.values()) == {"read 1: start 2, expected 1"}, texts


def test_select_one_below_the_need(ctx, dev, reads):
    rc, nN, nS, _ = _select_dev_raw(ctx, dev, *reads, 0, 0)
    assert (rc, nS) == (CFRK_ERR_SMALL_BUF, 2) and nN == (3 + 1) + (200 + 1)
    want = _select_dev_raw(ctx, dev, *reads, nN, nS)
    assert want[0] == 0 and list(want[3][3]) == [1, 3]
    for cap in ((nN - 1, nS), (nN, nS - 1)):
        h, d = _select_host_raw(ctx, *reads, *cap), _select_dev_raw(ctx, dev, *reads, *cap)
        assert h[:3] == d[:3] == (CFRK_ERR_SMALL_BUF, nN, nS), cap
    got = _select_host_raw(ctx, *reads, nN, nS)
    assert got[:3] == (0, nN, nS)
    _same(got[3], want[3])


def _parse_host_raw(ctx, fn, text, arg, cap_data, cap_reads):
    t = np.frombuffer(text, np.uint8)
    o = (np.empty(cap_data, np.int8), np.empty(cap_reads, np.int64), np.empty(cap_reads, np.int32))
    nN, nS = C.c_int64(-1), C.c_int64(-1)
    rc = getattr(ctx._L, fn)(ctx._h, _ptr(t), t.size, arg, _ptr(o[0]), cap_data, _ptr(o[1]), _ptr(o[2]), cap_reads, C.byref(nN), C.byref(nS))
    return rc, nN.value, nS.value, o


def _parse_dev_raw(ctx, dev, method, text, arg, cap_data, cap_reads):
    import cfrk_amd
    o = (dev.room(cap_data), dev.room(cap_reads * 8), dev.room(cap_reads * 4))
    try:
        nN, nS = getattr(ctx, method)(dev.up(np.frombuffer(text, np.uint8)), len(text), arg, o[0], cap_data, o[1], o[2], cap_reads)
    except cfrk_amd.CfrkError as e:
        return e.code, e.nN, e.nS, None
    return 0, nN, nS, (dev.down(o[0], nN, np.int8), dev.down(o[1], nS, np.int64), dev.down(o[2], nS, np.int32))


@pytest.mark.parametrize("fn,method,text,arg,lengths", [
    ("cfrk_fasta_parse", "parse_fasta_device", FASTA, 0, [5, 18, 4, 13]),
    ("cfrk_fasta_parse", "parse_fasta_device", FASTA, 1, None),                 # CFRK_COMPAT: the reference's reader
    ("cfrk_fastq_parse", "parse_fastq_device", FASTQ, 0, [5, 18, 4, 13]),
    ("cfrk_fastq_parse", "parse_fastq_device", FASTQ, 20, [5, 18, 4, 13]),      # bases below Q20 masked
], ids=["fasta", "fasta-compat", "fastq", "fastq-q20"])
def test_parser_host_form_equals_device_form_and_one_below_the_need(ctx, dev, fn, method, text, arg, lengths):
    rc, nN, nS, _ = _parse_dev_raw(ctx, dev, method, text, arg, 0, 0)
    assert rc == CFRK_ERR_SMALL_BUF and nN > 0 and nS > 0
    want = _parse_dev_raw(ctx, dev, method, text, arg, nN, nS)
    assert want[0] == 0 and (lengths is None or list(want[3][2]) == lengths)
    for cap in ((nN - 1, nS), (nN, nS - 1)):
        h, d = _parse_host_raw(ctx, fn, text, arg, *cap), _parse_dev_raw(ctx, dev, method, text, arg, *cap)
        assert h[:3] == d[:3] == (CFRK_ERR_SMALL_BUF, nN, nS), cap
    got = _parse_host_raw(ctx, fn, text, arg, nN, nS)
    assert got[:3] == (0, nN, nS)
    _same(got[3], want[3])
