"""GPU: paired-end reads -- the join of keep decisions (cfrk_reads_pair_keep / _device), the mate-name check
(cfrk_text_pair_check / _device) and paired normalisation (cfrk_global_normalize_pairs / _device) -- held EQUAL to the
plain-Python rules of tests/pair_ref.py.  Shapes are the smallest that cross the seams: wave and workgroup edges of the
join and more pairs than its grid has threads, names on both sides of the 256-byte class boundary and at every offset
mod 16, mates of a pair in different size classes of the normalise kernels."""
import ctypes as C
import functools

import numpy as np
import pytest

from . import normalize_ref as nr
from . import pair_ref as pr

pytestmark = pytest.mark.gpu

SPAN = np.dtype([("offset", "<i4"), ("length", "<i4")])


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


class Dev:
    """numpy arrays on the device for the length of a with block"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ctx.sync()
        for p in self.ptrs:
            self.ctx.free(p)

    def room(self, nbytes):
        p = self.ctx.alloc(max(int(nbytes), 1) + 16)
        self.ptrs.append(p)
        return p

    def up(self, arr):
        if arr is None:
            return 0
        arr = np.ascontiguousarray(arr)
        p = self.room(arr.nbytes)
        if arr.nbytes:
            self.ctx.h2d(p, arr)
        return p

    def down(self, p, n, dtype=np.uint8):
        out = np.zeros(n, dtype)
        if out.nbytes:
            self.ctx.d2h(out, p)
        return out


# ------------------------------------------------------------------ join

JOIN_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 70_001, 600_001]     # (the last: more pairs than the grid has threads)
MIN_LEN = 20


@functools.lru_cache(maxsize=None)
def _join_input(n):
    """2n reads (interleaved order): keep bytes of 0 / 1 / 255, lengths around MIN_LEN, spans that are fine, negative,
    past the read, and exactly MIN_LEN long"""
    rng = np.random.default_rng([n, 11])
    m = 2 * n
    keep = rng.choice(np.array([0, 1, 255], np.uint8), m, p=[0.3, 0.4, 0.3])
    length = rng.integers(MIN_LEN - 2, MIN_LEN + 30, m).astype(np.int32)
    span = np.zeros(m, SPAN)
    span["offset"] = rng.integers(0, 6, m)
    span["length"] = np.maximum(length - span["offset"] - rng.integers(0, 12, m), 0)
    kind = rng.integers(0, 10, m)
    span["offset"][kind == 0] = -1
    span["length"][kind == 1] = -3
    span["length"][kind == 2] = length[kind == 2] - span["offset"][kind == 2] + 1     # one base past the read
    span["length"][kind == 3] = MIN_LEN                                               # exactly at min_len (inside or not)
    span["length"][kind == 4] = MIN_LEN - 1
    for a in (keep, length, span):
        a.setflags(write=False)
    return keep, span, length


# which of (keep, span, orphans) are passed, and min_len
VARIANTS = [(True, True, True, MIN_LEN), (True, False, True, MIN_LEN), (False, True, False, MIN_LEN), (False, False, True, 0),
            (True, False, False, 0), (False, False, True, MIN_LEN)]


@functools.lru_cache(maxsize=None)
def _survive(n, use_keep, use_span, min_len, need_length):
    keep, span, length = _join_input(n)
    return tuple(pr.survive_all(2 * n, keep if use_keep else None, span if use_span else None, length if need_length else None, min_len))


@functools.lru_cache(maxsize=None)
def _join_want(n, use_keep, use_span, min_len, mode, need_length):
    sv = _survive(n, use_keep, use_span, min_len, need_length)
    return pr.join(sv[0::2], sv[1::2], mode)


@pytest.mark.parametrize("n", JOIN_SIZES)
def test_join_device_form_both_strides(ctx, n):
    keep, span, length = _join_input(n)
    for mode in (pr.BOTH, pr.EITHER):
        for use_keep, use_span, use_orph, min_len in (VARIANTS if n <= 257 else VARIANTS[:1]):
            need_length = use_span or min_len > 0
            pair, oa, ob, counts = _join_want(n, use_keep, use_span, min_len, mode, need_length)
            for stride in (2, 1):
                # interleaved: one array, b = a + one element; split: the even and the odd elements as two arrays
                sides = [(keep, span, length)] if stride == 2 else [(keep[0::2], span[0::2], length[0::2]), (keep[1::2], span[1::2], length[1::2])]
                with Dev(ctx) as d:
                    ptr = []
                    for k_, s_, l_ in sides:
                        ptr.append((d.up(k_) if use_keep else 0, d.up(s_) if use_span else 0, d.up(l_) if need_length else 0))
                    if stride == 2:
                        ka, sa, la = ptr[0]
                        ptr.append((ka + 1 if ka else 0, sa + 8 if sa else 0, la + 4 if la else 0))
                    out = d.up(np.full(2 * n, 7, np.uint8))
                    orph = d.up(np.full(2 * n, 7, np.uint8))
                    step = 1 if stride == 2 else n
                    got = ctx.pair_keep_device(n, stride, mode, min_len, ptr[0][0], ptr[1][0], ptr[0][1], ptr[1][1], ptr[0][2], ptr[1][2],
                                               out, out + step, orph if use_orph else 0, orph + step if use_orph else 0)
                    o, r = d.down(out, 2 * n), d.down(orph, 2 * n)
                what = (n, mode, use_keep, use_span, use_orph, min_len, stride)
                oa_got, ob_got = (r[0::2], r[1::2]) if stride == 2 else (r[:n], r[n:])
                pa_got, pb_got = (o[0::2], o[1::2]) if stride == 2 else (o[:n], o[n:])
                assert (pa_got == pair).all() and (pb_got == pair).all(), what
                if use_orph:
                    assert (oa_got == oa).all() and (ob_got == ob).all(), what
                else:
                    assert (r == 7).all(), what
                assert tuple(int(x) for x in got) == counts, what
                assert set(np.unique(o)) <= {0, 1} and (not use_orph or set(np.unique(r)) <= {0, 1}), what


@pytest.mark.parametrize("n", [1, 65, 257, 70_001])
def test_join_in_place(ctx, n):
    """the outputs are the keep inputs, as the paired normalise call uses the join; no counts: no synchronisation"""
    keep, span, length = _join_input(n)
    for mode in (pr.BOTH, pr.EITHER):
        pair, _, _, counts = _join_want(n, True, True, MIN_LEN, mode, True)
        with Dev(ctx) as d:
            k_, s_, l_ = d.up(keep), d.up(span), d.up(length)
            assert ctx.pair_keep_device(n, 2, mode, MIN_LEN, k_, k_ + 1, s_, s_ + 8, l_, l_ + 4, k_, k_ + 1, want_counts=False) is None
            got = d.down(k_, 2 * n)
        assert (got[0::2] == pair).all() and (got[1::2] == pair).all(), (n, mode)
        # split, in place, with the counts row
        with Dev(ctx) as d:
            ka, kb = d.up(keep[0::2]), d.up(keep[1::2])
            row = ctx.pair_keep_device(n, 1, mode, 0, ka, kb, 0, 0, 0, 0, ka, kb)
            a, b = d.down(ka, n), d.down(kb, n)
        want = _join_want(n, True, False, 0, mode, False)
        assert (a == want[0]).all() and (b == want[0]).all() and tuple(int(x) for x in row) == want[3], (n, mode)


@pytest.mark.parametrize("n", [0, 1, 64, 257, 70_001])
def test_join_host_form(ctx, n):
    import cfrk_amd
    keep, span, length = _join_input(n)
    for mode in (pr.BOTH, pr.EITHER):
        for use_keep, use_span, _, min_len in VARIANTS[:4]:
            need_length = use_span or min_len > 0
            want = _join_want(n, use_keep, use_span, min_len, mode, need_length)
            pair, oa, ob, row = ctx.pair_keep(keep[0::2] if use_keep else None, keep[1::2] if use_keep else None,
                                              span[0::2] if use_span else None, span[1::2] if use_span else None,
                                              length[0::2] if need_length else None, length[1::2] if need_length else None,
                                              min_len, mode, n_pairs=n)
            what = (n, mode, use_keep, use_span, min_len)
            assert (pair == want[0]).all() and (oa == want[1]).all() and (ob == want[2]).all(), what
            assert tuple(int(x) for x in row) == want[3], what
    # interleaved through the C entry point: the bytes between the addressed ones are not the call's to write
    if n:
        want = _join_want(n, True, True, MIN_LEN, pr.BOTH, True)
        out, orph = np.full(2 * n, 9, np.uint8), np.full(2 * n, 9, np.uint8)
        row = np.zeros(1, cfrk_amd.PAIR_COUNTS_DTYPE)
        p = lambda a, off=0: C.c_void_p(a.ctypes.data + off)
        rc = ctx._L.cfrk_reads_pair_keep(ctx._h, n, 2, pr.BOTH, MIN_LEN, p(keep), p(keep, 1), p(span), p(span, 8), p(length), p(length, 4),
                                         p(out), p(out, 1), p(orph), None, p(row))
        assert rc == 0
        assert (out[0::2] == want[0]).all() and (out[1::2] == want[0]).all() and (orph[0::2] == want[1]).all() and (orph[1::2] == 9).all()
        assert tuple(int(x) for x in row[0]) == want[3]


def test_join_argument_errors(ctx):
    import cfrk_amd
    with Dev(ctx) as d:
        buf = d.up(np.zeros(64, np.uint8))
        ok = dict(n_pairs=4, stride=2, mode=pr.BOTH, min_len=0, d_keep_a=buf, d_keep_b=buf + 1, d_span_a=0, d_span_b=0, d_length_a=0, d_length_b=0,
                  d_pair_a=buf, d_pair_b=buf + 1)
        ctx.pair_keep_device(**ok)
        for change in (dict(n_pairs=-1), dict(min_len=-1), dict(stride=0), dict(stride=3), dict(mode=2), dict(mode=-1), dict(min_len=1),
                       dict(d_span_a=buf), dict(d_span_b=buf, d_length_a=buf), dict(d_pair_a=0), dict(d_pair_b=0)):
            with pytest.raises(cfrk_amd.CfrkError) as e:
                ctx.pair_keep_device(**dict(ok, **change))
            assert e.value.code == -1, change
        assert tuple(ctx.pair_keep_device(**dict(ok, n_pairs=0, d_pair_a=0, d_pair_b=0))) == (0, 0, 0, 0)
    with pytest.raises(cfrk_amd.CfrkError) as e:
        ctx.pair_keep(keep_a=np.ones(3, np.uint8), keep_b=np.ones(3, np.uint8), min_len=5)
    assert e.value.code == -1


# ------------------------------------------------------------------ mate names

def _fasta(names_a, names_b, lead=b""):
    """interleaved FASTA text of the mates' header lines (behind `lead`, which belongs to no record)"""
    return lead + b"".join(b">" + a + b"\nACGT\n>" + b + b"\nTTGA\n" for a, b in zip(names_a, names_b))


def _fastq(names):
    return b"".join(b"@" + a + b"\nACGT\n+\nIIII\n" for a in names)


def _check_all_forms(ctx, text_a, rec_a, text_b, rec_b, want, what):
    """host and device form of one check; rec_b None: interleaved in text_a"""
    assert ctx.check_pairs(text_a, rec_a, text_b, rec_b) == want, (what, "host")
    with Dev(ctx) as d:
        ta, ra = d.up(np.frombuffer(text_a, np.uint8)), d.up(rec_a)
        if rec_b is None:
            got = ctx.check_pairs_device(len(rec_a) // 2, 2, ta, len(text_a), ra, ta, len(text_a), ra + 24)
        else:
            tb, rb = d.up(np.frombuffer(text_b, np.uint8)), d.up(rec_b)
            got = ctx.check_pairs_device(len(rec_a), 1, ta, len(text_a), ra, tb, len(text_b), rb)
    assert got == want, (what, "device")


GOOD = [(b"r1/1", b"r1/2"), (b"M01:8:000-AB:1:1101:15:13 1:N:0:ACGT", b"M01:8:000-AB:1:1101:15:13 2:N:0:ACGT"), (b"same\tx", b"same y"),
        (b"plain", b"plain"), (b"a/1", b"a/2"), (b"q/1 left", b"q/2\tright"), (b"r/1", b"r/1"), (b"x/2", b"x/2")]
BAD = [(b"", b""), (b"read_17x", b"read_17y"), (b"r5/2", b"r5/1"), (b"/1", b"/2"), (b"ab", b"abc"), (b" lead", b" lead"), (b"r/1", b"r"),
       (b"r/1", b"r/3"), (b"r", b"r/2"), (b"\t", b"\t")]


def test_names_good_and_bad_forms(ctx):
    import cfrk_amd
    for names in (GOOD, BAD, GOOD + BAD[:1] + GOOD + BAD[3:6] + GOOD, BAD[2:3] + GOOD):
        text = _fasta([a for a, _ in names], [b for _, b in names])
        rec = ctx.index_text(text, cfrk_amd.CFRK_TEXT_FASTA)
        assert len(rec) == 2 * len(names)
        want = pr.check_pairs(text, rec[0::2], text, rec[1::2])
        bad = [j for j, x in enumerate(names) if x in BAD]
        assert want == ((bad[0] if bad else -1), len(bad)), names      # (the reference against the hand-made lists)
        _check_all_forms(ctx, text, rec, None, None, want, names)


def test_names_split_fastq_texts_of_unequal_size(ctx):
    import cfrk_amd
    names = GOOD + BAD[1:4] + GOOD[:3]
    ta = _fastq([a for a, _ in names])
    tb = b"".join(b"@" + b + b"\nACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIII\n" for _, b in names)
    ra, rb = ctx.index_text(ta, cfrk_amd.CFRK_TEXT_FASTQ), ctx.index_text(tb, cfrk_amd.CFRK_TEXT_FASTQ)
    assert len(ra) == len(rb) == len(names) and len(ta) != len(tb)
    want = pr.check_pairs(ta, ra, tb, rb)
    assert want == (len(GOOD), 3)
    _check_all_forms(ctx, ta, ra, tb, rb, want, "split fastq")


def test_names_one_long_name_among_short_ones(ctx):
    """a 20 000-byte name among 300 short ones: good, then bad in its last byte, then bad in the last byte in front of a
    comment; and names on both sides of the fast class's 256 bytes"""
    import cfrk_amd
    rng = np.random.default_rng(8)
    long_name = bytes(rng.integers(ord("a"), ord("z") + 1, 20_000).astype(np.uint8))
    short = [b"read%d" % i for i in range(300)]
    for tail_a, tail_b, n_bad in ((b"", b"", 0), (b"x", b"y", 1), (b"x 1:N", b"y 2:N", 1), (b"/1", b"/2", 0), (b" 1", b"\t2", 0), (b"/2", b"/1", 1)):
        a = short[:137] + [long_name + tail_a] + short[137:]
        b = short[:137] + [long_name + tail_b] + short[137:]
        text = _fasta(a, b)
        rec = ctx.index_text(text, cfrk_amd.CFRK_TEXT_FASTA)
        want = pr.check_pairs(text, rec[0::2], text, rec[1::2])
        assert want == ((137 if n_bad else -1), n_bad)
        _check_all_forms(ctx, text, rec, None, None, want, (tail_a, tail_b))
    a, b = [], []
    for L in (15, 16, 17, 31, 32, 33, 254, 255, 256, 257, 258, 300, 511, 512, 513, 4095, 4096, 4097):
        base = bytes(rng.integers(ord("A"), ord("Z") + 1, L).astype(np.uint8))
        other = base[:-1] + b"!"
        a += [base, base, base + b"/1", base[:L // 2] + b" " + base[L // 2 + 1:], base, base + b" c"]
        b += [base, other, base + b"/2", base[:L // 2] + b" " + other[L // 2 + 1:], base + b"z", other + b" c"]
    text = _fasta(a, b)
    rec = ctx.index_text(text, cfrk_amd.CFRK_TEXT_FASTA)
    want = pr.check_pairs(text, rec[0::2], text, rec[1::2])
    assert want[1] == 3 * 18 and want[0] == 1
    _check_all_forms(ctx, text, rec, None, None, want, "class boundary")


def test_names_at_every_offset_mod_16(ctx):
    import cfrk_amd
    names = GOOD[:4] + BAD[1:3] + [(b"n" * 40 + b"/1", b"n" * 40 + b"/2"), (b"m" * 40, b"m" * 39 + b"w")]
    for lead in range(16):
        text = _fasta([a for a, _ in names], [b for _, b in names], b"#" * lead + b"\n" if lead else b"")
        rec = ctx.index_text(text, cfrk_amd.CFRK_TEXT_FASTA)
        want = pr.check_pairs(text, rec[0::2], text, rec[1::2])
        assert want == (4, 3)
        _check_all_forms(ctx, text, rec, None, None, want, lead)


def test_names_record_outside_the_text_and_errors(ctx):
    import cfrk_amd
    text = _fasta([a for a, _ in GOOD], [b for _, b in GOOD])
    rec0 = ctx.index_text(text, cfrk_amd.CFRK_TEXT_FASTA)
    for j, field, value in ((3, "head_off", -1), (5, "head_len", -2), (6, "head_off", len(text) + 1), (9, "head_len", len(text)),
                            (10, "head_off", 1 << 40), (15, "head_len", 0x7FFFFFFF)):
        rec = rec0.copy()
        rec[field][j] = value
        want = pr.check_pairs(text, rec[0::2], text, rec[1::2])
        assert want == (j // 2, 1)
        _check_all_forms(ctx, text, rec, None, None, want, (j, field, value))
    assert ctx.check_pairs(b"", rec0[:0]) == (-1, 0)
    with pytest.raises(ValueError):
        ctx.check_pairs(text, rec0[:3])
    for n, stride in ((-1, 2), (2, 0), (2, 3)):
        with pytest.raises(cfrk_amd.CfrkError) as e:
            ctx.check_pairs_device(n, stride, 0, 0, 0, 0, 0, 0)
        assert e.value.code == -1
    with pytest.raises(cfrk_amd.CfrkError) as e:
        ctx.check_pairs_device(2, 2, 0, 0, 0, 0, 0, 0)              # NULL records
    assert e.value.code == -1


# ------------------------------------------------------------------ paired normalisation

NK = [15, 31, 63]
CUTOFF = 5


@functools.lru_cache(maxsize=None)
def _pairs_set():
    """about 200 pairs at coverage ~30 of a 2 kb genome (read twice over, so that long reads can be drawn): mostly
    150 + 150, some 150 + 1000 and 150 + one read beyond the fast path (2048 + 63 windows and more), a mate of invalid
    codes only, a mate too short for a window; both strands; fixed shuffled order"""
    rng = np.random.default_rng(77)
    genome = rng.integers(0, 4, 2000).astype(np.int8)
    g2 = np.concatenate([genome, genome, genome])
    shapes = [(150, 150)] * 170 + [(150, 1000), (1000, 150)] * 4 + [(150, 2048 + 63 + 40), (2048 + 63 + 1, 150)] + [(150, 0), (10, 150), (150, 150)] * 2
    shapes = [shapes[i] for i in rng.permutation(len(shapes))]
    rows = []
    for j, (la, lb) in enumerate(shapes):
        for L in (la, lb):
            p = int(rng.integers(0, len(genome)))
            r = g2[p:p + L].copy()
            if rng.integers(0, 2):
                r = (3 - r[::-1]).astype(np.int8)
            rows.append(r)
        if j % 29 == 3:
            rows[-1][:] = -1                                      # a mate made of invalid codes only
        if j % 31 == 7 and len(rows[-2]):
            rows[-2][len(rows[-2]) // 2] = 4
    length = np.array([len(r) for r in rows], np.int32)
    start = np.concatenate([[0], np.cumsum(length[:-1].astype(np.int64) + 1)]).astype(np.int64)
    data = np.full(int(length.sum()) + len(rows), -1, np.int8)
    for s, r in zip(start, rows):
        data[s:s + len(r)] = r
    for a in (data, start, length):
        a.setflags(write=False)
    return data, start, length


@functools.lru_cache(maxsize=None)
def _pairs_keys(k, canonical):
    data, start, length = _pairs_set()
    return tuple(tuple(x) for x in nr.all_read_keys(data, start, length, k, canonical))


def _flags(canonical):
    import cfrk_amd
    return cfrk_amd.CFRK_CANONICAL if canonical else 0


def _assert_job(g, counts, two, what):
    wlo, whi, wcnt = nr.export_arrays(counts)
    lo, hi, cnt = g.export()
    assert len(lo) == len(wlo), (what, "distinct", len(lo), len(wlo))
    assert (lo == wlo).all() and (cnt == wcnt).all() and (not two or (hi == whi).all()), what
    assert g.digest() == nr.digest(counts, two), what


def _assert_keep(got, want, what):
    keep, n = got
    bad = np.nonzero(keep != want[0])[0]
    assert len(bad) == 0, (what, "keep differs at reads", bad[:10], keep[bad[:10]], want[0][bad[:10]])
    assert n == want[1] and n % 2 == 0, (what, n, want[1])
    assert (keep[0::2] == keep[1::2]).all(), what


def _norm_cases():
    nS = len(_pairs_set()[2])
    return [(k, c, m, b) for k in NK for c in (False, True) for m in (pr.EITHER, pr.BOTH) for b in (2, 64, nS, 2 * nS)]


@pytest.mark.parametrize("k,canonical,mode,batch", _norm_cases())
def test_normalize_pairs_matches_reference(ctx, k, canonical, mode, batch):
    import cfrk_amd
    data, start, length = _pairs_set()
    keys = _pairs_keys(k, canonical)
    g = cfrk_amd.GlobalCounter(ctx, k, _flags(canonical), 1 << 15)
    want = pr.normalize_pairs_keys(keys, CUTOFF, batch, mode)
    what = (k, canonical, mode, batch)
    _assert_keep(g.normalize_pairs(data, start, length, CUTOFF, batch, mode), want, what)
    _assert_job(g, want[2], k > 32, what)
    if batch <= 64:
        assert 0.1 < want[0].mean() < 0.9, "the verdicts do not flip during the call"
    if mode == pr.EITHER:
        empty = np.array([len(x) == 0 for x in keys])
        assert want[0][empty].any(), "no mate without a window is kept through its partner"
    # the job is an ordinary job afterwards: a plain normalise call on it continues from the same counts
    counts = dict(want[2])
    want2 = nr.normalize_keys(keys, CUTOFF + 3, 7, counts)
    keep2, n2 = g.normalize(data, start, length, CUTOFF + 3, 7)
    assert (keep2 == want2[0]).all() and n2 == want2[1], what
    _assert_job(g, want2[2], k > 32, (what, "plain call behind"))


@pytest.mark.parametrize("cutoff", [0, 0xFFFFFFFF])
def test_normalize_pairs_cutoff_extremes(ctx, cutoff):
    import cfrk_amd
    data, start, length = _pairs_set()
    for mode in (pr.EITHER, pr.BOTH):
        g = cfrk_amd.GlobalCounter(ctx, 31, cfrk_amd.CFRK_CANONICAL, 1 << 15)
        want = pr.normalize_pairs_keys(_pairs_keys(31, True), cutoff, 64, mode)
        _assert_keep(g.normalize_pairs(data, start, length, cutoff, 64, mode), want, (cutoff, mode))
        _assert_job(g, want[2], False, (cutoff, mode))
        assert want[1] == 0 if cutoff == 0 else want[1] > 0


@pytest.mark.parametrize("k", NK)
def test_normalize_pairs_device_form_with_ranges_outside_the_buffer(ctx, k):
    """unchecked start / length: one mate of some pairs does not lie inside [0, nN): it has no windows, never a fault"""
    import cfrk_amd
    data, start, length = _pairs_set()
    start, length = start.copy(), length.copy()
    nS, nN = len(length), len(data)
    start[4], start[11], start[20], length[33], start[41] = -5, nN - 10, nN + 7, -1, -(1 << 40)
    length[52] = 0x7FFFFFFF
    keys = nr.all_read_keys(data, start, length, k, True)
    assert not keys[4] and not keys[11] and not keys[52]
    for mode in (pr.EITHER, pr.BOTH):
        want = pr.normalize_pairs_keys(keys, CUTOFF, 64, mode)
        g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, 1 << 15)
        with Dev(ctx) as d:
            d_data, d_start, d_length, d_keep = d.up(data), d.up(start), d.up(length), d.up(np.full(nS, 9, np.uint8))
            n = g.normalize_pairs_device(d_data, d_start, d_length, nN, nS, CUTOFF, d_keep, 64, mode)
            keep = d.down(d_keep, nS)
        _assert_keep((keep, n), want, (k, mode))
        _assert_job(g, want[2], k > 32, (k, mode))


def test_normalize_pairs_of_identical_mates_equals_the_unpaired_call(ctx):
    """every read duplicated as its own mate, EITHER: both mates get the same verdict, the join changes nothing, and the
    paired call is the unpaired call on the same reads at the same batch"""
    import cfrk_amd
    data, start, length = _pairs_set()
    rows = [data[s:s + l] for s, l in zip(start[:160], length[:160]) for _ in (0, 1)]
    ln = np.array([len(r) for r in rows], np.int32)
    st = np.concatenate([[0], np.cumsum(ln[:-1].astype(np.int64) + 1)]).astype(np.int64)
    dd = np.full(int(ln.sum()) + len(rows), -1, np.int8)
    for s, r in zip(st, rows):
        dd[s:s + len(r)] = r
    for k, batch in ((15, 2), (31, 64), (63, 320)):
        for mode in (pr.EITHER, pr.BOTH):
            a = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, 1 << 15)
            keep_a, n_a = a.normalize_pairs(dd, st, ln, CUTOFF, batch, mode)
            exp_a, dig_a = a.export(), a.digest()
            b = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, 1 << 15)
            keep_b, n_b = b.normalize(dd, st, ln, CUTOFF, batch)
            assert (keep_a == keep_b).all() and n_a == n_b and dig_a == b.digest(), (k, batch, mode)
            assert all((x == y).all() for x, y in zip(exp_a, b.export())), (k, batch, mode)
            assert 0 < n_a < len(ln)


def test_normalize_pairs_argument_errors(ctx):
    import cfrk_amd
    data, start, length = _pairs_set()
    g = cfrk_amd.GlobalCounter(ctx, 31, 0, 1 << 15)
    for args in ((data[:int(start[3])], start[:3], length[:3], CUTOFF, 2, pr.EITHER),        # odd nS
                 (data, start, length, CUTOFF, 3, pr.EITHER),                                # odd batch
                 (data, start, length, CUTOFF, 0, pr.EITHER),
                 (data, start, length, CUTOFF, 2, 2), (data, start, length, CUTOFF, 2, -1)):  # no such mode
        with pytest.raises(cfrk_amd.CfrkError) as e:
            g.normalize_pairs(*args)
        assert e.value.code == -1, args[3:]
    assert g.digest()[0] == 0                                     # nothing was counted
    keep, n = g.normalize_pairs(data[:0], start[:0], length[:0], CUTOFF, 2)
    assert len(keep) == 0 and n == 0
