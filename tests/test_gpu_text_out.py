"""GPU: the text index (cfrk_text_index / _device) against tests/text_out_ref.py on every text of the parsers' case
modules, on hand-made tile seams and on a text of more than one scan block; the text emitter (cfrk_reads_emit_text /
_device) against the same reference on a mix of reads around the copy's tile, with guard bytes around every output; then
text -> parse -> index -> count -> spans -> emit on the device, and the CLI's --filter-names / --filter-format.  The
library's own calls are never the reference."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from . import fastq_cases as fc
from . import filter_ref as fr
from . import ingest_cases as ic
from . import text_out_ref as tr
from .test_gpu_filter import _Guarded, _noisy_reads, _upload
from .test_gpu_query import _cli, _oracle

pytestmark = pytest.mark.gpu

CFRK_ERR_ARG, CFRK_ERR_ALIGN, CFRK_ERR_LAYOUT, CFRK_ERR_SMALL_BUF = -1, -7, -5, -9
COUNT_MAX = 0xFFFFFFFE
T = ic._header_int("CFRK_TEXT_TILE_BYTES")
ET = ic._header_int("CFRK_EMIT_TILE_BYTES")
REC = tr.RECORD_DTYPE
FORMATS = (tr.TEXT_FASTA, tr.TEXT_FASTQ)


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


def test_error_codes_are_the_headers():
    header = open(os.path.join(ic.ROOT, "include", "cfrk_abi.h")).read()
    for name, value in (("ARG", CFRK_ERR_ARG), ("ALIGN", CFRK_ERR_ALIGN), ("LAYOUT", CFRK_ERR_LAYOUT), ("SMALL_BUF", CFRK_ERR_SMALL_BUF)):
        assert int(re.search(r"#define CFRK_ERR_%s\s+(-\d+)" % name, header).group(1)) == value


# ------------------------------------------------------------------ index

def _device_index(ctx, raw, fmt, cap=None, slack=3):
    """the device form on a guarded record array -> records.  cap None: room for the reference's records and `slack`
    more.  A CfrkError is passed on after the check that nothing was written."""
    import cfrk_amd
    raw = bytes(raw)
    want = len(tr.index_ref(raw, fmt)) if cap is None else 0
    cap = want + slack if cap is None else cap
    d_text = _upload(ctx, np.frombuffer(raw, np.uint8))
    out = _Guarded(ctx, cap * 24)
    try:
        try:
            nS = ctx.index_text_device(d_text if raw else 0, len(raw), fmt, out.ptr, cap)
        except cfrk_amd.CfrkError:
            ctx.sync()
            out.fetch(0)
            raise
        ctx.sync()
        return out.fetch(nS * 24, REC)
    finally:
        ctx.sync()
        ctx.free(d_text)
        out.free()


def _assert_records(got, exp, what):
    assert len(got) == len(exp), (what, len(got), len(exp))
    for f in REC.names:
        bad = np.nonzero(got[f] != exp[f])[0]
        assert len(bad) == 0, (what, f, bad[:5], got[bad[:5]], exp[bad[:5]])


def _fasta_module_texts():
    out = [(c[0], c[1]) for c in ic.grammar_cases() + ic.seam_cases() + ic.cr_run_cases()]
    return out + [(f"random text {i}", t) for i, t in enumerate(ic.random_texts())]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("module", ["fastq_cases", "ingest_cases"])
def test_index_on_every_text_of_the_case_modules(ctx, module, fmt):
    """grammar, refusal and seam cases and the 200 seeded random texts of each module, in both formats"""
    texts = fc.small_cases() if module == "fastq_cases" else _fasta_module_texts()
    assert len(texts) > 230
    records = 0
    for name, raw in texts:
        exp = tr.index_ref(raw, fmt)
        records += len(exp)
        _assert_records(_device_index(ctx, raw, fmt), exp, (module, fmt, name))
    assert records > 200


def _seam_texts():
    rng = np.random.default_rng(181)
    seq, qual = fc._seq(rng, 40), fc._qual(rng, 40)
    body = b"\n" + seq + b"\n+\n" + qual + b"\n"
    first = b"@first\nACGT\n+\nI5I5\n"
    out = []
    for mark in (b"@", b">"):
        # a header line that straddles a tile boundary, and one of three tiles
        t = first + mark + b"n" * (T - len(first) - 10) + b" across" * 4 + body + mark + b"next" + body
        assert t.find(b"\n", len(first)) > T > len(first)
        out.append((f"a '{mark.decode()}' header across a tile boundary", t))
        t = first + mark + b"h" * (3 * T + 17) + body + mark + b"next" + body
        out.append((f"a '{mark.decode()}' header of three tiles", t))
        # '\r' as a tile's last byte, '\n' as the next tile's first -- at the end of a header line
        t = first + mark + b"n" * (T - len(first) - 2) + b"\r" + body + mark + b"x\r" + body
        assert t[T - 1:T + 1] == b"\r\n"
        out.append((f"crlf across a tile boundary behind a '{mark.decode()}' header", t))
        out.append((f"'\\r' as the last byte of a '{mark.decode()}' header", first + mark + b"last\r"))
        out.append((f"a '{mark.decode()}' header without a trailing newline", first + mark + b"last"))
        out.append((f"a '{mark.decode()}' header that ends with a tile", (mark + b"n" * (T - 2) + b"\n") * 2 + mark + b"z" + body))
    # a quality line across a boundary, its '\r' the tile's last byte; the text's end in the middle of a record
    t = b"@q\n" + fc._seq(rng, T - 100) + b"\n+\n" + fc._qual(rng, T - 100) + b"\r\n@r\r\nAC\r\n+\r\nI5\r"
    out.append(("a quality line across a boundary, '\\r' as the text's last byte", t))
    out.append(("a quality line that ends the text", b"@q\nACGT\n+\nI5I5"))
    out.append(("lines of one byte", b"\n" * (T + 7)))
    out.append(("carriage returns only", b"\r" * 40 + b"\n" + b"\r" * 5))
    out.append(("empty text", b""))
    out.append(("sixteen bytes without a newline", b">" + b"a" * 15))
    out.append(("seventeen bytes without a newline", b">" + b"a" * 16))
    out.append(("a tile without a newline", b">" + b"a" * (T - 1)))
    return out


@pytest.mark.parametrize("fmt", FORMATS)
def test_index_hand_made_seams(ctx, fmt):
    for name, raw in _seam_texts():
        _assert_records(_device_index(ctx, raw, fmt), tr.index_ref(raw, fmt), (fmt, name))


@pytest.mark.parametrize("fmt", FORMATS)
def test_index_more_than_one_block_of_the_tile_scan(ctx, fmt):
    raw = fc.scan_block_case() if fmt == tr.TEXT_FASTQ else ic.scan_block_case()
    assert len(raw) > fc.SCAN_TILES * T and len(raw) > ic._header_int("CFRK_TEXT_SCAN_TILES") * T
    exp = tr.index_ref(raw, fmt)
    assert len(exp) > 50000
    _assert_records(_device_index(ctx, raw, fmt), exp, fmt)


def test_index_host_form_equals_device_form(ctx):
    texts = [t for _, t in _seam_texts()] + [t for _, t in fc.grammar_cases()] + fc.random_texts(12, 77) + ic.random_texts(12, 78)
    for raw in texts:
        for fmt in FORMATS:
            host = ctx.index_text(raw, fmt)
            assert host.dtype == REC
            _assert_records(host, _device_index(ctx, raw, fmt), fmt)
            _assert_records(host, tr.index_ref(raw, fmt), fmt)
    assert len(ctx.index_text(np.frombuffer(b">a\nAC\n", np.uint8), tr.TEXT_FASTA)) == 1       # an array as well as bytes


def test_index_capacities(ctx):
    import cfrk_amd
    raw = fc.random_texts(8, 5)[-1] + b"\n" + b"@a\nACGT\n+\nI5I5\n" * 50 + b">x\nAC\n>y\nAC\n"
    for fmt in FORMATS:
        exp = tr.index_ref(raw, fmt)
        nS = len(exp)
        assert nS >= 1
        for cap in (0, nS - 1):                                    # too small by all, by one: nS complete, nothing written
            with pytest.raises(cfrk_amd.CfrkError) as e:
                _device_index(ctx, raw, fmt, cap=cap)
            assert e.value.code == CFRK_ERR_SMALL_BUF and e.value.nS == nS
        _assert_records(_device_index(ctx, raw, fmt, cap=nS), exp, "exactly enough")
        d_text = _upload(ctx, np.frombuffer(raw, np.uint8))
        try:
            with pytest.raises(cfrk_amd.CfrkError) as e:                # sizes only: NULL with capacity 0
                ctx.index_text_device(d_text, len(raw), fmt, 0, 0)
            assert e.value.code == CFRK_ERR_SMALL_BUF and e.value.nS == nS
        finally:
            ctx.free(d_text)
    assert ctx.index_text_device(0, 0, tr.TEXT_FASTQ, 0, 0) == 0        # an empty text has no records


def test_index_arguments(ctx):
    import cfrk_amd
    L = cfrk_amd.load_library()
    raw = np.frombuffer(b"@a\nACGT\n+\nI5I5\n" * 4, np.uint8)
    d_text = _upload(ctx, raw, 0)
    d_rec = ctx.alloc(24 * 8)
    nS = C.c_int64(-1)
    host_rec = np.zeros(8, REC)
    h, vp = ctx._h, C.c_void_p
    try:
        for fn, text in ((L.cfrk_text_index_device, vp(d_text)), (L.cfrk_text_index, raw.ctypes.data_as(vp))):
            rec = vp(d_rec) if fn is L.cfrk_text_index_device else host_rec.ctypes.data_as(vp)
            for fmt in (2, -1):
                assert fn(h, text, raw.size, fmt, rec, 8, C.byref(nS)) == CFRK_ERR_ARG
            assert fn(h, text, raw.size, 1, rec, 8, None) == CFRK_ERR_ARG              # NULL size output
            assert fn(h, None, raw.size, 1, rec, 8, C.byref(nS)) == CFRK_ERR_ARG       # NULL text with nbytes > 0
            assert fn(h, text, raw.size, 1, None, 8, C.byref(nS)) == CFRK_ERR_ARG      # NULL array with cap_reads > 0
            assert fn(h, None, 0, 1, None, 0, C.byref(nS)) == 0 and nS.value == 0
        assert L.cfrk_text_index_device(h, vp(d_text + 8), raw.size - 8, 1, vp(d_rec), 8, C.byref(nS)) == CFRK_ERR_ALIGN
        assert L.cfrk_text_index_device(h, vp(d_text), raw.size, 1, vp(d_rec), 8, C.byref(nS)) == 0 and nS.value == 4
    finally:
        ctx.sync()
        ctx.free(d_text)
        ctx.free(d_rec)


# ------------------------------------------------------------------ emit

def _device_emit(ctx, data, start, length, text, rec, spans=None, keep=None, min_len=0, fmt=tr.TEXT_FASTA, cap=None, skews=(0, 0, 0),
                 sizes_only=False):
    """the device form on a guarded output of its own -> (nbytes, nS, text).  cap None: the reference's size.  A
    CfrkError is passed on after the check that nothing was written."""
    import cfrk_amd
    text = bytes(text)
    nN, nS = len(data), len(start)
    if cap is None:
        cap = len(tr.emit_ref(data, start, length, text, rec, spans, keep, min_len, fmt)[0])
    s_in, s_text, s_out = skews
    ins = [_upload(ctx, data, s_in), _upload(ctx, start), _upload(ctx, length), _upload(ctx, np.frombuffer(text, np.uint8), s_text),
           _upload(ctx, np.ascontiguousarray(rec, REC))]
    d_span = _upload(ctx, spans) if spans is not None else 0
    d_keep = _upload(ctx, np.ascontiguousarray(keep, np.uint8)) if keep is not None else 0
    out = _Guarded(ctx, cap, s_out)
    try:
        try:
            nb, ns = ctx.emit_reads_device(ins[0] + s_in, ins[1], ins[2], nN, nS, d_span, d_keep, min_len, ins[3] + s_text, len(text), ins[4],
                                           fmt, 0 if sizes_only else out.ptr, 0 if sizes_only else cap)
        except cfrk_amd.CfrkError:
            ctx.sync()
            out.fetch(0)
            raise
        ctx.sync()
        return nb, ns, out.fetch(nb).tobytes()
    finally:
        ctx.sync()
        for p in ins + [d_span, d_keep]:
            if p:
                ctx.free(p)
        out.free()


def _assert_text(got, exp, what):
    nb, ns, text = got
    etext, eindex = exp
    assert (nb, ns) == (len(etext), len(eindex)), (what, nb, ns, len(etext), len(eindex))
    if text != etext:
        a, b = np.frombuffer(text, np.uint8), np.frombuffer(etext, np.uint8)
        at = int(np.nonzero(a != b)[0][0])
        assert False, (what, at, text[max(at - 20, 0):at + 20], etext[max(at - 20, 0):at + 20])


def _fastq_of(reads, names, rng, crlf_every=5):
    parts = []
    for i, (s, name) in enumerate(zip(reads, names)):
        eol = b"\r\n" if crlf_every and i % crlf_every == 2 else b"\n"
        parts.append(b"@" + name + eol + s + eol + b"+" + eol + fc._qual(rng, len(s), 33, 127) + eol)
    return b"".join(parts)


_MIX = {}


def _mix(seed=0, fasta=False):
    """-> (text, rec, data, start, length, spans, keep): reads of every length class around the copy's tile with names of
    every size, parsed by the host parser (FASTQ with min_qual 20: masked bases read N), indexed by the reference"""
    if (seed, fasta) in _MIX:
        return _MIX[(seed, fasta)]
    rng = np.random.default_rng(500 + seed)
    lens = [0, 0, 1, 3, 4, 5, 150, ET - 1, ET, ET + 1, 40000] + [int(x) for x in rng.integers(0, 300, 60)]
    order = rng.permutation(len(lens))
    letters = np.frombuffer(b"ACGTACGTACGTNacgt", np.uint8)
    reads = [letters[rng.integers(0, len(letters), lens[i])].tobytes() for i in order]
    names = [b"r%d/%d some text" % (i, seed) if i % 7 else b"" for i in range(len(reads))]
    names[3] = b"n" * 20000                                       # a name of more than a tile
    names[12] = b"odd > @ + name\r"                               # its second '\r' stays (the line end takes one)
    if fasta:
        text = b"".join(b">" + n + b"\n" + b"\n".join(s[o:o + 70] for o in range(0, len(s), 70)) + b"\n" for s, n in zip(reads, names))
        rc, (data, start, length) = ic.host_parse(text, ic.NATIVE)
    else:
        text = _fastq_of(reads, names, rng)
        rc, _, (data, start, length) = fc.host_parse(text, 20)
    assert rc == 0 and len(start) == len(reads)
    rec = tr.index_ref(text, tr.TEXT_FASTA if fasta else tr.TEXT_FASTQ)
    spans = np.zeros(len(reads), tr.SPAN_DTYPE)
    for i, L in enumerate(length):
        off = min(i % 4, int(L))
        spans[i] = (off, int(L) - off if i % 3 else (int(L) - off) // 2)
    keep = rng.random(len(reads)) < 0.7
    _MIX[(seed, fasta)] = (text, rec, data, start, length, spans, keep)
    return _MIX[(seed, fasta)]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("min_len", [0, 1, 21])
def test_emit_vs_reference(ctx, min_len, fmt):
    text, rec, data, start, length, spans, keep = _mix(min_len)
    assert (data == -1).sum() > len(start) + 100 and (length == 0).sum() >= 2 and length.max() == 40000
    for sp, kp, skews in ((spans, keep, (0, 0, 0)), (spans, None, (1, 5, 3)), (None, keep, (2, 11, 15)), (None, None, (3, 0, 8)), (spans, keep, (15, 2, 9))):
        exp = tr.emit_ref(data, start, length, text, rec, sp, kp, min_len, fmt)
        assert 0 < len(exp[1]) < len(start) or (kp is None and min_len == 0)
        what = (fmt, min_len, sp is not None, kp is not None, skews)
        _assert_text(_device_emit(ctx, data, start, length, text, rec, sp, kp, min_len, fmt, skews=skews), exp, what)
        host = ctx.emit_reads(data, start, length, text, rec, sp, kp, min_len, fmt)                # the host form
        _assert_text((len(host), len(exp[1]), host), exp, ("host",) + what)
    import cfrk_amd
    exp = tr.emit_ref(data, start, length, text, rec, spans, keep, min_len, fmt)
    with pytest.raises(cfrk_amd.CfrkError) as e:                    # the sizes-only call: sizes complete, nothing written
        _device_emit(ctx, data, start, length, text, rec, spans, keep, min_len, fmt, sizes_only=True)
    assert e.value.code == CFRK_ERR_SMALL_BUF and (e.value.nbytes, e.value.nS) == (len(exp[0]), len(exp[1]))


def test_emit_fasta_text_and_index(ctx):
    """names from a FASTA text with wrapped sequence lines; FASTQ output has no quality line to copy: every read dropped"""
    text, rec, data, start, length, spans, keep = _mix(3, fasta=True)
    exp = tr.emit_ref(data, start, length, text, rec, spans, keep, 1, tr.TEXT_FASTA)
    assert exp[0].count(b">" + b"n" * 20000 + b"\n") == 1
    _assert_text(_device_emit(ctx, data, start, length, text, rec, spans, keep, 1, tr.TEXT_FASTA, skews=(5, 7, 1)), exp, "fasta")
    assert _device_emit(ctx, data, start, length, text, rec, None, None, 0, tr.TEXT_FASTQ)[:2] == (0, 0)


def test_emit_output_sizes_around_a_tile(ctx):
    """outputs of 2 ET - 1, 2 ET and 2 ET + 1 bytes: the last tile holds one byte less than, exactly and one byte more than a tile"""
    rng = np.random.default_rng(42)
    reads = [fc._seq(rng, int(n)) for n in rng.integers(1, 200, 40)]
    names = [b"s%d" % i for i in range(len(reads) + 1)]
    base = sum(len(s) + len(n) + 3 for s, n in zip(reads, names))
    for size in (2 * ET - 1, 2 * ET, 2 * ET + 1):
        last = fc._seq(rng, size - base - len(names[-1]) - 3)
        text = _fastq_of(reads + [last], names, rng, crlf_every=0)
        rc, _, (data, start, length) = fc.host_parse(text, 0)
        rec = tr.index_ref(text, tr.TEXT_FASTQ)
        exp = tr.emit_ref(data, start, length, text, rec)
        assert rc == 0 and len(exp[0]) == size
        for skew in (0, 7):
            _assert_text(_device_emit(ctx, data, start, length, text, rec, skews=(skew, 0, (3 * skew) % 16)), exp, (size, skew))


def test_emit_more_kept_reads_than_a_scan_block(ctx):
    """one-base reads, more of them kept than CFRK_SELECT_SCAN_TILES x CFRK_SELECT_TILE_READS: the scan walks a second
    block, and the copy's tiles hold 4096 reads each"""
    import cfrk_amd
    rng = np.random.default_rng(13)
    nS = cfrk_amd.CFRK_SELECT_SCAN_TILES * cfrk_amd.CFRK_SELECT_TILE_READS * 9 // 8
    codes = rng.integers(0, 4, nS).astype(np.int8)
    one = np.frombuffer(b">\nA\n", np.uint8)
    text = np.tile(one, nS)
    text[2::4] = np.frombuffer(b"ACGT", np.uint8)[codes]
    data = np.full(2 * nS, -1, np.int8)
    data[0::2] = codes
    start, length = np.arange(nS, dtype=np.int64) * 2, np.ones(nS, np.int32)
    rec = np.zeros(nS, REC)
    rec["head_off"], rec["head_len"], rec["qual_off"] = np.arange(nS, dtype=np.int64) * 4, 1, -1
    _assert_records(rec[:1000], tr.index_ref(text[:4000].tobytes(), tr.TEXT_FASTA), "the records by formula")
    keep = rng.random(nS) < 0.95
    etext = text.reshape(nS, 4)[keep].tobytes()
    assert keep.sum() > cfrk_amd.CFRK_SELECT_SCAN_TILES * cfrk_amd.CFRK_SELECT_TILE_READS
    got = _device_emit(ctx, data, start, length, text.tobytes(), rec, None, keep, 1, tr.TEXT_FASTA, cap=len(etext))
    _assert_text(got, (etext, np.nonzero(keep)[0]), "one-base reads")


def test_emit_nothing_kept_and_no_reads(ctx):
    text, rec, data, start, length, spans, keep = _mix()
    none = np.zeros(len(start), bool)
    for fmt in FORMATS:
        assert _device_emit(ctx, data, start, length, text, rec, spans, none, 0, fmt) == (0, 0, b"")
        assert _device_emit(ctx, data, start, length, text, rec, None, None, 0x7FFFFFFF, fmt) == (0, 0, b"")
        assert ctx.emit_reads(data, start, length, text, rec, spans, none, 0, fmt) == b""
        e = np.zeros(0, np.int8)
        assert _device_emit(ctx, e, e.astype(np.int64), e.astype(np.int32), text, rec[:0], fmt=fmt) == (0, 0, b"")     # nS = 0
        assert ctx.emit_reads(e, e.astype(np.int64), e.astype(np.int32), text, rec[:0], out_format=fmt) == b""


def test_emit_small_buffer_reports_the_sizes_and_writes_nothing(ctx):
    import cfrk_amd
    text, rec, data, start, length, spans, keep = _mix(7)
    for fmt in FORMATS:
        exp = tr.emit_ref(data, start, length, text, rec, spans, keep, 1, fmt)
        for cap in (len(exp[0]) - 1, ET, 1):
            with pytest.raises(cfrk_amd.CfrkError) as e:           # (the helper checks the guard bytes and the array itself)
                _device_emit(ctx, data, start, length, text, rec, spans, keep, 1, fmt, cap=cap, skews=(0, 0, 5))
            assert e.value.code == CFRK_ERR_SMALL_BUF and (e.value.nbytes, e.value.nS) == (len(exp[0]), len(exp[1]))
        _assert_text(_device_emit(ctx, data, start, length, text, rec, spans, keep, 1, fmt, cap=len(exp[0])), exp, "exactly enough")


def test_emit_drops_on_the_device_and_refuses_on_the_host(ctx):
    import cfrk_amd
    text, rec, data, start, length, spans, keep = _mix(5)
    nb = len(text)
    a, b, c, d = [int(i) for i in np.nonzero(length > 20)[0][:4]]
    cases = []
    sp = spans.copy(); sp[a] = (-1, 5); cases.append(("a negative span offset", sp, rec, a, FORMATS))
    sp = spans.copy(); sp[b] = (2, int(length[b])); cases.append(("a span longer than its read", sp, rec, b, FORMATS))
    r = rec.copy(); r[c]["head_len"] = nb - int(r[c]["head_off"]) + 1; cases.append(("a header past the text", spans, r, c, FORMATS))
    r = rec.copy(); r[c]["head_off"] = -3; cases.append(("a negative header offset", spans, r, c, FORMATS))
    r = rec.copy(); r[d]["head_len"] = -1; cases.append(("a negative header length", spans, r, d, FORMATS))
    r = rec.copy(); r[d]["qual_off"] = nb - 2; cases.append(("a quality line past the text", spans, r, d, FORMATS))
    r = rec.copy(); r[a]["qual_off"] = 1 << 62; cases.append(("a quality offset far outside", spans, r, a, FORMATS))
    r = rec.copy(); r[b]["qual_len"] += 1; cases.append(("qual_len above the read's length", spans, r, b, (tr.TEXT_FASTQ,)))
    r = rec.copy(); r[b]["qual_len"] -= 1; cases.append(("qual_len below the read's length", spans, r, b, (tr.TEXT_FASTQ,)))
    r = rec.copy(); r[c]["qual_off"], r[c]["qual_len"] = -1, 0; cases.append(("no quality line", spans, r, c, (tr.TEXT_FASTQ,)))
    for what, sp, r, i, fmts in cases:
        for fmt in fmts:
            exp = tr.emit_ref(data, start, length, text, r, sp, None, 0, fmt)
            assert i not in exp[1] and len(exp[1]) == len(start) - 1, what
            _assert_text(_device_emit(ctx, data, start, length, text, r, sp, None, 0, fmt), exp, what)
            for kp in (None, np.arange(len(start)) != i):          # the host form names the read, whatever its keep byte
                with pytest.raises(cfrk_amd.CfrkError, match=r"read %d: " % i) as e:
                    ctx.emit_reads(data, start, length, text, r, sp, kp, 0, fmt)
                assert e.value.code == CFRK_ERR_LAYOUT, what
    # under FASTA output a quality length that is not the read's is no fault
    r = rec.copy(); r[b]["qual_len"] -= 1
    exp = tr.emit_ref(data, start, length, text, r, spans, None, 0, tr.TEXT_FASTA)
    assert b in exp[1]
    _assert_text(_device_emit(ctx, data, start, length, text, r, spans, None, 0, tr.TEXT_FASTA), exp, "fasta output ignores qual_len")
    assert ctx.emit_reads(data, start, length, text, r, spans, None, 0, tr.TEXT_FASTA) == exp[0]
    # read ranges outside [0, nN): dropped; the host form checks the layout
    st, ln = start.copy(), length.copy()
    st[a], ln[b] = -3, 0x7FFFFFFF
    exp = tr.emit_ref(data, st, ln, text, rec, None, None, 0, tr.TEXT_FASTA)
    assert len(exp[1]) == len(start) - 2
    _assert_text(_device_emit(ctx, data, st, ln, text, rec, None, None, 0, tr.TEXT_FASTA), exp, "ranges")
    with pytest.raises(cfrk_amd.CfrkError) as e:
        ctx.emit_reads(data, st, ln, text, rec)
    assert e.value.code == CFRK_ERR_LAYOUT


def test_emit_arguments(ctx):
    import cfrk_amd
    L = cfrk_amd.load_library()
    text, rec, data, start, length, spans, keep = _mix()
    raw = np.frombuffer(text, np.uint8)
    out = np.zeros(len(text) + 64, np.uint8)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    nb, ns = C.c_uint64(), C.c_int64()

    def call(fn=L.cfrk_reads_emit_text, **kw):
        a = dict(data=vp(data), start=vp(start), length=vp(length), nN=len(data), nS=len(start), span=vp(spans), keep=None, min_len=0,
                 text=vp(raw), nbytes=raw.size, rec=vp(rec), fmt=1, out=vp(out), cap=out.size, nb=C.byref(nb), ns=C.byref(ns))
        a.update(kw)
        return fn(ctx._h, *[a[k] for k in ("data", "start", "length", "nN", "nS", "span", "keep", "min_len", "text", "nbytes", "rec", "fmt", "out",
                                           "cap", "nb", "ns")])

    assert call() == 0 and nb.value == len(tr.emit_ref(data, start, length, text, rec, spans, None, 0, tr.TEXT_FASTQ)[0])
    for fn in (L.cfrk_reads_emit_text, L.cfrk_reads_emit_text_device):
        for kw in (dict(fmt=2), dict(fmt=-1), dict(rec=None), dict(nN=-1), dict(nS=-1), dict(min_len=-1), dict(nb=None), dict(ns=None),
                   dict(start=None), dict(length=None), dict(data=None), dict(text=None), dict(out=None)):
            assert call(fn, **kw) == CFRK_ERR_ARG, (fn, kw)
        assert call(fn, nS=0, start=None, length=None, rec=None, span=None) == 0 and (nb.value, ns.value) == (0, 0)


def test_round_trip_on_the_device(ctx):
    """FASTQ text -> parse_fastq_device + index_text_device -> count at k = 21 -> spans -> emit as FASTQ: the emitted text,
    parsed again by the host parser, is what cfrk_reads_select makes of the same arguments; names and quality slices are
    the reference's"""
    import cfrk_amd
    k = 21
    rng = np.random.default_rng(79)
    genome = rng.integers(0, 4, 20000).astype(np.int8)
    reads = _noisy_reads(rng, genome, 1200, 80, 200, 0.01) + [rng.integers(0, 4, int(n)).astype(np.int8) for n in rng.integers(30, 200, 50)]
    reads = [np.frombuffer(b"ACGT", np.uint8)[reads[i]].tobytes() for i in rng.permutation(len(reads))]
    text = _fastq_of(reads, [b"read_%d len=%d" % (i, len(s)) for i, s in enumerate(reads)], rng, crlf_every=0)
    rc, _, (data, start, length) = fc.host_parse(text, 0)
    assert rc == 0
    want = _oracle(data, k, True)
    counts, valid = fr.window_counts(data, k, True, want)
    spans = fr.ref_spans(data, start, length, k, 2, COUNT_MAX, fr.SPAN_LONGEST, counts, valid)
    rec = tr.index_ref(text, tr.TEXT_FASTQ)
    etext, eindex = tr.emit_ref(data, start, length, text, rec, spans, None, k, tr.TEXT_FASTQ)
    assert 0 < len(eindex) < len(start) and (spans["length"][eindex] < length[eindex]).any()      # some dropped, some trimmed
    nb, nS = len(text), len(start)
    d_text = _upload(ctx, np.frombuffer(text, np.uint8))
    d_data, d_start, d_length = ctx.alloc(nb // 2 + 16), ctx.alloc(nS * 8), ctx.alloc(nS * 4)
    d_rec, d_span, d_out = ctx.alloc(nS * 24), ctx.alloc(nS * 8), ctx.alloc(nb + 16)
    try:
        assert ctx.parse_fastq_device(d_text, nb, 0, d_data, nb // 2, d_start, d_length, nS) == (len(data), nS)
        assert ctx.index_text_device(d_text, nb, tr.TEXT_FASTQ, d_rec, nS) == nS
        g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, 0)
        g.add_device(d_data, len(data))
        g.read_spans_device(d_data, d_start, d_length, len(data), nS, 2, COUNT_MAX, cfrk_amd.CFRK_SPAN_LONGEST, d_span)
        ob, os_ = ctx.emit_reads_device(d_data, d_start, d_length, len(data), nS, d_span, 0, k, d_text, nb, d_rec, tr.TEXT_FASTQ, d_out, nb)
        ctx.sync()
        got = np.empty(ob, np.uint8)
        ctx.d2h(got, d_out)
        got_rec, got_span = np.empty(nS, REC), np.empty(nS, tr.SPAN_DTYPE)
        ctx.d2h(got_rec, d_rec)
        ctx.d2h(got_span, d_span)
    finally:
        ctx.sync()
        for p in (d_text, d_data, d_start, d_length, d_rec, d_span, d_out):
            ctx.free(p)
    _assert_records(got_rec, rec, "index")
    assert (got_span == spans).all()
    _assert_text((ob, os_, got.tobytes()), (etext, eindex), "round trip")
    rc, _, again = fc.host_parse(got.tobytes(), 0)
    sel = ctx.select_reads(data, start, length, spans, None, k)
    assert rc == 0 and (sel[3] == eindex).all()
    for g_, w_ in zip(again, sel[:3]):
        assert g_.dtype == w_.dtype and len(g_) == len(w_) and (g_ == w_).all()
    lines = got.tobytes().split(b"\n")
    for j, i in enumerate(eindex[:200]):
        off, n = int(spans[i]["offset"]), int(spans[i]["length"])
        q = int(rec[i]["qual_off"]) + off
        assert lines[4 * j] == b"@read_%d len=%d" % (i, length[i]) and lines[4 * j + 3] == text[q:q + n]


def test_cli_filter_names_and_format(tmp_path):
    cli = _cli()
    k = 21
    rng = np.random.default_rng(8812)
    genome = rng.integers(0, 4, 8000).astype(np.int8)
    letters = np.frombuffer(b"ACGT", np.uint8)
    fa = tmp_path / "g.fasta"
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, letters[r].tobytes()) for i, r in enumerate(_noisy_reads(rng, genome, 1200, 60, 220, 0.0))))
    qs = [letters[r].tobytes() for r in _noisy_reads(rng, genome, 300, 30, 260, 0.01)]
    qs += [b"", b"ACGT", qs[0][:k - 1], qs[1][:40] + b"N" + qs[1][40:], qs[2].lower(), letters[genome[:3000]].tobytes()]
    names = [b"q%d extra words" % i for i in range(len(qs))]
    fq_text = _fastq_of(qs, names, rng)
    fa_text = b"".join(b">" + n + b"\n" + s + b"\n" for s, n in zip(qs, names))
    qfq, qfa = tmp_path / "q.fastq", tmp_path / "q.fasta"
    qfq.write_bytes(fq_text)
    qfa.write_bytes(fa_text)
    creads = ic.host_parse(fa.read_bytes(), ic.NATIVE)[1]
    want = _oracle(creads[0], k, True)
    rc, _, (qd, qst, qln) = fc.host_parse(fq_text, 0)
    assert rc == 0
    counts, valid = fr.window_counts(qd, k, True, want)
    spans = fr.ref_spans(qd, qst, qln, k, 2, COUNT_MAX, fr.SPAN_LONGEST, counts, valid)
    rec_q, rec_a = tr.index_ref(fq_text, tr.TEXT_FASTQ), tr.index_ref(fa_text, tr.TEXT_FASTA)
    base = [cli, str(fa), str(tmp_path / "none.cfrk"), str(k), "--global", "--canonical", "--query-only"]

    def run(q, out, *more):
        subprocess.run(base + ["--query", str(q), "--filter-out", str(out)] + list(more), check=True, timeout=300)
        return out.read_bytes()

    as_fastq = tr.emit_ref(qd, qst, qln, fq_text, rec_q, spans, None, k, tr.TEXT_FASTQ)[0]
    assert 0 < as_fastq.count(b"\n") // 4 < len(qs)
    assert run(qfq, tmp_path / "f1.fq", "--filter-format", "fastq") == as_fastq
    named = tr.emit_ref(qd, qst, qln, fq_text, rec_q, spans, None, k, tr.TEXT_FASTA)[0]
    assert run(qfq, tmp_path / "f2.fa", "--filter-names") == named
    assert run(qfq, tmp_path / "f3.fa", "--filter-names", "--filter-format", "fasta") == named
    assert run(qfa, tmp_path / "f4.fa", "--filter-names") == tr.emit_ref(qd, qst, qln, fa_text, rec_a, spans, None, k, tr.TEXT_FASTA)[0] == named
    whole = tr.emit_ref(qd, qst, qln, fq_text, rec_q, None, None, 0, tr.TEXT_FASTQ)[0]
    assert run(qfq, tmp_path / "f5.fq", "--filter-format", "fastq", "--filter-trim", "none", "--filter-min-len", "0") == whole
    # without the options: today's bytes, records named by number
    numbered = fr.fasta_text(*fr.ref_select(qd, qst, qln, spans, None, k))
    assert run(qfq, tmp_path / "f6.fa") == numbered == run(qfa, tmp_path / "f7.fa", "--filter-format", "fasta")
    assert not (tmp_path / "none.cfrk").exists()
