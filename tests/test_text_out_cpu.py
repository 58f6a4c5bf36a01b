"""CPU-side checks of the text index and the text emitter: the C ABI declares and exports the four calls,
cfrk_text_record is 24 bytes in the header's field order (header, ctypes and TEXT_RECORD_DTYPE), the references of
tests/text_out_ref.py are held to what the project already has -- the host parsers' record numbering and lengths, a round
trip through them, cfrk_host_format_fasta -- and the CLI refuses bad --filter-names / --filter-format uses before it
opens a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from . import fastq_cases as fc
from . import ingest_cases as ic
from . import text_out_ref as tr

ROOT = ic.ROOT
TEXT_CALLS = ("cfrk_text_index", "cfrk_text_index_device", "cfrk_reads_emit_text", "cfrk_reads_emit_text_device")


class _Record(C.Structure):
    """cfrk_text_record as include/cfrk_abi.h declares it"""
    _fields_ = [("head_off", C.c_int64), ("qual_off", C.c_int64), ("head_len", C.c_int32), ("qual_len", C.c_int32)]


@pytest.fixture(scope="module")
def built():
    import cfrk_amd
    if not os.path.exists(cfrk_amd.library_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return cfrk_amd


@pytest.fixture(scope="module")
def host():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host"), "../libcfrk_host.so"], stdout=subprocess.DEVNULL)
    L = C.CDLL(os.path.join(ROOT, "cfrk_amd", "libcfrk_host.so"))
    L.cfrk_host_format_fasta.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_char_p, C.c_size_t]
    L.cfrk_host_format_fasta.restype = C.c_size_t
    return L


@pytest.fixture(scope="module")
def cli(built):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "cfrk_amd", "cfrk")


def test_abi_declares_and_exports_the_text_calls(built):
    syms = built.abi_symbols()
    L = C.CDLL(built.library_path())
    for s in TEXT_CALLS:
        assert s in syms
        assert hasattr(L, s)
    header = open(os.path.join(ROOT, "include", "cfrk_abi.h")).read()
    for name in ("CFRK_TEXT_FASTA", "CFRK_TEXT_FASTQ", "CFRK_TEXT_TILE_BYTES", "CFRK_TEXT_SCAN_TILES", "CFRK_EMIT_TILE_BYTES"):
        m = re.search(r"#define %s (\d+)\b" % name, header)
        assert m and int(m.group(1)) == getattr(built, name), name
    assert (built.CFRK_TEXT_FASTA, built.CFRK_TEXT_FASTQ, built.CFRK_EMIT_TILE_BYTES) == (0, 1, 16384)
    assert (tr.TEXT_FASTA, tr.TEXT_FASTQ) == (built.CFRK_TEXT_FASTA, built.CFRK_TEXT_FASTQ)
    for name in ("index_text", "index_text_device", "emit_reads", "emit_reads_device"):
        assert callable(getattr(built.Context, name))


def test_record_is_24_bytes_in_the_headers_field_order(built):
    header = open(os.path.join(ROOT, "include", "cfrk_abi.h")).read()
    body = re.search(r"typedef struct cfrk_text_record \{(.*?)\} cfrk_text_record;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+)\s+(\w+);", body)
    assert fields == [("int64_t", "head_off"), ("int64_t", "qual_off"), ("int32_t", "head_len"), ("int32_t", "qual_len")]
    assert C.sizeof(_Record) == 24
    dt = built.TEXT_RECORD_DTYPE
    assert dt.itemsize == 24 and dt.names == tuple(n for _, n in fields)
    assert [dt.fields[n][1] for n in dt.names] == [getattr(_Record, n).offset for n in dt.names] == [0, 8, 16, 20]
    assert [dt.fields[n][0].str for n in dt.names] == ["<i8", "<i8", "<i4", "<i4"]
    assert dt == tr.RECORD_DTYPE


def test_references_on_hand_worked_texts():
    fq = b"@a b\r\nACGT\r\n+x\r\nI5#!\r\n@\n\n+\n\n@c\nAC\n+\n5I"
    rec = tr.index_ref(fq, tr.TEXT_FASTQ)
    assert rec.tolist() == [(0, 16, 4, 4), (22, 27, 1, 0), (28, 36, 2, 2)]
    assert tr.index_ref(fq + b"\n@d\nA\n+", tr.TEXT_FASTQ).tolist() == rec.tolist()        # three more lines: no fourth record
    assert tr.index_ref(b"\r", tr.TEXT_FASTQ).tolist() == [] and tr.lines_ref(b"\r") == [(0, 0)]
    assert tr.lines_ref(b"a\n\nb\r\r\n\r") == [(0, 1), (2, 0), (3, 2), (7, 0)] and tr.lines_ref(b"") == [] and tr.lines_ref(b"\n") == [(0, 0)]
    fa = b"AC\n>one\r\nAC\nGT\n>\n>two words"
    assert tr.index_ref(fa, tr.TEXT_FASTA).tolist() == [(3, -1, 4, 0), (15, -1, 1, 0), (17, -1, 10, 0)]
    data = np.array([0, 1, 2, 3, -1, -1, 0, 7, -1], np.int8)
    start, length = np.array([0, 5, 6], np.int64), np.array([4, 0, 2], np.int32)
    text, index = tr.emit_ref(data, start, length, fq, rec, out_format=tr.TEXT_FASTQ)
    assert text == b"@a b\nACGT\n+\nI5#!\n@\n\n+\n\n@c\nAN\n+\n5I\n" and index == [0, 1, 2]
    spans = np.array([(1, 2), (0, 0), (1, 1)], tr.SPAN_DTYPE)
    text, index = tr.emit_ref(data, start, length, fq, rec, spans, [1, 1, 1], 1, tr.TEXT_FASTQ)
    assert text == b"@a b\nCG\n+\n5#\n@c\nN\n+\nI\n" and index == [0, 2]
    assert tr.emit_ref(data, start, length, fq, rec, spans, [0, 1, 1], 0, tr.TEXT_FASTA) == (b">\n\n>c\nN\n", [1, 2])
    farec = tr.index_ref(fa, tr.TEXT_FASTA)
    assert tr.emit_ref(data, start, length, fa, farec)[0] == b">one\nACGT\n>\n\n>two words\nAN\n"
    assert tr.emit_ref(data, start, length, fa, farec, out_format=tr.TEXT_FASTQ) == (b"", [])      # no quality lines
    bad = rec.copy()
    bad[0]["head_len"] = len(fq) + 1         # runs past the text
    bad[2]["qual_len"] = 1                   # inside the text, but not the read's length
    assert tr.emit_ref(data, start, length, fq, bad, out_format=tr.TEXT_FASTQ)[1] == [1]
    assert tr.emit_ref(data, start, length, fq, bad, out_format=tr.TEXT_FASTA)[1] == [1, 2]


def _fastq_texts():
    return fc.small_cases()


def _fasta_texts():
    out = [(c[0], c[1]) for c in ic.grammar_cases() + ic.seam_cases()] + [(c[0], c[1]) for c in ic.cr_run_cases()]
    return out + [(f"random text {i}", t) for i, t in enumerate(ic.random_texts())]


def test_index_ref_has_the_fastq_parsers_numbering_and_the_round_trip_holds():
    accepted = lost_cr = 0
    for name, raw in _fastq_texts():
        rc, _, parsed = fc.host_parse(raw, 0)
        if rc:
            continue
        accepted += 1
        data, start, length = parsed
        rec = tr.index_ref(raw, tr.TEXT_FASTQ)
        assert len(rec) == len(start), name
        assert (rec["qual_len"] == length).all(), name
        text, index = tr.emit_ref(data, start, length, raw, rec, out_format=tr.TEXT_FASTQ)
        assert index == list(range(len(start))), name
        rc2, _, again = fc.host_parse(text, 0)
        # qualities are copied verbatim: a quality line that still ends in '\r' behind the one the grammar drops loses
        # that byte to the next parse, which then refuses the record -- the only texts that do not come back
        if any(raw[int(r["qual_off"]) + int(r["qual_len"]) - 1:][:1] == b"\r" for r in rec if r["qual_len"] > 0):
            lost_cr += 1
            assert rc2 == fc.LENGTHS, name
            continue
        assert rc2 == 0, name
        for got, want in zip(again, parsed):
            assert got.dtype == want.dtype and len(got) == len(want) and (got == want).all(), name
    assert accepted > 120 and lost_cr * 20 < accepted


def test_index_ref_has_the_fasta_parsers_numbering_and_the_round_trip_holds():
    accepted = 0
    for name, raw in _fasta_texts():
        rec = tr.index_ref(raw, tr.TEXT_FASTA)
        rc_c, compat = ic.host_parse(raw, ic.COMPAT)
        if not rc_c:
            assert len(rec) == len(compat[1]), name
        rc, parsed = ic.host_parse(raw, ic.NATIVE)
        if rc:
            continue
        accepted += 1
        data, start, length = parsed
        assert len(rec) == len(start), name
        assert (rec["qual_off"] == -1).all() and (rec["qual_len"] == 0).all()
        text, index = tr.emit_ref(data, start, length, raw, rec)
        assert index == list(range(len(start))), name
        rc2, again = ic.host_parse(text, ic.NATIVE)
        assert rc2 == 0, name
        for got, want in zip(again, parsed):
            assert got.dtype == want.dtype and len(got) == len(want) and (got == want).all(), name
    assert accepted > 150


def test_emit_ref_equals_the_host_fasta_formatter_on_numbered_headers(host):
    rng = np.random.default_rng(18)
    lens = [0, 1, 150] + [int(x) for x in rng.integers(0, 300, 200)]
    seqs = [np.frombuffer(b"ACGTNacgtn-", np.uint8)[rng.integers(0, 11, n)].tobytes() for n in lens]
    raw = b"".join(b">%d\n%s\n" % (i, s) for i, s in enumerate(seqs))
    rc, (data, start, length) = ic.host_parse(raw, ic.NATIVE)
    assert rc == 0 and length.tolist() == lens
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    n = host.cfrk_host_format_fasta(vp(data), vp(start), vp(length), None, len(start), None, 0)
    buf = C.create_string_buffer(n + 1)
    assert host.cfrk_host_format_fasta(vp(data), vp(start), vp(length), None, len(start), buf, n) == n
    text, _ = tr.emit_ref(data, start, length, raw, tr.index_ref(raw, tr.TEXT_FASTA))
    assert text == buf.raw[:n] and text.count(b"N") > 100


Q = ["--global", "--query"]


@pytest.mark.parametrize("qtext, args, msg", [
    (None, ["--global", "--filter-names"], b"need --query QFILE"),
    (None, ["--global", "--filter-format", "fastq"], b"need --query QFILE"),
    (b">a\nACGT\n", Q + ["Q", "--query-out", "o.q", "--filter-names"], b"need --filter-out FFILE"),
    (b"@a\nACGT\n+\nIIII\n", Q + ["Q", "--query-out", "o.q", "--filter-format", "fastq"], b"need --filter-out FFILE"),
    (b"@a\nACGT\n+\nIIII\n", Q + ["Q", "--query-out", "o.q", "--filter-format", "fasta"], b"need --filter-out FFILE"),
    (b"@a\nACGT\n+\nIIII\n", Q + ["Q", "--filter-out", "f.fa", "--filter-format", "fastx"], b"--filter-format takes fasta or fastq"),
    (b"@a\nACGT\n+\nIIII\n", Q + ["Q", "--filter-out", "f.fa", "--filter-format", "FASTQ"], b"--filter-format takes fasta or fastq"),
    (b"@a\nACGT\n+\nIIII\n", Q + ["Q", "--filter-out", "f.fa", "--filter-format"], b"--filter-format needs a value"),
    (b">a\nACGT\n", Q + ["Q", "--filter-out", "f.fa", "--filter-format", "fastq"], b"--filter-format fastq needs a FASTQ --query file"),
    (b"@a\nACGT\n+\nIIII\n", Q + ["Q", "--format", "fasta", "--filter-out", "f.fa", "--filter-format", "fastq"],
     b"--filter-format fastq needs a FASTQ --query file"),
    (b">a\nACGT\n", ["--sparse", "--filter-names"], b"--sparse is a per-read mode"),
])
def test_cli_refuses_before_a_device_is_opened(cli, tmp_path, qtext, args, msg):
    """refused with status 1 and a message before the input is read or a device is opened: the input does not exist, and
    no output file is created"""
    q = tmp_path / "q.txt"
    if qtext is not None:
        q.write_bytes(qtext)
    args = [str(q) if a == "Q" else a for a in args]
    out = tmp_path / "o.txt"
    p = subprocess.run([cli, str(tmp_path / "missing.fasta"), str(out), "15"] + args, cwd=tmp_path, capture_output=True, timeout=60)
    assert p.returncode == 1
    assert msg in p.stderr
    assert not out.exists() and not (tmp_path / "o.q").exists() and not (tmp_path / "f.fa").exists()
