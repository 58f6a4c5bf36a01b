"""CPU-side checks of the read filter: the C ABI declares and exports the spans and select calls, cfrk_read_span is 8
bytes with the documented offsets (header, ctypes and READ_SPAN_DTYPE), the Python methods exist, the FASTA formatter
of libcfrk_host.so renders selected reads, the CLI refuses bad --filter-* options before it reads any input or opens a
device, the kernels of read_filter.hip use no scratch memory, and the numpy span rule of tests/filter_ref.py gives the
hand-worked answers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from . import filter_ref as fr
from .test_kernel_resources import CSRC, HIPCC, ROOT, _functions

FILTER_CALLS = ("cfrk_global_read_spans", "cfrk_global_read_spans_device", "cfrk_reads_select", "cfrk_reads_select_device")


class _Span(C.Structure):
    """cfrk_read_span as include/cfrk_abi.h declares it"""
    _fields_ = [("offset", C.c_int32), ("length", C.c_int32)]


@pytest.fixture(scope="module")
def built():
    import cfrk_amd
    if not os.path.exists(cfrk_amd.library_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "csrc"), "-j4"],
                              stdout=subprocess.DEVNULL)
    return cfrk_amd


@pytest.fixture(scope="module")
def host():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host"), "../libcfrk_host.so"],
                          stdout=subprocess.DEVNULL)
    L = C.CDLL(os.path.join(ROOT, "cfrk_amd", "libcfrk_host.so"))
    L.cfrk_host_format_fasta.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_char_p, C.c_size_t]
    L.cfrk_host_format_fasta.restype = C.c_size_t
    return L


@pytest.fixture(scope="module")
def cli(built):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "cfrk_amd", "cfrk")


def test_abi_declares_and_exports_the_filter_calls(built, host):
    syms = built.abi_symbols()
    L = C.CDLL(built.library_path())
    for s in FILTER_CALLS:
        assert s in syms
        assert hasattr(L, s)
    assert hasattr(host, "cfrk_host_format_fasta")
    assert "cfrk_host_format_fasta" in open(os.path.join(ROOT, "cfrk_amd", "host", "cfrk_host.h")).read()
    header = open(os.path.join(ROOT, "include", "cfrk_abi.h")).read()
    for name in ("CFRK_SPAN_PREFIX", "CFRK_SPAN_LONGEST", "CFRK_SPANS_FAST_WINDOWS", "CFRK_SELECT_TILE_BYTES",
                 "CFRK_SELECT_SCAN_TILES"):
        m = re.search(r"#define %s (\d+)\b" % name, header)
        assert m and int(m.group(1)) == getattr(built, name), name
    assert (built.CFRK_SPAN_PREFIX, built.CFRK_SPAN_LONGEST, built.CFRK_SPANS_FAST_WINDOWS) == (0, 1, 2048)
    for name in ("read_spans", "read_spans_device"):
        assert callable(getattr(built.GlobalCounter, name))
    for name in ("select_reads", "select_reads_device"):
        assert callable(getattr(built.Context, name))


def test_span_is_8_bytes_with_the_documented_offsets(built):
    header = open(os.path.join(ROOT, "include", "cfrk_abi.h")).read()
    body = re.search(r"typedef struct cfrk_read_span \{(.*?)\} cfrk_read_span;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s+(\w+);", body) == [("int32_t", "offset"), ("int32_t", "length")]
    assert C.sizeof(_Span) == 8 and _Span.offset.offset == 0 and _Span.length.offset == 4
    dt = built.READ_SPAN_DTYPE
    assert dt.itemsize == 8 and dt.names == ("offset", "length")
    assert dt.fields["offset"][1] == 0 and dt.fields["length"][1] == 4
    assert [dt.fields[n][0].str for n in dt.names] == ["<i4", "<i4"]
    assert dt == fr.SPAN_DTYPE


def _format(L, data, start, length, index):
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and len(a) else None
    n = L.cfrk_host_format_fasta(vp(data), vp(start), vp(length), vp(index), len(start), None, 0)
    buf = C.create_string_buffer(n + 1)
    assert L.cfrk_host_format_fasta(vp(data), vp(start), vp(length), vp(index), len(start), buf, n) == n
    assert buf.raw[n:] == b"\0"                                  # nothing behind the size it asked for
    return buf.raw[:n]


def test_fasta_formatter(host):
    # ACGT, an empty read, N for code -1 and for code 7, indices above 2^32
    data = np.array([0, 1, 2, 3, -1,   -1,   0, -1, 7, 3, -1,   2, -1], np.int8)
    start = np.array([0, 5, 6, 11], np.int64)
    length = np.array([4, 0, 4, 1], np.int32)
    index = np.array([0, 7, (1 << 32) + 5, (1 << 40) + 123456789], np.int64)
    want = b">0\nACGT\n>7\n\n>4294967301\nANNT\n>1099635084565\nG\n"
    assert _format(host, data, start, length, index) == want
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert host.cfrk_host_format_fasta(vp(data), vp(start), vp(length), vp(index), 4, None, 0) == len(want)   # size only
    assert _format(host, data[:0], start[:0], length[:0], index[:0]) == b""
    assert _format(host, data, start, length, None) == b">0\nACGT\n>1\n\n>2\nANNT\n>3\nG\n"     # no index: 0, 1, ..
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 200, 300).astype(np.int32)
    st = np.concatenate([[0], np.cumsum(lens.astype(np.int64) + 1)[:-1]]).astype(np.int64)
    d = rng.integers(-3, 9, int(lens.sum()) + len(lens)).astype(np.int8)
    idx = rng.integers(0, 1 << 45, 300).astype(np.int64)
    assert _format(host, d, st, lens, idx) == fr.fasta_text(d, st, lens, idx)


Q = ["--global", "--query", "q.fa"]


@pytest.mark.parametrize("args, msg", [
    (["--global", "--filter-out", "f.fa"], b"need --query QFILE"),
    (["--global", "--filter-min-count", "3"], b"need --query QFILE"),
    (["--filter-out", "f.fa", "--query", "q.fa"], b"--query needs --global or --query-db"),
    (Q + ["--query-out", "o.q", "--filter-min-count", "3"], b"need --filter-out FFILE"),
    (Q + ["--query-out", "o.q", "--filter-trim", "prefix"], b"need --filter-out FFILE"),
    (Q + ["--query-out", "o.q", "--filter-min-len", "30"], b"need --filter-out FFILE"),
    (Q + ["--query-out", "o.q", "--filter-max-median", "30"], b"need --filter-out FFILE"),
    (Q + ["--filter-out", "f.fa", "--filter-min-count", "two"], b"--filter-min-count needs a count"),
    (Q + ["--filter-out", "f.fa", "--filter-min-count", "-1"], b"--filter-min-count needs a count"),
    (Q + ["--filter-out", "f.fa", "--filter-max-count", "4294967296"], b"--filter-max-count needs a count"),
    (Q + ["--filter-out", "f.fa", "--filter-min-median", "x"], b"--filter-min-median needs a count"),
    (Q + ["--filter-out", "f.fa", "--filter-max-median", "1.5"], b"--filter-max-median needs a count"),
    (Q + ["--filter-out", "f.fa", "--filter-trim", "shortest"], b"--filter-trim takes longest, prefix or none"),
    (Q + ["--filter-out", "f.fa", "--filter-min-len", "-1"], b"--filter-min-len needs a length"),
    (Q + ["--filter-out", "f.fa", "--filter-min-len", "2147483648"], b"--filter-min-len needs a length"),
    (Q + ["--filter-out", "f.fa", "--filter-min-len", "ten"], b"--filter-min-len needs a length"),
    (Q + ["--filter-out", "f.fa", "--filter-trim"], b"--filter-trim needs a value"),
    (Q + ["--filter-out", "f.fa", "--filter-length", "3"], b"unknown option --filter-length"),
    (Q + ["--filter-out", "f.fa", "--gpus", "2"], b"not with --gpus"),
    (Q + ["--filter-out", "f.fa", "--batch", "2"], b"not with --batch"),
    (["--sparse", "--filter-out", "f.fa"], b"--sparse is a per-read mode"),
    (["--sparse", "--filter-min-count", "2"], b"--sparse is a per-read mode"),
])
def test_cli_refuses_bad_filter_options_before_reading_input(cli, tmp_path, args, msg):
    """refused with status 1 and a message before any input is read or a device is opened: neither the input nor the
    query file exists, and no output file is created"""
    out = tmp_path / "o.txt"
    p = subprocess.run([cli, str(tmp_path / "missing.fasta"), str(out), "15"] + args, cwd=tmp_path,
                       capture_output=True, timeout=60)
    assert p.returncode == 1
    assert msg in p.stderr
    assert not out.exists() and not (tmp_path / "o.q").exists() and not (tmp_path / "f.fa").exists()


def test_cli_refuses_filter_options_with_query_db_before_reading_input(cli, tmp_path):
    for args, msg in ((["--query-db", "db.bin", "--filter-out", "f.fa"], b"need --query QFILE"),
                      (["--query-db", "db.bin", "--query", "q.fa", "--filter-trim", "none", "--query-out", "o.q"],
                       b"need --filter-out FFILE"),
                      (["--query-db", "db.bin", "--query", "q.fa", "--filter-out", "f.fa", "--filter-trim", "all"],
                       b"--filter-trim takes longest, prefix or none")):
        p = subprocess.run([cli] + args, cwd=tmp_path, capture_output=True, timeout=60)
        assert p.returncode == 1
        assert msg in p.stderr
        assert not (tmp_path / "o.q").exists() and not (tmp_path / "f.fa").exists()


def test_read_filter_kernels_use_no_scratch(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path / "read_filter.s"
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(CSRC, "read_filter.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = []
    for name, ops, size in _functions(out.read_text()):
        names.append(name)
        assert ops == 0, f"{name} has {ops} scratch instructions"
        assert not size, f"{name} reserves {size} bytes of scratch per thread"
    # three index modes x canonical for each of the three span kernels, and the four passes of the select
    assert sum("read_spans_kernelILi16E" in n for n in names) == 6
    assert sum("read_spans_kernelILi64E" in n for n in names) == 6
    assert sum("read_spans_long_kernel" in n for n in names) == 6
    for kern in ("sel_reduce_kernel", "sel_scan_kernel", "sel_index_kernel", "sel_copy_kernel"):
        assert sum(kern in n for n in names) == 1, kern


@pytest.mark.parametrize("solid, k, longest, prefix", [
    ("", 5, (0, 0), (0, 0)),                       # a read shorter than k: no window
    ("0", 5, (0, 0), (0, 0)),                      # a single window, not solid
    ("1", 5, (0, 5), (0, 5)),                      # a single window, solid: exactly k bases
    ("0000", 3, (0, 0), (0, 0)),                   # none solid
    ("1111", 3, (0, 6), (0, 6)),                   # all solid: the whole read, 4 + 3 - 1 bases
    ("1100", 4, (0, 5), (0, 5)),                   # a run touching the beginning
    ("0011", 4, (2, 5), (0, 0)),                   # a run touching the end; window 0 is not solid
    ("0110", 7, (1, 8), (0, 0)),                   # an interior run
    ("1011", 2, (2, 3), (0, 2)),                   # a solid window 0 followed by a non-solid window 1
    ("110110", 6, (0, 7), (0, 7)),                 # two runs of equal length: the earlier one
    ("0110110", 1, (1, 2), (0, 0)),                # the same away from the beginning, k = 1
    ("10110111", 3, (5, 5), (0, 3)),               # the longest run is the last
    ("1110110", 64, (0, 66), (0, 66)),             # the longest run is the first, k = 64
    ("0100010", 4, (1, 4), (0, 0)),                # single-window runs tie: the first
])
def test_span_rule_on_hand_worked_strings(solid, k, longest, prefix):
    s = np.array([c == "1" for c in solid], bool)
    assert fr.span_rule(s, k, fr.SPAN_LONGEST) == longest
    assert fr.span_rule(s, k, fr.SPAN_PREFIX) == prefix
    for off, n in (longest, prefix):                # a span holds at least k bases when it is not empty, and stays inside
        assert n == 0 or (n >= k and off + n <= len(s) + k - 1)


def test_ref_select_is_plain_slicing():
    data = np.array([0, 1, 2, 3, -1, 3, 3, -1, -1, 1, 7, 1, -1], np.int8)
    start, length = np.array([0, 5, 8, 9], np.int64), np.array([4, 2, 0, 3], np.int32)
    spans = np.array([(1, 2), (0, 2), (0, 0), (1, 2)], fr.SPAN_DTYPE)
    d, s, l, i = fr.ref_select(data, start, length, spans, None, 0)
    assert d.tolist() == [1, 2, -1, 3, 3, -1, -1, 7, 1, -1] and s.tolist() == [0, 3, 6, 7]
    assert l.tolist() == [2, 2, 0, 2] and i.tolist() == [0, 1, 2, 3]
    d, s, l, i = fr.ref_select(data, start, length, spans, np.array([1, 0, 1, 1]), 1)
    assert d.tolist() == [1, 2, -1, 7, 1, -1] and s.tolist() == [0, 3] and l.tolist() == [2, 2] and i.tolist() == [0, 3]
    d, s, l, i = fr.ref_select(data, start, length, None, None, 3)
    assert d.tolist() == [0, 1, 2, 3, -1, 1, 7, 1, -1] and i.tolist() == [0, 3]
    bad = np.array([(-1, 2), (1, 2), (0, 0), (0, 3)], fr.SPAN_DTYPE)     # outside their reads: dropped
    assert fr.ref_select(data, start, length, bad, None, 0)[3].tolist() == [2, 3]
