"""CPU-side checks of the per-read abundance statistics: the C ABI declares and exports the two calls, the row is 32
bytes with the documented offsets (ctypes and READ_STATS_DTYPE), the Python methods exist, the formatter of
libcfrk_host.so renders rows, the CLI refuses bad --query-stats / --stats-below options before it reads any input or
opens a device, and the kernels of read_stats.hip use no scratch memory."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from .test_kernel_resources import CSRC, HIPCC, ROOT, _functions

STATS_CALLS = ("cfrk_global_read_stats", "cfrk_global_read_stats_device")
FIELDS = ("windows", "present", "below", "min", "median", "max", "sum")


class _Row(C.Structure):
    """cfrk_read_stats as include/cfrk_abi.h declares it"""
    _fields_ = [(n, C.c_uint32) for n in FIELDS[:6]] + [("sum", C.c_uint64)]


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
    L.cfrk_host_format_read_stats.argtypes = [C.c_void_p, C.c_int64, C.c_char_p, C.c_size_t]
    L.cfrk_host_format_read_stats.restype = C.c_size_t
    return L


@pytest.fixture(scope="module")
def cli(built):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "cfrk_amd", "cfrk")


def test_abi_declares_and_exports_the_read_stats_calls(built):
    syms = built.abi_symbols()
    L = C.CDLL(built.library_path())
    for s in STATS_CALLS:
        assert s in syms
        assert hasattr(L, s)
    assert L.cfrk_abi_version() == 1
    header = open(os.path.join(ROOT, "include", "cfrk_abi.h")).read()
    m = re.search(r"#define CFRK_STATS_FAST_WINDOWS (\d+)\b", header)
    assert m and int(m.group(1)) == built.CFRK_STATS_FAST_WINDOWS
    # the struct in the header: seven fields in this order, six uint32 and one uint64
    body = re.search(r"typedef struct cfrk_read_stats \{(.*?)\} cfrk_read_stats;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = [(t, [n.strip() for n in names.split(",")]) for t, names in re.findall(r"(uint32_t|uint64_t)\s+([^;]+);", body)]
    assert [n for _, ns in decl for n in ns] == list(FIELDS)
    assert [t for t, ns in decl for _ in ns] == ["uint32_t"] * 6 + ["uint64_t"]
    for name in ("read_stats", "read_stats_device"):
        assert callable(getattr(built.GlobalCounter, name))


def test_row_is_32_bytes_with_the_documented_offsets(built):
    want = dict(zip(FIELDS, (0, 4, 8, 12, 16, 20, 24)))
    assert C.sizeof(_Row) == 32
    assert {n: getattr(_Row, n).offset for n in FIELDS} == want
    dt = built.READ_STATS_DTYPE
    assert dt.itemsize == 32 and dt.names == FIELDS
    assert {n: dt.fields[n][1] for n in FIELDS} == want
    assert [dt.fields[n][0].str for n in FIELDS] == ["<u4"] * 6 + ["<u8"]


def _format(L, rows):
    p = rows.ctypes.data_as(C.c_void_p) if len(rows) else None
    n = L.cfrk_host_format_read_stats(p, len(rows), None, 0)
    buf = C.create_string_buffer(n + 1)
    assert L.cfrk_host_format_read_stats(p, len(rows), buf, n) == n
    return buf.raw[:n]


def test_read_stats_formatter(built, host):
    rows = np.zeros(4, built.READ_STATS_DTYPE)
    rows[0] = (120, 118, 3, 0, 17, 4294967294, 2100)
    # rows[1] stays all-zero: a read without a valid window
    rows[2] = (3, 3, 0, 4294967294, 4294967294, 4294967294, 3 * 4294967294)       # a CFRK_COUNT_MAX median, sum > 2^32
    rows[3] = (4294967295, 1, 4294967295, 1, 2, 3, 18446744073709551615)
    want = (b"120\t118\t3\t0\t17\t4294967294\t2100\n"
            b"0\t0\t0\t0\t0\t0\t0\n"
            b"3\t3\t0\t4294967294\t4294967294\t4294967294\t12884901882\n"
            b"4294967295\t1\t4294967295\t1\t2\t3\t18446744073709551615\n")
    assert _format(host, rows) == want
    assert host.cfrk_host_format_read_stats(rows.ctypes.data_as(C.c_void_p), 4, None, 0) == len(want)   # size only
    assert _format(host, rows[:0]) == b""
    rng = np.random.default_rng(9)
    big = np.zeros(500, built.READ_STATS_DTYPE)
    for n in FIELDS[:6]:
        big[n] = rng.integers(0, 1 << 32, 500, dtype=np.uint64)
    big["sum"] = rng.integers(0, 1 << 63, 500, dtype=np.uint64)
    text = "".join("\t".join(str(int(r[n])) for n in FIELDS) + "\n" for r in big).encode()
    assert _format(host, big) == text


@pytest.mark.parametrize("args, msg", [
    (["--global", "--query-stats", "s.txt"], b"need --query QFILE"),
    (["--global", "--stats-below", "2"], b"need --query QFILE"),
    (["--global", "--query", "q.fa", "--query-out", "o.q", "--stats-below", "2"], b"--stats-below needs --query-stats"),
    (["--global", "--query", "q.fa", "--query-stats", "s.txt", "--stats-below", "two"], b"--stats-below needs a count"),
    (["--global", "--query", "q.fa", "--query-stats", "s.txt", "--stats-below", "-1"], b"--stats-below needs a count"),
    (["--global", "--query", "q.fa", "--query-stats", "s.txt", "--stats-below", "4294967296"],
     b"--stats-below needs a count"),
    (["--global", "--query", "q.fa", "--query-stats", "s.txt", "--batch", "2"], b"not with --batch"),
    (["--global", "--query", "q.fa", "--query-out", "o.q", "--query-stats", "s.txt", "--stats-below", "2", "--batch", "2"],
     b"not with --batch"),
    (["--sparse", "--query-stats", "s.txt"], b"--sparse is a per-read mode"),
    (["--sparse", "--stats-below", "2"], b"--sparse is a per-read mode"),
    (["--global", "--query", "q.fa"], b"--query needs --query-out"),
    (["--global", "--query", "q.fa", "--query-stats", "s.txt", "--gpus", "2"], b"not with --gpus"),
])
def test_cli_refuses_bad_stats_options_before_reading_input(cli, tmp_path, args, msg):
    """refused with status 1 and a message before any input is read or a device is opened: neither the input nor the
    query file exists, and no output file is created"""
    out = tmp_path / "o.txt"
    p = subprocess.run([cli, str(tmp_path / "missing.fasta"), str(out), "15"] + args, cwd=tmp_path,
                       capture_output=True, timeout=60)
    assert p.returncode == 1
    assert msg in p.stderr
    assert not out.exists() and not (tmp_path / "o.q").exists() and not (tmp_path / "s.txt").exists()


def test_cli_refuses_stats_options_with_query_db_before_reading_input(cli, tmp_path):
    for args, msg in ((["--query-db", "db.bin", "--query-stats", "s.txt"], b"need --query QFILE"),
                      (["--query-db", "db.bin", "--query", "q.fa", "--stats-below", "2", "--query-out", "o.q"],
                       b"--stats-below needs --query-stats")):
        p = subprocess.run([cli] + args, cwd=tmp_path, capture_output=True, timeout=60)
        assert p.returncode == 1
        assert msg in p.stderr
        assert not (tmp_path / "o.q").exists() and not (tmp_path / "s.txt").exists()


def test_read_stats_kernels_use_no_scratch(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path / "read_stats.s"
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(CSRC, "read_stats.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = []
    for name, ops, size in _functions(out.read_text()):
        names.append(name)
        assert ops == 0, f"{name} has {ops} scratch instructions"
        assert not size, f"{name} reserves {size} bytes of scratch per thread"
    # three index modes x canonical for each of the three kernels
    assert sum("read_stats_kernelILi16E" in n for n in names) == 6
    assert sum("read_stats_kernelILi64E" in n for n in names) == 6
    assert sum("read_stats_long_kernel" in n for n in names) == 6
