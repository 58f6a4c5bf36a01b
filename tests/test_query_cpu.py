"""CPU-side checks of the point queries: the C ABI declares and exports the four query calls, the query formatter of
libcfrk_host.so renders the answers, the CLI refuses bad query options before it reads any input or opens a device,
and the query kernels use no scratch memory."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from .test_kernel_resources import CSRC, HIPCC, ROOT, _functions

NONE = 0xFFFFFFFF
QUERY_CALLS = ("cfrk_global_query", "cfrk_global_query_device", "cfrk_global_query_reads",
               "cfrk_global_query_reads_device")


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
    L.cfrk_host_format_query.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_char_p,
                                         C.c_size_t]
    L.cfrk_host_format_query.restype = C.c_size_t
    return L


@pytest.fixture(scope="module")
def cli(built):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "cfrk_amd", "cfrk")


def test_abi_declares_and_exports_the_query_calls(built):
    syms = built.abi_symbols()
    L = C.CDLL(built.library_path())
    for s in QUERY_CALLS:
        assert s in syms
        assert hasattr(L, s)
    assert L.cfrk_abi_version() == 1
    header = open(os.path.join(ROOT, "include", "cfrk_abi.h")).read()
    assert re.search(r"#define CFRK_QUERY_NONE 0xFFFFFFFF\b", header)
    assert built.CFRK_QUERY_NONE == NONE
    for name in ("query", "query_device", "query_reads", "query_reads_device"):
        assert callable(getattr(built.GlobalCounter, name))


def _format(L, counts, start, length, k):
    counts = np.ascontiguousarray(counts, np.uint32)
    start = np.ascontiguousarray(start, np.int64)
    length = np.ascontiguousarray(length, np.int32)
    p = [a.ctypes.data_as(C.c_void_p) if len(a) else None for a in (counts, start, length)]
    n = L.cfrk_host_format_query(*p, len(start), k, None, 0)
    buf = C.create_string_buffer(n + 1)
    m = L.cfrk_host_format_query(*p, len(start), k, buf, n)
    assert m == n
    return buf.raw[:n]


def _py_format(counts, start, length, k):
    out = []
    for s, L in zip(start, length):
        w = counts[s:s + max(L - k + 1, 0)]
        out.append(" ".join("-" if c == NONE else str(int(c)) for c in w) + "\n")
    return "".join(out).encode()


@pytest.mark.parametrize("k", [1, 5, 31, 64])
def test_query_formatter_matches_python(host, k):
    rng = np.random.default_rng(k)
    lengths = np.concatenate([rng.integers(0, 200, 60), [0, k - 1, k, k + 1]]).astype(np.int32)
    start = np.concatenate([[0], np.cumsum(lengths.astype(np.int64) + 1)[:-1]])
    nN = int(start[-1] + lengths[-1] + 1)
    counts = rng.integers(0, 50, nN).astype(np.uint32)
    counts[rng.random(nN) < 0.2] = NONE
    counts[rng.random(nN) < 0.05] = 0xFFFFFFFE
    assert _format(host, counts, start, lengths, k) == _py_format(counts, start, lengths, k)


def test_query_formatter_edges(host):
    assert _format(host, np.zeros(0, np.uint32), [], [], 3) == b""
    assert _format(host, np.array([NONE] * 4, np.uint32), [0], [3], 3) == b"-\n"
    assert _format(host, np.array([7, 0, NONE, 4294967294, NONE], np.uint32), [0], [4], 1) == b"7 0 - 4294967294\n"
    assert _format(host, np.array([1, 2, NONE, NONE], np.uint32), [0, 3], [2, 0], 2) == b"1\n\n"


@pytest.mark.parametrize("args, msg", [
    (["--query", "q.fa", "--query-out", "o.q"], b"--query needs --global or --query-db"),
    (["--global", "--query-out", "o.q"], b"need --query QFILE"),
    (["--global", "--query-only"], b"need --query QFILE"),
    (["--global", "--query", "q.fa"], b"--query needs --query-out"),
    (["--global", "--query", "q.fa", "--query-out", "o.q", "--batch", "2"], b"not with --batch"),
])
def test_cli_refuses_bad_query_options_before_reading_input(cli, tmp_path, args, msg):
    """refused with status 1 and a message before any input is read or a device is opened: neither the input nor the
    query file exists, and no output file is created"""
    out = tmp_path / "o.txt"
    p = subprocess.run([cli, str(tmp_path / "missing.fasta"), str(out), "15"] + args, cwd=tmp_path,
                       capture_output=True, timeout=60)
    assert p.returncode == 1
    assert msg in p.stderr
    assert not out.exists() and not (tmp_path / "o.q").exists()


@pytest.mark.parametrize("args, msg", [
    (["--query-db", "db.bin"], b"need --query QFILE"),
    (["--query-db", "db.bin", "--query", "q.fa"], b"--query needs --query-out"),
    (["--query-db", "db.bin", "--query", "q.fa", "--query-out", "o.q", "in.fa", "out.txt", "15"],
     b"no positional arguments"),
])
def test_cli_refuses_bad_query_db_options_before_reading_input(cli, tmp_path, args, msg):
    p = subprocess.run([cli] + args, cwd=tmp_path, capture_output=True, timeout=60)
    assert p.returncode == 1
    assert msg in p.stderr
    assert not (tmp_path / "o.q").exists() and not (tmp_path / "out.txt").exists()


def test_query_kernels_use_no_scratch(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path / "query.s"
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(CSRC, "query.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = []
    for name, ops, size in _functions(out.read_text()):
        names.append(name)
        assert ops == 0, f"{name} has {ops} scratch instructions"
        assert not size, f"{name} reserves {size} bytes of scratch per thread"
    assert any("query_reads1_kernel" in n for n in names) and any("query_keys_kernel" in n for n in names)
