"""CPU-side checks of the per-read sparse form: the C ABI declares and exports both calls, the Python mirror has them,
the row formatter of libcfrk_host.so renders CSR rows, the CLI refuses bad --sparse combinations before it reads any
input or opens a device, and the kernels of sparse.hip use no scratch memory."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from .test_kernel_resources import CSRC, HIPCC, ROOT, _functions

SPARSE_CALLS = ("cfrk_per_read_sparse", "cfrk_per_read_sparse_device")


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
    L.cfrk_host_format_sparse_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_char_p, C.c_size_t]
    L.cfrk_host_format_sparse_rows.restype = C.c_size_t
    L.cfrk_host_format_sparse_rows_mt.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_char_p,
                                                  C.c_size_t, C.c_int]
    L.cfrk_host_format_sparse_rows_mt.restype = C.c_size_t
    return L


@pytest.fixture(scope="module")
def cli(built):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "cfrk_amd", "cfrk")


def test_abi_declares_and_exports_the_sparse_calls(built):
    syms = built.abi_symbols()
    L = C.CDLL(built.library_path())
    for s in SPARSE_CALLS:
        assert s in syms
        assert hasattr(L, s)
    assert L.cfrk_abi_version() == 1
    header = open(os.path.join(ROOT, "include", "cfrk_abi.h")).read()
    assert re.search(r"#define CFRK_ABI_VERSION 1\b", header)
    m = re.search(r"#define CFRK_SPARSE_FAST_WINDOWS (\d+)", header)
    assert m and int(m.group(1)) == built.CFRK_SPARSE_FAST_WINDOWS >= 1024
    for name in ("per_read_sparse", "per_read_sparse_device"):
        assert callable(getattr(built.Context, name))
    assert built.load_library().cfrk_per_read_sparse.argtypes is not None


def py_format_rows(row_ptr, keys, counts):
    """the Python rendering of CSR rows: one line per read, "key:count" tokens separated by single spaces"""
    out = []
    for i in range(len(row_ptr) - 1):
        a, b = int(row_ptr[i]), int(row_ptr[i + 1])
        out.append(" ".join(f"{int(k)}:{int(c)}" for k, c in zip(keys[a:b], counts[a:b])) + "\n")
    return "".join(out).encode()


def _format(L, row_ptr, keys, counts, threads=None):
    row_ptr = np.ascontiguousarray(row_ptr, np.int64)
    keys = np.ascontiguousarray(keys, np.uint64)
    counts = np.ascontiguousarray(counts, np.uint32)
    nS = len(row_ptr) - 1
    p = [a.ctypes.data_as(C.c_void_p) if len(a) else None for a in (row_ptr, keys, counts)]
    if threads is None:
        fn = lambda buf, cap: L.cfrk_host_format_sparse_rows(*p, nS, buf, cap)
    else:
        fn = lambda buf, cap: L.cfrk_host_format_sparse_rows_mt(*p, nS, buf, cap, threads)
    n = fn(None, 0)
    buf = C.create_string_buffer(n + 1)
    assert fn(buf, n) == n
    return buf.raw[:n]


def _random_rows(rng, nS, max_row):
    sizes = rng.integers(0, max_row, nS)
    sizes[rng.random(nS) < 0.2] = 0                              # empty rows
    row_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    keys = np.concatenate([np.sort(rng.integers(0, 1 << 62, int(s), dtype=np.uint64)) for s in sizes] + [np.zeros(0, np.uint64)])
    counts = rng.integers(1, 300, len(keys)).astype(np.uint32)
    return row_ptr, keys.astype(np.uint64), counts


@pytest.mark.parametrize("nS, threads", [(50, None), (50, 1), (5000, 7), (3, 16)])
def test_row_formatter_matches_python(host, nS, threads):
    rng = np.random.default_rng(nS)
    row_ptr, keys, counts = _random_rows(rng, nS, 40)
    assert _format(host, row_ptr, keys, counts, threads) == py_format_rows(row_ptr, keys, counts)


def test_row_formatter_edges(host):
    assert _format(host, [0], [], []) == b""                                           # nS = 0
    assert _format(host, [0], [], [], threads=4) == b""
    assert _format(host, [0, 0, 0], [], []) == b"\n\n"                                   # empty rows only
    assert _format(host, [0, 1], [2 ** 64 - 1], [1]) == b"18446744073709551615:1\n"      # k = 32, all T
    assert _format(host, [0, 1], [0], [4294967295]) == b"0:4294967295\n"                 # a single-entry row
    assert _format(host, [0, 0, 2, 2, 3], [5, 9, 2 ** 64 - 1], [1, 2, 119]) == b"\n5:1 9:2\n\n18446744073709551615:119\n"


@pytest.mark.parametrize("args, k, msg", [
    (["--sparse", "--global"], "21", b"--sparse is a per-read mode"),
    (["--sparse", "--binary"], "21", b"--sparse is a per-read mode"),
    (["--sparse", "--histo", "h.txt"], "21", b"--sparse is a per-read mode"),
    (["--sparse", "--histo-only"], "21", b"--sparse is a per-read mode"),
    (["--sparse", "--query", "q.fa", "--query-out", "o.q"], "21", b"--sparse is a per-read mode"),
    (["--sparse", "--query-out", "o.q"], "21", b"--sparse is a per-read mode"),
    (["--sparse", "--query-only"], "21", b"--sparse is a per-read mode"),
    (["--sparse", "--query-db", "db.bin"], "21", b"--sparse is a per-read mode"),
    (["--sparse", "--min-count", "2"], "21", b"--sparse is a per-read mode"),
    (["--sparse", "--max-count", "9"], "21", b"--sparse is a per-read mode"),
    (["--sparse"], "33", b"--sparse needs 1 <= k <= 32"),
    (["--sparse", "--canonical"], "0", b"--sparse needs 1 <= k <= 32"),
])
def test_cli_refuses_bad_sparse_options_before_reading_input(cli, tmp_path, args, k, msg):
    """refused with status 1 and a message before any input is read or a device is opened: the input does not exist
    and no output file is created"""
    out = tmp_path / "o.txt"
    p = subprocess.run([cli, str(tmp_path / "missing.fasta"), str(out), k] + args, cwd=tmp_path,
                       capture_output=True, timeout=60)
    assert p.returncode == 1
    assert msg in p.stderr
    assert not out.exists() and not (tmp_path / "o.q").exists() and not (tmp_path / "h.txt").exists()


def test_sparse_kernels_use_no_scratch(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path / "sparse.s"
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(CSRC, "sparse.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = []
    for name, ops, size in _functions(out.read_text()):
        names.append(name)
        assert ops == 0, f"{name} has {ops} scratch instructions"
        assert not size, f"{name} reserves {size} bytes of scratch per thread"
    for kernel in ("sparse_count_kernel", "sparse_compact_kernel", "sparse_runlength_kernel", "sparse_long_sort_kernel",
                   "sparse_scan_apply_kernel"):
        assert any(kernel in n for n in names), kernel
