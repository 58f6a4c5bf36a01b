"""CPU-side checks of the abundance histogram and the count-range export: the C ABI declares and exports both
functions, the histo formatter of libcfrk_host.so renders the spectrum, and the CLI refuses bad spectrum / range
options before it parses the input or opens a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    L.cfrk_host_format_histo.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t]
    L.cfrk_host_format_histo.restype = C.c_size_t
    return L


@pytest.fixture(scope="module")
def cli(built):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "cfrk_amd", "cfrk")


def test_abi_declares_and_exports_histogram_and_range_export(built):
    syms = built.abi_symbols()
    L = C.CDLL(built.library_path())
    for s in ("cfrk_global_histogram", "cfrk_global_export_range"):
        assert s in syms
        assert hasattr(L, s)
    assert L.cfrk_abi_version() == 1


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and len(a) else None


def _format(L, hist, tail):
    hist = None if hist is None else np.ascontiguousarray(hist, np.uint64)
    tail = np.ascontiguousarray(tail, np.uint32)
    nb = 0 if hist is None else len(hist)
    n = L.cfrk_host_format_histo(_ptr(hist), nb, _ptr(tail), len(tail), None, 0)
    buf = C.create_string_buffer(n + 1)
    m = L.cfrk_host_format_histo(_ptr(hist), nb, _ptr(tail), len(tail), buf, n)
    assert m == n
    return buf.raw[:n]


def _numpy_histo(hist, tail):
    spec = {}
    for c in range(1, len(hist)):
        if hist[c]:
            spec[c] = spec.get(c, 0) + int(hist[c])
    for c in np.asarray(tail, np.uint64).tolist():
        if c:
            spec[c] = spec.get(c, 0) + 1
    return b"".join(b"%d\t%d\n" % (c, spec[c]) for c in sorted(spec) if spec[c])


def test_histo_formatter_matches_numpy(host):
    rng = np.random.default_rng(5)
    hist = rng.integers(0, 1000, 300).astype(np.uint64)
    hist[rng.random(300) < 0.4] = 0
    hist[0] = 77                                            # (bin 0 is ignored)
    hist[5] = 2 ** 40
    tail = np.concatenate([rng.integers(300, 5000, 50), [0xFFFFFFFE] * 3, [0xFFFFFFFD, 2 ** 31],
                           [7, 7, 299]]).astype(np.uint32)  # (tail counts below nbins land in their bin)
    rng.shuffle(tail)
    assert _format(host, hist, tail) == _numpy_histo(hist, tail)


def test_histo_formatter_empty_and_tail_only(host):
    assert _format(host, np.zeros(16, np.uint64), []) == b""
    assert _format(host, None, []) == b""
    assert _format(host, np.zeros(2, np.uint64), np.array([0xFFFFFFFE, 0xFFFFFFFE, 4294967293], np.uint32)) == \
        b"4294967293\t1\n4294967294\t2\n"
    h = np.zeros(4, np.uint64)
    h[1] = 10
    h[3] = 1
    assert _format(host, h, []) == b"1\t10\n3\t1\n"


@pytest.mark.parametrize("args, msg", [
    (["--histo", "h.txt"], b"need --global"),
    (["--min-count", "2"], b"need --global"),
    (["--max-count", "9"], b"need --global"),
    (["--histo", "h.txt", "--histo-only"], b"need --global"),
    (["--global", "--min-count", "9", "--max-count", "2"], b"above --max-count"),
    (["--global", "--min-count", "two"], b"needs a count"),
    (["--global", "--max-count", "-3"], b"needs a count"),
    (["--global", "--max-count", "4294967296"], b"needs a count"),
    (["--global", "--max-count", "1e3"], b"needs a count"),
    (["--global", "--histo-only"], b"--histo-only needs --histo"),
])
def test_cli_refuses_bad_spectrum_options_before_reading_input(cli, tmp_path, args, msg):
    """refused with status 1 and a message before the input is parsed or a device is opened: the input file does not
    even exist, and no output (or histo) file is created"""
    out = tmp_path / "o.txt"
    p = subprocess.run([cli, str(tmp_path / "missing.fasta"), str(out), "15"] + args, cwd=tmp_path,
                       capture_output=True, timeout=60)
    assert p.returncode == 1
    assert msg in p.stderr
    assert not out.exists() and not (tmp_path / "h.txt").exists()
