"""FASTA texts for the device parser's tests (test_gpu_ingest.py, test_ingest_cpu.py) and the host parser they are
held against.  Every text is generated here on the CPU; `expect` is what the host parser must say about it per mode:
0, or its error code (-2: a sequence line before the first header, -3: a compat record without a sequence line)."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE, COMPAT = 0, 1


def _header_int(name):
    text = open(os.path.join(ROOT, "include", "cfrk_abi.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


T = _header_int("CFRK_FASTA_TILE_BYTES")
SCAN_TILES = _header_int("CFRK_FASTA_SCAN_TILES")
MAX_CR = _header_int("CFRK_FASTA_MAX_CR_RUN")


class Batch(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_int8)), ("start", C.POINTER(C.c_int64)),
                ("length", C.POINTER(C.c_int32)), ("nN", C.c_int64), ("nS", C.c_int64)]


_host = None


def host_lib():
    global _host
    if _host is None:
        L = C.CDLL(os.path.join(ROOT, "cfrk_amd", "libcfrk_host.so"))
        L.cfrk_host_parse_fasta.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(Batch)]
        L.cfrk_host_free_batch.argtypes = [C.POINTER(Batch)]
        L.cfrk_host_format_dense.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_char_p, C.c_size_t]
        L.cfrk_host_format_dense.restype = C.c_size_t
        _host = L
    return _host


def host_parse(raw, flags):
    """-> (rc, (data, start, length) or None) from cfrk_host_parse_fasta"""
    L = host_lib()
    b = Batch()
    rc = L.cfrk_host_parse_fasta(raw, len(raw), flags, C.byref(b))
    if rc:
        return rc, None
    data = np.ctypeslib.as_array(b.data, (max(b.nN, 1),))[:b.nN].copy()
    start = np.ctypeslib.as_array(b.start, (max(b.nS, 1),))[:b.nS].copy()
    length = np.ctypeslib.as_array(b.length, (max(b.nS, 1),))[:b.nS].copy()
    L.cfrk_host_free_batch(C.byref(b))
    return 0, (data, start, length)


def _seq(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def grammar_cases():
    """(name, text, expected host rc native, expected host rc compat)"""
    return [
        ("one record, final newline", b">a\nACGTACGT\n", 0, 0),
        ("one record, no final newline", b">a\nACGTACGT", 0, 0),          # compat drops the last base
        ("multi-line records", b">a\nACGT\nTTGA\nC\n>b\nGG\nA\n", 0, 0),
        ("crlf", b">a\r\nACGT\r\nTT\r\n>b\r\nG\r\n", 0, 0),
        ("two carriage returns", b">a\nACG\r\r\n", 0, 0),
        ("interior carriage return", b">a\nA\rC\nG\n", 0, 0),
        ("carriage return at the end of the text", b">a\nACG\r", 0, 0),
        ("blank lines inside and after", b">a\nAC\n\n\nGT\n\n>b\nA\n\n\n", 0, 0),
        ("lower case, N and other bytes", b">a\nacgtnNRYKM-*.\x00\xff\x80Uu\n", 0, 0),
        ("'>' in mid-line", b">a > b\nAC>GT\nA>\n", 0, 0),
        ("header as the last line, no newline", b">a\nACGT\n>x", 0, -3),
        ("header as the last line, newline", b">a\nACGT\n>x\n", 0, -3),
        ("two headers in a row", b">a\n>b\nACGT\n", 0, -3),
        ("starts with a base", b"ACGT\n>a\nAC\n", -2, -2),
        ("starts with a blank line", b"\n>a\nAC\n", -2, -2),
        ("empty text", b"", 0, 0),
        ("a single '>'", b">", 0, -3),
        ("only line breaks in a record", b">a\n\r\n\n>b\nA\n", 0, 0),
    ]


def seam_cases():
    """texts whose interesting byte sits on a tile boundary (T = CFRK_FASTA_TILE_BYTES)"""
    rng = np.random.default_rng(77)
    out = []

    def body(n, width=61):
        s = _seq(rng, n)
        return b"\n".join(s[o:o + width] for o in range(0, len(s), width))

    def pad_to(prefix_len, at):
        """sequence lines of exactly `at - prefix_len` bytes, the last one ending in a newline"""
        n = at - prefix_len
        b = body(n)[:n - 1] + b"\n"
        return b.replace(b"\n\n", b"A\n")

    for off in (T - 1, T, T + 1):
        head = b">first\n"
        t = head + pad_to(len(head), off) + b">second\nACGTTGCA\nAC\n"
        assert t[off:off + 1] == b">" and t[off - 1:off] == b"\n"
        out.append((f"'>' line start at offset {off}", t, 0, 0))
    head = b">a\n"
    fill = _seq(rng, T - 1 - len(head))
    out.append(("crlf split across T", head + fill + b"\r\nACGT\r\n", 0, 0))
    assert out[-1][1][T - 1:T + 1] == b"\r\n"
    fill = _seq(rng, T - 5 - len(head))
    out.append(("carriage returns across T, then newline", head + fill + b"\r" * 11 + b"\nACG\n", 0, 0))
    out.append(("carriage returns across T, then a base", head + fill + b"\r" * 11 + b"ACG\n", 0, 0))
    out.append(("carriage returns across T, then the end", head + fill + b"\r" * 11, 0, 0))
    out.append(("carriage returns up to T exactly", head + _seq(rng, T - 3 - len(head)) + b"\r\r\r", 0, 0))
    long_header = b">" + b"h" * (2 * T + 100) + b"\n"
    out.append(("header line longer than 2 T", b">a\nAC\n" + long_header + b"ACGT\nGG\n>c\nT\n", 0, 0))
    out.append(("header line longer than 2 T, with '>' and line-start look-alikes", b">" + b">ACGT" * (2 * T // 5 + 7) + b"\nACGT\n", 0, 0))
    out.append(("sequence line longer than 2 T", b">a\n" + _seq(rng, 2 * T + 333) + b"\n>b\n" + _seq(rng, 50) + b"\n", 0, 0))
    out.append(("sequence line longer than 2 T, no final newline", b">a\n" + _seq(rng, 2 * T + 333), 0, 0))
    hdrs = b"".join(b">h%05d\n" % i for i in range(3 * T // 7))
    out.append(("tiles made only of headers", b">a\nACGT\n" + hdrs + b"ACGT\n", 0, -3))
    out.append(("headers of two bytes", b">\n" * (T + 5) + b"A\n", 0, -3))
    out.append(("records of four bytes", b">\nA\n" * (T // 2 + 3), 0, 0))
    return out


def cr_run_cases():
    """(name, text, offset of the refused run or None).  The host parser accepts every one of these texts; the device
    parser refuses, in native mode only, a sequence line with more than CFRK_FASTA_MAX_CR_RUN carriage returns in a row
    -- exactly, wherever the run lies in the 16-byte pieces -- and names the run's first byte."""
    rng = np.random.default_rng(99)
    out = []
    for align in (0, 1, 5, 15):
        head = b">a\n" + _seq(rng, 61 + align)          # the run begins at offset 64 + align
        for tail, what in ((b"\nACGT\n", "newline"), (b"ACGT\n", "a base"), (b"", "the end")):
            out.append((f"{MAX_CR} carriage returns at offset 64+{align}, then {what}", head + b"\r" * MAX_CR + tail, None))
            out.append((f"{MAX_CR + 1} carriage returns at offset 64+{align}, then {what}", head + b"\r" * (MAX_CR + 1) + tail, 64 + align))
    out.append(("three times the bound", b">a\nAC\n>b\nACG" + b"\r" * (3 * MAX_CR) + b"\nA\n", 12))
    out.append(("two runs over the bound: the first is named", b">a\nAC" + b"\r" * (2 * MAX_CR) + b"G" + b"\r" * (2 * MAX_CR) + b"\n", 5))
    # a run behind a tile seam, no line start in that tile in front of it: only the scan knows whether it is in a header
    pre = T + 100
    out.append(("header line across a seam with a long run", b">a\nAC\n>" + b"h" * pre + b"\r" * (3 * MAX_CR) + b"h\nACGT\r\n", None))
    out.append(("header line with a long run in its own tile", b">" + b"\r" * (2 * MAX_CR) + b"\nACGT\n", None))
    out.append(("sequence line across a seam with a long run", b">a\n" + _seq(rng, pre) + b"\r" * (MAX_CR + 1) + b"A\n", 3 + pre))
    out.append(("sequence line across a seam with a run at the bound", b">a\n" + _seq(rng, pre) + b"\r" * MAX_CR + b"A\n", None))
    out.append(("a run over the bound that begins before a seam", b">a\n" + _seq(rng, T - 13) + b"\r" * (MAX_CR + 1) + b"\n", T - 10))
    out.append(("a run at the bound that begins before a seam", b">a\n" + _seq(rng, T - 13) + b"\r" * MAX_CR + b"\n>b\nAC\n", None))
    return out


def scan_block_case():
    """more than one block of the tile scan: CFRK_FASTA_SCAN_TILES + 3 tiles of short records"""
    rng = np.random.default_rng(5)
    n = (SCAN_TILES + 3) * T
    rec = [b">r\n" + _seq(rng, int(L)) + b"\n" for L in rng.integers(20, 90, 64)]
    idx = rng.integers(0, len(rec), n // 40)
    return b"".join(rec[i] for i in idx)[:n]


def random_texts(count=200, seed=2024):
    """seeded texts of 0 .. 3 T bytes over ACGTNacgt>\\r\\n, lines of 1 .. 200 bytes on average"""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"ACGTNacgt>\r\n", np.uint8)
    out = []
    for i in range(count):
        n = int(rng.integers(0, 3 * T + 1)) if i >= 8 else (0, 1, 2, 15, 16, 17, T, 3 * T)[i]
        line = float(rng.integers(1, 201))
        w = np.ones(len(alphabet))
        w[9] = rng.choice([0.0, 0.02, 0.2])                    # '>'
        w[10] = rng.choice([0.0, 0.2, 1.0, 9.0 / line * 3])    # '\r'
        w[11] = 9.0 / line * (1 + w[10] / 9)                   # '\n': one per `line` bytes or so
        a = alphabet[rng.choice(len(alphabet), n, p=w / w.sum())].copy()
        if n:
            after_nl = np.flatnonzero(a[:-1] == 10) + 1
            a[after_nl[rng.random(len(after_nl)) < rng.choice([0.005, 0.03, 0.3])]] = ord(">")
            if rng.random() < 0.85:
                a[0] = ord(">")
        out.append(a.tobytes())
    return out
