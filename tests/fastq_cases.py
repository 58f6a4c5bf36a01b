"""FASTQ texts for the parsers' tests (test_fastq_cpu.py, test_gpu_fastq.py) and the host parser they are held against.
Every text is generated here on the CPU.  What a parser must say about a text comes from tests/fastq_ref.py; the
refusal cases state cause and place by hand as well.

`python -m tests.fastq_cases --dump FILE` writes the small cases as length-prefixed texts (a little-endian uint64, then
the bytes) for tools/fastq_host_check.cpp, the sanitizer run of the host parser."""
import ctypes as C
import os
import re
import sys

import numpy as np

from .ingest_cases import Batch, ROOT, host_parse as host_parse_fasta

MIN_QUALS = (0, 1, 2, 20, 41, 93)
NO_AT, NO_PLUS, TRUNCATED, LENGTHS, LONG, MIN_QUAL = -5, -6, -7, -8, -9, -10
CAUSES = {NO_AT: "no_at", NO_PLUS: "no_plus", TRUNCATED: "truncated", LENGTHS: "lengths", LONG: "long", MIN_QUAL: "min_qual"}


def _header_int(name):
    text = open(os.path.join(ROOT, "include", "cfrk_abi.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


T = _header_int("CFRK_FASTQ_TILE_BYTES")
SCAN_TILES = _header_int("CFRK_FASTQ_SCAN_TILES")

_host = None


def host_lib():
    global _host
    if _host is None:
        L = C.CDLL(os.path.join(ROOT, "cfrk_amd", "libcfrk_host.so"))
        L.cfrk_host_parse_fastq.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(Batch), C.POINTER(C.c_uint64)]
        L.cfrk_host_read_fastq.argtypes = [C.c_char_p, C.c_int, C.POINTER(Batch), C.POINTER(C.c_uint64)]
        L.cfrk_host_sniff_format.argtypes = [C.c_char_p, C.c_size_t]
        L.cfrk_host_fastq_message.argtypes = [C.c_int, C.c_uint64, C.c_char_p, C.c_size_t]
        L.cfrk_host_fastq_message.restype = C.c_size_t
        L.cfrk_host_free_batch.argtypes = [C.POINTER(Batch)]
        L.cfrk_host_set_parse_threads.argtypes = [C.c_int]
        _host = L
    return _host


def _take(L, b):
    data = np.ctypeslib.as_array(b.data, (max(b.nN, 1),))[:b.nN].copy()
    start = np.ctypeslib.as_array(b.start, (max(b.nS, 1),))[:b.nS].copy()
    length = np.ctypeslib.as_array(b.length, (max(b.nS, 1),))[:b.nS].copy()
    L.cfrk_host_free_batch(C.byref(b))
    return data, start, length


def host_parse(raw, min_qual=0, threads=0):
    """-> (0, 0, (data, start, length)) or (rc, where, None) from cfrk_host_parse_fastq"""
    L = host_lib()
    b, where = Batch(), C.c_uint64(0)
    L.cfrk_host_set_parse_threads(threads)
    try:
        rc = L.cfrk_host_parse_fastq(raw, len(raw), min_qual, C.byref(b), C.byref(where))
    finally:
        L.cfrk_host_set_parse_threads(0)
    if rc:
        return rc, where.value, None
    return 0, 0, _take(L, b)


def _seq(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def _qual(rng, n, lo=33, hi=75):
    """n quality bytes; the first is never one of the line markers of another kind unless asked for"""
    return rng.integers(lo, hi, n, dtype=np.uint8).tobytes()


def _rec(rng, n, name=b"r", plus=b"", eol=b"\n"):
    return b"@" + name + eol + _seq(rng, n) + eol + b"+" + plus + eol + _qual(rng, n) + eol


def grammar_cases():
    """(name, text): texts every parser accepts, unless the name says otherwise (the restatement decides)"""
    return [
        ("one record, final newline", b"@a\nACGTACGT\n+\nIIII!!5I\n"),
        ("one record, no final newline", b"@a\nACGTACGT\n+\nIIII!!5I"),
        ("three records", b"@a\nACGT\n+\nII5I\n@b x y\nTTGACCA\n+\n#5I+I@I\n@c\nG\n+\n5\n"),
        ("crlf everywhere", b"@a\r\nACGT\r\n+\r\nI5I#\r\n@b\r\nGG\r\n+\r\n5I\r\n"),
        ("crlf everywhere, no final newline", b"@a\r\nACGT\r\n+\r\nI5I#\r\n@b\r\nGG\r\n+\r\n5I\r"),
        ("a lone carriage return inside a sequence line", b"@a\nA\rCG\n+\nI5II\n"),
        ("a lone carriage return inside a quality line", b"@a\nACGT\n+\nI\r5I\n"),
        ("two carriage returns in front of the newline: one is dropped", b"@a\nACG\r\r\n+\nII5\r\r\n"),
        ("carriage return as the last byte", b"@a\nACG\n+\nI5I\r"),
        ("'+name' lines", b"@a\nACGT\n+a\nI5I#\n@b\nAC\n+b and more @ + >\n5I\n"),
        ("quality lines that begin with '@', '+' and '>'", b"@a\nACGT\n+\n@II5\n@b\nACGT\n+\n+5II\n@c\nACGT\n+\n>I5I\n@d\nA\n+\n@\n"),
        ("sequence lines that begin with '@', '+' and '>'", b"@a\n@CGT\n+\nIII5\n@b\n+CGT\n+\n5III\n@c\n>CGT\n+\nI5II\n"),
        ("empty records", b"@a\n\n+\n\n@b\nAC\n+\nI5\n@c\n\n+\n\n"),
        ("an empty record at the end, crlf", b"@a\r\nAC\r\n+\r\nI5\r\n@b\r\n\r\n+\r\n\r\n"),
        ("a final empty quality line without its newline: three lines", b"@a\n\n+\n"),
        ("lower case, N and other bytes in the sequence", b"@a\nacgtnNRYKM-*.\x00\xff\x80Uu\n+\nIIIIIIIII5IIIIII5I\n"),
        ("quality bytes below 33 and 0xFF", b"@a\nACGTACGTAC\n+\n\x00\x01 !\x1f\xff\x80\x7fI5\n"),
        ("empty text", b""),
        ("a single '@'", b"@"),
        ("a single newline", b"\n"),
        ("sixteen and seventeen bytes", b"@\nACGT\n+\nIII5\n@\n\n+\n\n@ab\nAC\n+\n5I\n"),
    ]


def refusal_cases():
    """(name, text, cause, where) -- stated by hand; the restatement must say the same"""
    rng = np.random.default_rng(31)
    good = b"".join(_rec(rng, int(n), b"r%d" % i) for i, n in enumerate(rng.integers(1, 120, 60)))
    nl = [i for i, c in enumerate(good) if c == 10]

    def line_start(i):
        return 0 if i == 0 else nl[i - 1] + 1

    def put(text, at, byte):
        return text[:at] + byte + text[at + 1:]

    def drop_byte(text, at):
        return text[:at] + text[at + 1:]

    out = [
        ("no '@' on line 0", b"a\nACGT\n+\nIIII\n", "no_at", 0),
        ("FASTA input", b">a\nACGT\n", "no_at", 0),
        ("an empty first line", b"\n@a\nACGT\n+\nIIII\n", "no_at", 0),
        ("no '@' late", put(good, line_start(200), b"a"), "no_at", 200),
        ("no '+' early", b"@a\nACGT\n-\nIIII\n", "no_plus", 2),
        ("an empty '+' line", b"@a\nACGT\n\nIIII\n", "no_plus", 2),
        ("no '+' late", put(good, line_start(4 * 57 + 2), b"x"), "no_plus", 4 * 57 + 2),
        ("wrapped FASTQ", b"@a\nACGT\nACGT\n+\nIIII\nIIII\n", "no_plus", 2),
        ("4n + 1 lines", good + b"@x\n", "truncated", 241),
        ("4n + 1 lines, no final newline", good + b"@x", "truncated", 241),
        ("4n + 2 lines", good + b"@x\nAC\n", "truncated", 242),
        ("4n + 3 lines", good + b"@x\nAC\n+\n", "truncated", 243),
        ("4n + 3 lines, no final newline", good + b"@x\nAC\n+", "truncated", 243),
        ("a blank line at the end", good + b"\n", "no_at", 240),
        ("two blank lines at the end", good + b"\n\n", "no_at", 240),
        ("lengths differ early", b"@a\nACGT\n+\nIII\n@b\nAC\n+\nII\n", "lengths", 0),
        ("lengths differ late: a quality byte removed", drop_byte(good, line_start(4 * 58 + 3)), "lengths", 58),
        ("lengths differ in the last record", drop_byte(good, len(good) - 2), "lengths", 59),
        ("lengths differ in the last record, no final newline", good[:-2], "lengths", 59),
        ("lengths differ in two records, sums agree", b"@a\nACGT\n+\nIII\n@b\nAC\n+\nIII\n", "lengths", 0),
        ("an empty quality line for a base", b"@a\nA\n+\n\n", "lengths", 0),
        ("two structural faults: the earlier line wins ('+' first)", put(put(good, line_start(6), b"x"), line_start(16), b"x"), "no_plus", 6),
        ("two structural faults: the earlier line wins ('@' first)", put(put(good, line_start(8), b"x"), line_start(14), b"x"), "no_at", 8),
        ("a length mismatch and a later structural fault: the structural one wins",
         put(drop_byte(good, line_start(3)), line_start(100) - 1, b"x"), "no_at", 100),
        ("a bad line and a truncated record: the line wins", put(good, line_start(4 * 59), b"x") + b"@x\n", "no_at", 4 * 59),
        ("a length mismatch and a truncated record: the truncated record wins", drop_byte(good, line_start(3)) + b"@x\nA\n", "truncated", 242),
    ]
    # faults behind a tile seam: the fault's tile starts in another phase than 0, the faulty line start is a tile's first byte
    big = b"".join(_rec(rng, int(n), b"s%d" % i) for i, n in enumerate(rng.integers(60, 160, 3 * T // 200)))
    bnl = np.flatnonzero(np.frombuffer(big, np.uint8) == 10)
    for kind, cause in ((0, "no_at"), (2, "no_plus")):
        i = next(j for j in range(4 * 8 + kind, len(bnl), 4) if bnl[j - 1] + 1 > 2 * T + 50)
        out.append((f"a bad line of kind {kind} in the third tile", put(big, int(bnl[i - 1]) + 1, b"x"), cause, i))
    r = next(j for j in range(len(bnl) // 4) if bnl[4 * j + 2] > T + 100)
    out.append(("lengths differ in the second tile", drop_byte(big, int(bnl[4 * r + 2]) + 1), "lengths", r))

    def head(n):
        """a record of n bytes"""
        return b"@" + b"h" * (n - 14) + b"\nACGT\n+\nIIII\n"

    out.append(("a bad '@' line start as a tile's first byte", head(T) + b"xr\nAC\n+\nII\n", "no_at", 4))
    out.append(("a bad '+' line start as a tile's first byte", head(T - 6) + b"@r\nAC\nxx\nII\n", "no_plus", 6))
    assert all(c[1][T - 1:T + 1] == b"\nx" for c in out[-2:])
    return out


def seam_cases():
    """(name, text): valid texts whose interesting byte sits on a tile boundary (T = CFRK_FASTQ_TILE_BYTES)"""
    rng = np.random.default_rng(78)
    out = []
    # record 1 is "@r1\n" + 8 bases + "\n+r1\n" + 8 qualities + "\n": its lines start 0, 4, 13 and 17 bytes into it
    for kind, into in enumerate((0, 4, 13, 17)):
        for off in (T - 1, T, T + 1):
            head = b"@" + b"h" * (off - into - 14) + b"\n" + _seq(rng, 4) + b"\n+\n" + _qual(rng, 4) + b"\n"     # off - into bytes
            t = head + b"@r1\n" + _seq(rng, 8) + b"\n+r1\n" + _qual(rng, 8) + b"\n" + _rec(rng, 33) + _rec(rng, 5)
            assert t[off - 1:off] == b"\n" and t[:off].count(b"\n") == 4 + kind
            out.append((f"a line start of kind {kind} at offset {off}", t))
    for what, h in (("sequence", T - 4 - 40), ("quality", T - 9 - 80)):
        # "\r\n" of a crlf text split across T: '@', h name bytes, "\r\n", 40 bases, "\r\n+\r\n", 40 qualities, "\r\n"
        t = b"@" + b"a" * h + b"\r\n" + _seq(rng, 40) + b"\r\n+\r\n" + _qual(rng, 40) + b"\r\n@b\r\nACGT\r\n+\r\nI5I5\r\n"
        assert t[T - 1:T + 1] == b"\r\n" and t[:T - 1].count(b"\n") == (1 if what == "sequence" else 3)
        out.append((f"crlf split across T at the end of a {what} line", t))
    long = 2 * T + 333
    out.append(("a header line longer than 2 T", _rec(rng, 7) + b"@" + b"h@+>" * (long // 4) + b"\nACGT\n+\nI5I5\n" + _rec(rng, 9)))
    out.append(("a '+' line longer than 2 T", _rec(rng, 7) + b"@r\nACGT\n+" + b"p@+>" * (long // 4) + b"\nI5I5\n" + _rec(rng, 9)))
    out.append(("a read longer than 2 T (a tile of sequence bytes only, a tile of quality bytes only)", _rec(rng, 7) + _rec(rng, long) + _rec(rng, 9)))
    out.append(("a read longer than 2 T, no final newline", _rec(rng, 3) + _rec(rng, long)[:-1]))
    out.append(("a read longer than 2 T, crlf", _rec(rng, 3, eol=b"\r\n") + _rec(rng, long, eol=b"\r\n")))
    out.append(("records of eight bytes", b"@\nA\n+\nI\n" * (T // 4 + 3)))
    out.append(("empty records of six bytes", b"@\n\n+\n\n" * (T // 3 + 5)))
    return out


_scan_block = None


def scan_block_case():
    """more than one block of the tile scan: over CFRK_FASTQ_SCAN_TILES + 3 tiles of short records"""
    global _scan_block
    if _scan_block is None:
        rng = np.random.default_rng(6)
        n = (SCAN_TILES + 3) * T
        rec = [_rec(rng, int(L), b"r%d" % i) for i, L in enumerate(rng.integers(20, 160, 64))]
        idx = rng.integers(0, len(rec), n // 40)
        sizes = np.cumsum([len(rec[i]) for i in idx])
        _scan_block = b"".join(rec[i] for i in idx[:int(np.searchsorted(sizes, n)) + 1])
    return _scan_block


def random_texts(count=200, seed=2025):
    """seeded texts of 0 .. 3 T bytes: valid four-line FASTQ with random line widths, line ends and quality ranges; a
    share of them mutated -- a line dropped, a marker byte changed, a quality byte removed, '\\r' sprinkled"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        target = int(rng.integers(0, 3 * T + 1)) if i >= 6 else (0, 7, 15, 16, T, 3 * T)[i]
        width = int(rng.choice([0, 1, 3, 30, 150, 600, 5000]))
        eol = b"\r\n" if rng.random() < 0.25 else b"\n"
        qlo = int(rng.choice([33, 33, 20, 0]))
        qhi = int(rng.choice([75, 127, 256]))
        parts, size = [], 0
        while True:
            n = int(rng.integers(0, 2 * width + 1))
            name = b"x" * int(rng.integers(0, 20))
            r = b"@" + name + eol + _seq(rng, n) + eol + b"+" + (name if rng.random() < 0.3 else b"") + eol + _qual(rng, n, qlo, qhi).replace(b"\n", b"5").replace(b"\r", b"6") + eol
            if size + len(r) > target:
                break
            parts.append(r)
            size += len(r)
        t = b"".join(parts)
        if t and rng.random() < 0.3:
            t = t[:-len(eol)]                         # no final line end
        mutation = rng.random()
        if t and mutation < 0.4:
            a = bytearray(t)
            nls = [j for j, c in enumerate(a) if c == 10]
            kind = int(rng.integers(0, 4))
            if kind == 0 and len(nls) > 1:            # a line dropped
                j = int(rng.integers(0, len(nls) - 1))
                del a[nls[j] + 1:nls[j + 1] + 1]
            elif kind == 1 and nls:                   # a marker (or another line's first byte) changed
                j = int(rng.integers(0, len(nls)))
                at = 0 if j == 0 else nls[j - 1] + 1
                a[at] = int(rng.choice(list(b"@+>A\n")))
            elif kind == 2:                           # one byte removed (a quality byte, often)
                del a[int(rng.integers(0, len(a)))]
            else:                                     # '\r' sprinkled
                for at in rng.integers(0, len(a), int(rng.integers(1, 12))):
                    a[int(at)] = 13
            t = bytes(a)
        out.append(t)
    return out


def small_cases():
    """every small text, named: what the CPU test, the GPU test and the sanitizer run walk"""
    out = [(n, t) for n, t in grammar_cases()] + [(c[0], c[1]) for c in refusal_cases()] + seam_cases()
    return out + [(f"random text {i}", t) for i, t in enumerate(random_texts())]


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--dump":
        sys.exit("usage: python -m tests.fastq_cases --dump FILE")
    with open(sys.argv[2], "wb") as f:
        for _, text in small_cases():
            f.write(len(text).to_bytes(8, "little") + text)
