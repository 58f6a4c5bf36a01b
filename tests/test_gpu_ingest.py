"""The device FASTA parser (cfrk_fasta_parse_device / cfrk_fasta_parse, cfrk_amd/csrc/ingest.hip) against the host
parser on the same bytes: data, start, length, nN and nS exactly, in both modes; where the host parser refuses a text
the device call returns CFRK_ERR_LAYOUT.  The texts come from tests/ingest_cases.py (test_ingest_cpu.py holds the host
parser to what that file states)."""
import os
import subprocess

import numpy as np
import pytest

import cfrk_amd
from cfrk_amd.lib import CfrkError

from . import ingest_cases as ic
from . import ref_lib as ref

pytestmark = pytest.mark.gpu

ROOT = ic.ROOT
T = ic.T
ERR_ARG, ERR_LAYOUT, ERR_ALIGN, ERR_SMALL_BUF = -1, -5, -7, -9
MODES = [(ic.NATIVE, 0), (ic.COMPAT, cfrk_amd.CFRK_COMPAT)]
GUARD = 64


class Dev:
    """device buffers shared by the cases: text, data, start, length, each with guard bytes behind it"""

    def __init__(self, ctx, cap):
        self.ctx, self.cap = ctx, cap
        self.d_text = ctx.alloc(cap + 64)
        self.d_data = ctx.alloc(cap + GUARD)
        self.d_start = ctx.alloc((cap + 1) // 2 * 8 + GUARD)
        self.d_length = ctx.alloc((cap + 1) // 2 * 4 + GUARD)

    def close(self):
        for p in (self.d_text, self.d_data, self.d_start, self.d_length):
            self.ctx.free(p)

    def put(self, raw, at=0):
        if len(raw):
            self.ctx.h2d(self.d_text + at, np.frombuffer(raw, np.uint8))

    def fetch(self, nN, nS):
        data, start, length = np.empty(nN, np.int8), np.empty(nS, np.int64), np.empty(nS, np.int32)
        self.ctx.sync()
        for a, p in ((data, self.d_data), (start, self.d_start), (length, self.d_length)):
            if a.size:
                self.ctx.d2h(a, p)
        return data, start, length

    def parse(self, raw, flags):
        """-> (0, (data, start, length)) or (error code, None), with the capacities the header promises"""
        self.put(raw)
        try:
            nN, nS = self.ctx.parse_fasta_device(self.d_text, len(raw), flags, self.d_data, len(raw), self.d_start,
                                                 self.d_length, (len(raw) + 1) // 2)
        except CfrkError as e:
            return e.code, None
        return 0, self.fetch(nN, nS)


@pytest.fixture(scope="module")
def ctx():
    c = cfrk_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dev(ctx):
    d = Dev(ctx, (ic.SCAN_TILES + 3) * T)
    yield d
    d.close()


def _same(dev, raw, what, want_rcs=None):
    for i, (hflags, dflags) in enumerate(MODES):
        hrc, want = ic.host_parse(raw, hflags)
        if want_rcs is not None:
            assert hrc == want_rcs[i], f"{what}: the host parser returns {hrc}"
        rc, got = dev.parse(raw, dflags)
        mode = "compat" if hflags else "native"
        if hrc:
            assert rc == ERR_LAYOUT, f"{what} ({mode}): host rc {hrc}, device rc {rc}"
            continue
        assert rc == 0, f"{what} ({mode}): device rc {rc}: {dev.ctx._L.cfrk_last_error(dev.ctx._h).decode()}"
        for name, g, w in zip(("data", "start", "length"), got, want):
            assert g.shape == w.shape, f"{what} ({mode}): {name} has {g.size} entries, the host parser's {w.size}"
            if not (g == w).all():
                j = int(np.flatnonzero(g != w)[0])
                raise AssertionError(f"{what} ({mode}): {name}[{j}] = {g[j]}, the host parser's {w[j]} ({len(raw)} bytes of text)")


@pytest.mark.parametrize("case", ic.grammar_cases(), ids=lambda c: c[0])
def test_grammar(dev, case):
    name, raw, rn, rc = case
    _same(dev, raw, name, (rn, rc))


@pytest.mark.parametrize("case", ic.seam_cases(), ids=lambda c: c[0])
def test_tile_seams(dev, case):
    name, raw, rn, rc = case
    _same(dev, raw, name, (rn, rc))


def test_more_than_one_block_of_the_tile_scan(dev):
    raw = ic.scan_block_case()
    assert len(raw) > ic.SCAN_TILES * T
    _same(dev, raw, "scan blocks", (0, 0))


def test_random_texts(dev):
    for i, raw in enumerate(ic.random_texts()):
        _same(dev, raw, f"random text {i}")


def test_error_text_names_the_cause(ctx, dev):
    dev.put(b"ACGT\n>a\nA\n")
    with pytest.raises(CfrkError, match="before the first header") as e:
        ctx.parse_fasta_device(dev.d_text, 10, 0, dev.d_data, 10, dev.d_start, dev.d_length, 5)
    assert e.value.code == ERR_LAYOUT
    dev.put(b">a\nAC\n>b\n>c\nA\n")
    with pytest.raises(CfrkError, match="without a sequence line.*byte offset 9") as e:
        ctx.parse_fasta_device(dev.d_text, 14, cfrk_amd.CFRK_COMPAT, dev.d_data, 14, dev.d_start, dev.d_length, 7)
    assert e.value.code == ERR_LAYOUT


@pytest.mark.parametrize("case", ic.cr_run_cases(), ids=lambda c: c[0])
def test_carriage_return_bound(ctx, dev, case):
    """the one text the host parser accepts and the device parser refuses: a sequence line with more than
    CFRK_FASTA_MAX_CR_RUN carriage returns in a row, native mode; exact at the bound, never in a header, never in compat"""
    name, raw, refused_at = case
    hrc, want = ic.host_parse(raw, ic.COMPAT)
    rc, got = dev.parse(raw, cfrk_amd.CFRK_COMPAT)
    assert hrc == 0 and rc == 0 and all(g.shape == w.shape and (g == w).all() for g, w in zip(got, want)), name
    if refused_at is None:
        _same(dev, raw, name, (0, 0))
        return
    dev.put(raw)
    with pytest.raises(CfrkError, match=r"more than %d carriage returns in a row.* byte offset %d$" % (ic.MAX_CR, refused_at)) as e:
        ctx.parse_fasta_device(dev.d_text, len(raw), 0, dev.d_data, len(raw), dev.d_start, dev.d_length, (len(raw) + 1) // 2)
    assert e.value.code == ERR_LAYOUT and (e.value.nN, e.value.nS) == (0, 0)


def test_staged_copy_equals_the_plain_one(ctx):
    rng = np.random.default_rng(1)
    for n in (0, 1000, (8 << 20) - 1, (37 << 20) + 12345):       # below the ring's threshold; whole and partial pieces
        a = rng.integers(0, 256, n, dtype=np.uint8)
        d = ctx.alloc(n + 16)
        try:
            ctx.h2d_staged(d, a)
            b = np.empty(n, np.uint8)
            if n:
                ctx.d2h(b, d)
        finally:
            ctx.free(d)
        assert (a == b).all()


def test_capacities(ctx, dev):
    rng = np.random.default_rng(3)
    raw = b"".join(b">r%d\n%s\n" % (i, ic._seq(rng, int(rng.integers(1, 300)))) for i in range(300))
    _, (wdata, wstart, wlength) = ic.host_parse(raw, ic.NATIVE)
    nN, nS = len(wdata), len(wstart)
    dev.put(raw)
    fill = np.full(dev.cap + GUARD, 0x5A, np.uint8)
    for p, nbytes in ((dev.d_data, dev.cap + GUARD), (dev.d_start, nS * 8 + GUARD), (dev.d_length, nS * 4 + GUARD)):
        ctx.h2d(p, fill[:nbytes])

    def untouched(data_bytes, start_bytes, length_bytes):
        """everything behind the given number of bytes of each array still holds the fill"""
        for p, used, total in ((dev.d_data, data_bytes, nN + GUARD), (dev.d_start, start_bytes, nS * 8 + GUARD),
                               (dev.d_length, length_bytes, nS * 4 + GUARD)):
            a = np.empty(total, np.uint8)
            ctx.d2h(a, p)
            assert (a[used:] == 0x5A).all()

    # the sizing call, then each capacity one short: sizes complete, nothing written
    for args in ((0, 0, 0, 0, 0), (dev.d_data, nN - 1, dev.d_start, dev.d_length, nS), (dev.d_data, nN, dev.d_start, dev.d_length, nS - 1)):
        with pytest.raises(CfrkError) as e:
            ctx.parse_fasta_device(dev.d_text, len(raw), 0, *args)
        assert e.value.code == ERR_SMALL_BUF and (e.value.nN, e.value.nS) == (nN, nS)
        ctx.sync()
        untouched(0, 0, 0)
    assert ctx.parse_fasta_device(dev.d_text, len(raw), 0, dev.d_data, nN, dev.d_start, dev.d_length, nS) == (nN, nS)
    got = dev.fetch(nN, nS)
    assert (got[0] == wdata).all() and (got[1] == wstart).all() and (got[2] == wlength).all()
    untouched(nN, nS * 8, nS * 4)


def test_arguments(ctx, dev):
    raw = b">a\nACGT\n"
    dev.put(raw, at=1)
    with pytest.raises(CfrkError) as e:
        ctx.parse_fasta_device(dev.d_text + 1, len(raw), 0, dev.d_data, 64, dev.d_start, dev.d_length, 8)
    assert e.value.code == ERR_ALIGN
    dev.put(raw)
    for flags in (cfrk_amd.CFRK_CANONICAL, cfrk_amd.CFRK_COMPAT | 0x40, -1):
        with pytest.raises(CfrkError) as e:
            ctx.parse_fasta_device(dev.d_text, len(raw), flags, dev.d_data, 64, dev.d_start, dev.d_length, 8)
        assert e.value.code == ERR_ARG
    with pytest.raises(CfrkError) as e:
        ctx.parse_fasta_device(0, len(raw), 0, dev.d_data, 64, dev.d_start, dev.d_length, 8)
    assert e.value.code == ERR_ARG
    L = ctx._L
    assert L.cfrk_fasta_parse_device(ctx._h, dev.d_text, len(raw), 0, dev.d_data, 64, dev.d_start, dev.d_length, 8, None, None) == ERR_ARG
    # a data array that is not 16-byte aligned is fine
    nN, nS = ctx.parse_fasta_device(dev.d_text, len(raw), 0, dev.d_data + 3, 64, dev.d_start, dev.d_length, 8)
    a = np.empty(nN, np.int8)
    ctx.sync()
    ctx.d2h(a, dev.d_data + 3)
    assert (nN, nS) == (5, 1) and a.tolist() == [0, 1, 2, 3, -1]


def test_host_form_and_python_wrapper(ctx):
    for _, raw, rn, rc in ic.grammar_cases()[:10] + ic.seam_cases()[:5]:
        for hflags, dflags in MODES:
            hrc, want = ic.host_parse(raw, hflags)
            if hrc:
                with pytest.raises(CfrkError) as e:
                    ctx.parse_fasta(raw, dflags)
                assert e.value.code == ERR_LAYOUT
                continue
            got = ctx.parse_fasta(raw if hflags else np.frombuffer(raw, np.uint8), dflags)
            assert all(g.dtype == w.dtype and g.shape == w.shape and (g == w).all() for g, w in zip(got, want))


def test_parsed_reads_feed_the_counting_calls(ctx, dev):
    """native parse of ~2000 reads -> cfrk_global_add_device (k = 31 canonical) and cfrk_per_read_sparse_device"""
    rng = np.random.default_rng(11)
    genome = ic._seq(rng, 20000)
    parts = []
    for i in range(2000):
        o, n = int(rng.integers(0, 19000)), int(rng.integers(40, 400))
        s = genome[o:o + n]
        parts.append(b">read%d\n" % i + b"\n".join(s[j:j + 70] for j in range(0, len(s), 70)) + b"\n")
    raw = b"".join(parts)
    _, (data, start, length) = ic.host_parse(raw, ic.NATIVE)
    rc, got = dev.parse(raw, 0)
    assert rc == 0 and (got[0] == data).all()
    nN, nS = len(data), len(start)
    g = cfrk_amd.GlobalCounter(ctx, 31, cfrk_amd.CFRK_CANONICAL, 1 << 20)
    g.add(data, start, length)
    want = g.digest()
    g = cfrk_amd.GlobalCounter(ctx, 31, cfrk_amd.CFRK_CANONICAL, 1 << 20)
    g.add_device(dev.d_data, nN)
    assert g.digest() == want and want[0] > 10000
    wrow, wkeys, wcnt = ctx.per_read_sparse(data, start, length, 31, cfrk_amd.CFRK_CANONICAL)
    d_row, d_keys, d_cnt = ctx.alloc((nS + 1) * 8), ctx.alloc(len(wkeys) * 8), ctx.alloc(len(wkeys) * 4)
    try:
        nnz = ctx.per_read_sparse_device(dev.d_data, dev.d_start, dev.d_length, nN, nS, 31, cfrk_amd.CFRK_CANONICAL,
                                         d_row, d_keys, d_cnt, len(wkeys))
        row, keys, cnt = np.empty(nS + 1, np.int64), np.empty(nnz, np.uint64), np.empty(nnz, np.uint32)
        ctx.sync()
        for a, p in ((row, d_row), (keys, d_keys), (cnt, d_cnt)):
            ctx.d2h(a, p)
    finally:
        for p in (d_row, d_keys, d_cnt):
            ctx.free(p)
    assert nnz == len(wkeys) and (row == wrow).all() and (keys == wkeys).all() and (cnt == wcnt).all()


def _crlf_fasta(path):
    rng = np.random.default_rng(8)
    genome = ic._seq(rng, 30000)
    with open(path, "wb") as f:
        for i in range(1500):
            o, n = int(rng.integers(0, 29000)), int(rng.integers(35, 500))
            s = genome[o:o + n]
            f.write(b">r%d x\r\n" % i + b"".join(s[j:j + 60] + b"\r\n" for j in range(0, len(s), 60)))
    return str(path)


@pytest.mark.parametrize("k", [15, 31])
@pytest.mark.parametrize("which", ["golden", "crlf"])
def test_cli_device_parse_writes_the_same_files(tmp_path, which, k):
    cli = os.path.join(ROOT, "cfrk_amd", "cfrk")
    fasta = os.path.join(ROOT, "tests", "golden", "seq2-derived.fasta") if which == "golden" else _crlf_fasta(tmp_path / "crlf.fasta")
    for tail in (["--histo", "HISTO"], ["--binary"], ["--auto-hint"]):
        files = []
        # (--binary also through the ring of pinned staging buffers)
        for extra in ([], ["--device-parse"]) + ((["--device-parse", "--text-copy", "staged"],) if tail == ["--binary"] else ()):
            out, histo = tmp_path / "out.bin", tmp_path / "histo.txt"
            for p in (out, histo):
                if p.exists():
                    p.unlink()
            args = [str(histo) if a == "HISTO" else a for a in tail]
            subprocess.run([cli, fasta, str(out), str(k), "--global", "--canonical"] + args + extra, check=True, timeout=120,
                           stdout=subprocess.DEVNULL)
            files.append((out.read_bytes(), histo.read_bytes() if histo.exists() else b""))
        assert files[0][0] and all(f == files[0] for f in files[1:]), f"{which} k={k} {tail}"


def test_cli_device_parse_reports_what_the_host_parser_reports(tmp_path):
    cli = os.path.join(ROOT, "cfrk_amd", "cfrk")
    bad = tmp_path / "bad.fasta"
    bad.write_bytes(b"ACGT\n>a\nACGT\n")
    res = [subprocess.run([cli, str(bad), str(tmp_path / "o"), "15", "--global"] + extra, capture_output=True, text=True, timeout=60)
           for extra in ([], ["--device-parse"])]
    assert res[0].returncode == res[1].returncode == 1
    assert res[0].stderr.strip() == res[1].stderr.strip() and "(error -2)" in res[1].stderr


def test_cli_device_parse_on_an_empty_file_and_on_a_refused_run(tmp_path):
    cli = os.path.join(ROOT, "cfrk_amd", "cfrk")
    empty = tmp_path / "empty.fasta"
    empty.write_bytes(b"")
    outs = []
    for extra in ([], ["--device-parse"]):
        out = tmp_path / "out.txt"
        if out.exists():
            out.unlink()
        subprocess.run([cli, str(empty), str(out), "15", "--global"] + extra, check=True, timeout=60, stdout=subprocess.DEVNULL)
        outs.append(out.read_bytes())
    assert outs[0] == outs[1]
    # the host parser takes this file, the device parser refuses it and says why
    cr = tmp_path / "cr.fasta"
    cr.write_bytes(b">a\nACGT" + b"\r" * (ic.MAX_CR + 1) + b"\n")
    res = [subprocess.run([cli, str(cr), str(tmp_path / "o"), "15", "--global"] + extra, capture_output=True, text=True, timeout=60)
           for extra in ([], ["--device-parse"])]
    assert res[0].returncode == 0 and res[1].returncode == 1
    assert f"more than {ic.MAX_CR} carriage returns in a row" in res[1].stderr and "byte offset 7" in res[1].stderr


@pytest.mark.skipif(not ref.have_ref(), reason=ref.SKIP_REASON)
def test_compat_parse_and_dense_count_write_the_reference_cli_file(ctx, dev, tmp_path):
    rng = np.random.default_rng(21)
    parts = []
    for i in range(40):
        s = ic._seq(rng, int(rng.integers(25, 200)))
        parts.append(b">r%d some text\n" % i + b"".join(s[j:j + 17] + b"\n" for j in range(0, len(s), 17)))
    raw = b"".join(parts)
    fa = tmp_path / "in.fasta"
    fa.write_bytes(raw)
    k = 3
    want = ref.run_cli(fa, tmp_path / "ref.cfrk", (k,), timeout=60)
    rc, (data, start, length) = dev.parse(raw, cfrk_amd.CFRK_COMPAT)
    assert rc == 0
    nN, nS = len(data), len(start)
    d_freq = ctx.alloc(nS * 4 ** k * 4)
    try:
        ctx.check(ctx._L.cfrk_per_read_dense_device(ctx._h, dev.d_data, dev.d_start, dev.d_length, nN, nS, k, cfrk_amd.CFRK_COMPAT, d_freq),
                  "cfrk_per_read_dense_device")
        freq = np.empty(nS * 4 ** k, np.int32)
        ctx.sync()
        ctx.d2h(freq, d_freq)
    finally:
        ctx.free(d_freq)
    H = ic.host_lib()
    size = H.cfrk_host_format_dense(freq.ctypes.data, nS, k, None, 0)
    buf = (ic.C.c_char * size)()
    assert H.cfrk_host_format_dense(freq.ctypes.data, nS, k, buf, size) == size
    assert want and bytes(buf) == want
