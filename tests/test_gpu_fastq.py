"""The device FASTQ parser (cfrk_fastq_parse_device / cfrk_fastq_parse, cfrk_amd/csrc/ingest_fastq.hip) against the host
parser and the plain-Python restatement of the grammar (tests/fastq_ref.py) on the same bytes: data, start, length, nN
and nS exactly for every min_qual; where they refuse a text the device call returns CFRK_ERR_LAYOUT and names the same
cause and place.  The texts come from tests/fastq_cases.py (test_fastq_cpu.py holds the host parser to the restatement
and to the FASTA parser)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import cfrk_amd
from cfrk_amd.lib import CfrkError

from . import fastq_cases as fc
from . import fastq_ref as fr

pytestmark = pytest.mark.gpu

ROOT = fc.ROOT
T = fc.T
ERR_ARG, ERR_LAYOUT, ERR_ALIGN, ERR_SMALL_BUF = -1, -5, -7, -9
GUARD = 64
FILL = 0x5A


def cap_data(nbytes):
    return nbytes // 2             # the capacities the header promises to suffice


def cap_reads(nbytes):
    return (nbytes + 1) // 6


class Dev:
    """device buffers shared by the cases: text, data, start, length, the last three with guard bytes behind them"""

    def __init__(self, ctx, cap):
        self.ctx, self.cap = ctx, cap
        self.d_text = ctx.alloc(cap + 64)
        self.d_data = ctx.alloc(cap_data(cap) + GUARD)
        self.d_start = ctx.alloc(cap_reads(cap) * 8 + GUARD)
        self.d_length = ctx.alloc(cap_reads(cap) * 4 + GUARD)

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

    def parse(self, raw, min_qual, put=True):
        """-> (0, (data, start, length), "") or (error code, None, message), with the capacities the header promises"""
        if put:
            self.put(raw)
        try:
            nN, nS = self.ctx.parse_fastq_device(self.d_text, len(raw), min_qual, self.d_data, cap_data(len(raw)), self.d_start,
                                                 self.d_length, cap_reads(len(raw)))
        except CfrkError as e:
            return e.code, None, str(e)
        return 0, self.fetch(nN, nS), ""


@pytest.fixture(scope="module")
def ctx():
    c = cfrk_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dev(ctx):
    d = Dev(ctx, len(fc.scan_block_case()) + T)
    yield d
    d.close()


def _message(raw, verdict):
    """the words cfrk_last_error must hold for a refusal of the restatement's"""
    cause, where = verdict
    if cause in ("no_at", "no_plus"):
        return r"FASTQ: line %d does not begin with '%s' \(byte offset %d\)$" % (where, "@" if cause == "no_at" else r"\+", fr.lines_of(raw)[where][0])
    if cause == "truncated":
        return r"FASTQ: %d lines, not a multiple of four$" % where
    assert cause == "lengths"
    return r"FASTQ: record %d has sequence and quality lines of different lengths$" % where


def _same_arrays(got, want, what):
    for name, g, w in zip(("data", "start", "length"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name} has {g.size} entries, expected {w.size}"
        if not (g == w).all():
            j = int(np.flatnonzero(g != w)[0])
            raise AssertionError(f"{what}: {name}[{j}] = {g[j]}, expected {w[j]}")


def _held(dev, raw, what, min_quals=fc.MIN_QUALS, restatement=True):
    dev.put(raw)
    for q in min_quals:
        hrc, hwhere, hgot = fc.host_parse(raw, q)
        rc, got, msg = dev.parse(raw, q, put=False)
        tag = f"{what} (min_qual {q}, {len(raw)} bytes)"
        if hrc:
            verdict = (fc.CAUSES[hrc], hwhere)
            if restatement:
                assert fr.parse(raw, q) == verdict, tag
            assert rc == ERR_LAYOUT and re.search(_message(raw, verdict), msg), f"{tag}: host {verdict}, device rc {rc}: {msg}"
            continue
        assert rc == 0, f"{tag}: device rc {rc}: {msg}"
        _same_arrays(got, hgot, tag + ": against the host parser")
        if restatement:
            _same_arrays(got, fr.parse(raw, q)[1:], tag + ": against the restatement")


@pytest.mark.parametrize("case", fc.grammar_cases(), ids=lambda c: c[0])
def test_grammar(dev, case):
    _held(dev, case[1], case[0])


@pytest.mark.parametrize("case", fc.refusal_cases(), ids=lambda c: c[0])
def test_refusals_name_cause_and_place(dev, case):
    name, raw, cause, where = case
    for q in (0, 20):
        rc, _, msg = dev.parse(raw, q)
        assert rc == ERR_LAYOUT and re.search(_message(raw, (cause, where)), msg), f"{name}: rc {rc}: {msg}"


@pytest.mark.parametrize("case", fc.seam_cases(), ids=lambda c: c[0])
def test_tile_seams(dev, case):
    _held(dev, case[1], case[0])


def test_more_than_one_block_of_the_tile_scan(dev):
    raw = fc.scan_block_case()
    assert len(raw) > fc.SCAN_TILES * T
    _held(dev, raw, "scan blocks", min_quals=(0, 20), restatement=False)       # (test_fastq_cpu.py holds the host parser to the restatement here)
    # faults behind the first scan block: a marker, then a missing quality byte, in the last record
    nlines = raw.count(b"\n")
    at = int(np.flatnonzero(np.frombuffer(raw, np.uint8) == 10)[nlines - 5]) + 1       # the last record's '@'
    assert raw[at:at + 1] == b"@" and raw.endswith(b"\n") and nlines % 4 == 0
    rc, _, msg = dev.parse(raw[:at] + b"x" + raw[at + 1:], 20)
    assert rc == ERR_LAYOUT and msg.endswith(f"FASTQ: line {nlines - 4} does not begin with '@' (byte offset {at})"), msg
    rc, _, msg = dev.parse(raw[:-2] + b"\n", 20)
    assert rc == ERR_LAYOUT and msg.endswith(f"FASTQ: record {nlines // 4 - 1} has sequence and quality lines of different lengths"), msg


def test_random_texts(dev):
    for i, raw in enumerate(fc.random_texts()):
        _held(dev, raw, f"random text {i}")


def test_min_qual_outside_its_range(ctx, dev):
    raw = b"@a\nACGT\n+\nIIII\n"
    dev.put(raw)
    for q in (94, -1):
        with pytest.raises(CfrkError) as e:
            ctx.parse_fastq_device(dev.d_text, len(raw), q, dev.d_data, 64, dev.d_start, dev.d_length, 8)
        assert e.value.code == ERR_ARG
        with pytest.raises(CfrkError) as e:
            ctx.parse_fastq(raw, q)
        assert e.value.code == ERR_ARG
    assert ctx.parse_fastq_device(dev.d_text, len(raw), 93, dev.d_data, 64, dev.d_start, dev.d_length, 8) == (5, 1)
    assert dev.fetch(5, 1)[0].tolist() == [-1, -1, -1, -1, -1]


def test_capacities_and_guard_bytes(ctx, dev):
    rng = np.random.default_rng(4)
    raw = b"".join(fc._rec(rng, int(rng.integers(0, 300)), b"r%d" % i) for i in range(299)) + fc._rec(rng, 50)
    _, _, (wdata, wstart, wlength) = fc.host_parse(raw, 20)
    nN, nS = len(wdata), len(wstart)
    dev.put(raw)
    fill = np.full(nN + GUARD, FILL, np.uint8)
    for p, nbytes in ((dev.d_data, nN + GUARD), (dev.d_start, nS * 8 + GUARD), (dev.d_length, nS * 4 + GUARD)):
        ctx.h2d(p, fill[:nbytes])

    def untouched(data_bytes, start_bytes, length_bytes):
        """everything behind the given number of bytes of each array still holds the fill"""
        for p, used, total in ((dev.d_data, data_bytes, nN + GUARD), (dev.d_start, start_bytes, nS * 8 + GUARD),
                               (dev.d_length, length_bytes, nS * 4 + GUARD)):
            a = np.empty(total, np.uint8)
            ctx.d2h(a, p)
            assert (a[used:] == FILL).all()

    # the sizes-only call, then each capacity one short: sizes complete, nothing written
    for args in ((0, 0, 0, 0, 0), (dev.d_data, nN - 1, dev.d_start, dev.d_length, nS), (dev.d_data, nN, dev.d_start, dev.d_length, nS - 1)):
        with pytest.raises(CfrkError) as e:
            ctx.parse_fastq_device(dev.d_text, len(raw), 20, *args)
        assert e.value.code == ERR_SMALL_BUF and (e.value.nN, e.value.nS) == (nN, nS)
        ctx.sync()
        untouched(0, 0, 0)
    # exact capacities
    assert ctx.parse_fastq_device(dev.d_text, len(raw), 20, dev.d_data, nN, dev.d_start, dev.d_length, nS) == (nN, nS)
    _same_arrays(dev.fetch(nN, nS), (wdata, wstart, wlength), "exact capacities")
    untouched(nN, nS * 8, nS * 4)
    # a text that is refused late (the last record's quality line is short): nothing behind the capacities either
    bad = raw[:-2] + b"\n"
    dev.put(bad)
    with pytest.raises(CfrkError) as e:
        ctx.parse_fastq_device(dev.d_text, len(bad), 20, dev.d_data, nN, dev.d_start, dev.d_length, nS)
    assert e.value.code == ERR_LAYOUT
    untouched(nN, nS * 8, nS * 4)


def test_arguments(ctx, dev):
    raw = b"@a\nACGT\n+\nII5I\n"
    dev.put(raw, at=1)
    with pytest.raises(CfrkError) as e:
        ctx.parse_fastq_device(dev.d_text + 1, len(raw), 0, dev.d_data, 64, dev.d_start, dev.d_length, 8)
    assert e.value.code == ERR_ALIGN
    dev.put(raw)
    with pytest.raises(CfrkError) as e:
        ctx.parse_fastq_device(0, len(raw), 0, dev.d_data, 64, dev.d_start, dev.d_length, 8)
    assert e.value.code == ERR_ARG
    with pytest.raises(CfrkError) as e:
        ctx.parse_fastq_device(dev.d_text, len(raw), 0, 0, 64, dev.d_start, dev.d_length, 8)
    assert e.value.code == ERR_ARG
    L = ctx._L
    assert L.cfrk_fastq_parse_device(ctx._h, dev.d_text, len(raw), 0, dev.d_data, 64, dev.d_start, dev.d_length, 8, None, None) == ERR_ARG
    # empty text: sizes 0, nothing needed
    assert ctx.parse_fastq_device(0, 0, 0, 0, 0, 0, 0, 0) == (0, 0)
    # a data array that is not 16-byte aligned is fine
    for skew in (1, 3, 15):
        nN, nS = ctx.parse_fastq_device(dev.d_text, len(raw), 21, dev.d_data + skew, 64, dev.d_start, dev.d_length, 8)
        a = np.empty(nN, np.int8)
        ctx.sync()
        ctx.d2h(a, dev.d_data + skew)
        assert (nN, nS) == (5, 1) and a.tolist() == [0, 1, -1, 3, -1]


def test_an_open_global_job_is_unaffected(ctx, dev):
    rng = np.random.default_rng(12)
    genome = fc._seq(rng, 5000)
    reads = [genome[o:o + 100] for o in rng.integers(0, 4900, 400)]
    data = np.concatenate([np.append(fr._CODES[np.frombuffer(r, np.uint8)], np.int8(-1)) for r in reads])
    g = cfrk_amd.GlobalCounter(ctx, 21, cfrk_amd.CFRK_CANONICAL, 1 << 16)
    g.add(data)
    raw = fc.seam_cases()[0][1]
    rc, got, _ = dev.parse(raw, 20)
    assert rc == 0
    assert ctx.parse_fastq(raw, 20)[0].shape == got[0].shape
    g.add(data)
    digest = g.digest()
    want = cfrk_amd.GlobalCounter(ctx, 21, cfrk_amd.CFRK_CANONICAL, 1 << 16)
    want.add(np.concatenate([data, data]))
    assert digest == want.digest() and digest[0] > 1000


def test_host_form_and_python_wrapper(ctx):
    cases = fc.grammar_cases() + fc.seam_cases()[::3] + [(c[0], c[1]) for c in fc.refusal_cases()[::4]]
    for name, raw in cases:
        for q in (0, 20):
            want = fr.parse(raw, q)
            if want[0] != "ok":
                with pytest.raises(CfrkError, match=_message(raw, want[:2])) as e:
                    ctx.parse_fastq(raw, q)
                assert e.value.code == ERR_LAYOUT
                continue
            got = ctx.parse_fastq(raw if q else np.frombuffer(raw, np.uint8), q)
            _same_arrays(got, want[1:], f"{name} (min_qual {q})")


# ------------------------------------------------------------------ end to end

def _reads_fastq(n=3000, seed=9):
    """-> (FASTQ text, the FASTA text with every base below quality 20 replaced by N, the unmasked FASTA text)"""
    rng = np.random.default_rng(seed)
    genome = fc._seq(rng, 40000)
    parts = []
    for i in range(n):
        o, m = int(rng.integers(0, 39000)), int(rng.integers(30, 260))
        s = genome[o:o + m]
        q = rng.choice(np.frombuffer(b"#+5:?FI", np.uint8), len(s), p=[.03, .03, .04, .1, .2, .3, .3]).tobytes()
        parts.append(b"@read%d/1\n" % i + s + b"\n+\n" + q + b"\n")
    raw = b"".join(parts)
    return raw, fr.equivalent_fasta(raw, 20), fr.equivalent_fasta(raw, 0)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("fastq")
    raw, masked, plain = _reads_fastq()
    for name, text in (("reads.fastq", raw), ("masked.fasta", masked), ("plain.fasta", plain)):
        (d / name).write_bytes(text)
    return d


def _run(args, **kw):
    return subprocess.run([os.path.join(ROOT, "cfrk_amd", "cfrk")] + [str(a) for a in args], timeout=120, **kw)


def test_cli_global_counts_equal_those_of_the_masked_fasta(files):
    outs = {}
    for name, src, extra in (("fasta", "masked.fasta", []), ("fasta, device parse", "masked.fasta", ["--device-parse"]),
                             ("fastq", "reads.fastq", ["--min-qual", "20"]), ("fastq, device parse", "reads.fastq", ["--min-qual", "20", "--device-parse"]),
                             ("fastq, --format", "reads.fastq", ["--min-qual", "20", "--format", "fastq"])):
        out = files / "out.bin"
        _run([files / src, out, 31, "--global", "--canonical", "--binary"] + extra, check=True, stdout=subprocess.DEVNULL)
        outs[name] = out.read_bytes()
        out.unlink()
    assert len(outs["fasta"]) > 32 + 12 * 10000          # (a 40000-base genome: tens of thousands of distinct 31-mers)
    for name, b in outs.items():
        assert b == outs["fasta"], name
    # without --min-qual: the unmasked reads, another result
    out = files / "plain.bin"
    _run([files / "reads.fastq", out, 31, "--global", "--canonical", "--binary", "--device-parse"], check=True, stdout=subprocess.DEVNULL)
    want = files / "plain_fa.bin"
    _run([files / "plain.fasta", want, 31, "--global", "--canonical", "--binary"], check=True, stdout=subprocess.DEVNULL)
    assert out.read_bytes() == want.read_bytes() != outs["fasta"]


def test_cli_timing_reports_the_format(files):
    for src, extra, fmt in (("reads.fastq", ["--device-parse"], "fastq"), ("reads.fastq", [], "fastq"), ("masked.fasta", [], "fasta")):
        p = _run([files / src, files / "t.bin", 21, "--global", "--binary", "--timing"] + extra, check=True, capture_output=True, text=True)
        line = next(x for x in p.stderr.splitlines() if x.startswith("cfrk-timing "))
        assert json.loads(line[len("cfrk-timing "):])["format"] == fmt


def test_cli_takes_a_fastq_query_file(files):
    outs = []
    for q in ("plain.fasta", "reads.fastq"):
        out = files / "q.txt"
        _run([files / "masked.fasta", files / "c.bin", 21, "--global", "--canonical", "--binary", "--query", files / q, "--query-out", out],
             check=True, stdout=subprocess.DEVNULL)
        outs.append(out.read_bytes())
        out.unlink()
    assert outs[0] == outs[1] and outs[0].count(b"\n") >= 2999


def test_cli_native_and_sparse_take_fastq(files, tmp_path):
    small = b"".join((files / "reads.fastq").read_bytes().split(b"\n@read300/")[:1]) + b"\n"
    (tmp_path / "s.fastq").write_bytes(small)
    (tmp_path / "s.fasta").write_bytes(fr.equivalent_fasta(small, 20))
    for mode in (["3", "--native"], ["15", "--sparse"]):
        outs = []
        for src, extra in (("s.fasta", []), ("s.fastq", ["--min-qual", "20"])):
            out = tmp_path / "o.txt"
            _run([tmp_path / src, out] + mode + extra, check=True, stdout=subprocess.DEVNULL)
            outs.append(out.read_bytes())
        assert outs[0] and outs[0] == outs[1], mode


def test_cli_reports_a_refused_fastq_in_the_host_parsers_words(files, tmp_path):
    bad = tmp_path / "bad.fastq"
    bad.write_bytes(b"@a\nACGT\n+\nIIII\n@b\nACGT\n-\nIIII\n")
    res = [_run([bad, tmp_path / "o", 15, "--global"] + extra, capture_output=True, text=True) for extra in ([], ["--device-parse"])]
    assert res[0].returncode == res[1].returncode == 1
    assert "(FASTQ: line 6 does not begin with '+')" in res[0].stderr and "FASTQ: line 6 does not begin with '+' (byte offset 23)" in res[1].stderr


def test_parsed_reads_feed_the_counting_calls(ctx, dev):
    """Context.parse_fastq_device -> GlobalCounter.add_device and read_stats_device on the same buffers"""
    raw, _, _ = _reads_fastq(2000, seed=10)
    _, _, (data, start, length) = fc.host_parse(raw, 20)
    rc, got, msg = dev.parse(raw, 20)
    assert rc == 0, msg
    _same_arrays(got, (data, start, length), "reads")
    nN, nS = len(data), len(start)
    g = cfrk_amd.GlobalCounter(ctx, 31, cfrk_amd.CFRK_CANONICAL, 1 << 20)
    g.add(data, start, length)
    want = g.digest()
    want_rows = g.read_stats(data, start, length, 2)
    g = cfrk_amd.GlobalCounter(ctx, 31, cfrk_amd.CFRK_CANONICAL, 1 << 20)
    g.add_device(dev.d_data, nN)
    assert g.digest() == want and want[0] > 10000
    d_out = ctx.alloc(nS * 32)
    try:
        g.read_stats_device(dev.d_data, dev.d_start, dev.d_length, nN, nS, 2, d_out)
        rows = np.empty(nS, cfrk_amd.READ_STATS_DTYPE)
        ctx.sync()
        ctx.d2h(rows, d_out)
    finally:
        ctx.sync()
        ctx.free(d_out)
    assert (rows == want_rows).all() and rows["windows"].sum() > 0
