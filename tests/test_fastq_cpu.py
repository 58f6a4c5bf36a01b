"""The host FASTQ parser (cfrk_host_parse_fastq, cfrk_amd/host/cfrk_host.cpp) against two yardsticks that are not it:
the plain-Python restatement of the grammar (tests/fastq_ref.py) and, for valid texts, the host FASTA parser on the
equivalent FASTA text (every base below min_qual replaced by N).  Cause and place of every refusal, the same result
with 1, 3 and 16 parse threads, the format sniffer, and the CLI's refusals that need no device."""
import os
import subprocess

import numpy as np
import pytest

from . import fastq_cases as fc
from . import fastq_ref as fr

ROOT = fc.ROOT
THREADS = (1, 3, 16)


@pytest.fixture(scope="module", autouse=True)
def host():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host"), "../libcfrk_host.so"], stdout=subprocess.DEVNULL)
    return fc.host_lib()


@pytest.fixture(scope="module")
def cli():
    import cfrk_amd
    if not os.path.exists(cfrk_amd.library_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "cfrk_amd", "cfrk")


def _same_arrays(got, want, what):
    for name, g, w in zip(("data", "start", "length"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name} has {g.size} entries, expected {w.size}"
        if not (g == w).all():
            j = int(np.flatnonzero(g != w)[0])
            raise AssertionError(f"{what}: {name}[{j}] = {g[j]}, expected {w[j]}")


def _held(raw, what, min_quals=fc.MIN_QUALS, threads=THREADS):
    for q in min_quals:
        want = fr.parse(raw, q)
        for thr in threads:
            rc, where, got = fc.host_parse(raw, q, thr)
            tag = f"{what} (min_qual {q}, {thr} threads)"
            if want[0] != "ok":
                assert rc != 0 and (fc.CAUSES.get(rc), where) == want, f"{tag}: rc {rc} where {where}, expected {want}"
                continue
            assert rc == 0, f"{tag}: rc {rc} where {where}"
            _same_arrays(got, want[1:], tag)
        if want[0] == "ok":
            frc, fasta = fc.host_parse_fasta(fr.equivalent_fasta(raw, q), 0)
            assert frc == 0
            _same_arrays(want[1:], fasta, f"{what} (min_qual {q}): the restatement against the FASTA parser")


@pytest.mark.parametrize("case", fc.grammar_cases(), ids=lambda c: c[0])
def test_grammar(case):
    _held(case[1], case[0])


def test_grammar_cases_say_what_their_names_say():
    verdicts = {name: fr.parse(raw)[:2] for name, raw in fc.grammar_cases()}
    refused = {n: v for n, v in verdicts.items() if v[0] != "ok"}
    assert refused == {"a final empty quality line without its newline: three lines": ("truncated", 3),
                       "a single '@'": ("truncated", 1), "a single newline": ("no_at", 0)}
    _, data, start, length = fr.parse(b"@a\nACGTACGT\n+\nIIII!!5I", 20)
    assert data.tolist() == [0, 1, 2, 3, -1, -1, 2, 3, -1] and start.tolist() == [0] and length.tolist() == [8]
    _, data, start, length = fr.parse(b"@a\n\n+\n\n@b\nAC\n+\nI5\n@c\n\n+\n\n", 21)
    assert data.tolist() == [-1, 0, -1, -1, -1] and start.tolist() == [0, 1, 4] and length.tolist() == [0, 2, 0]
    # min_qual 0 masks nothing, bytes below 33 included; min_qual 1 masks exactly those; 0x80 and 0xFF never mask
    raw = dict(fc.grammar_cases())["quality bytes below 33 and 0xFF"]
    assert fr.parse(raw, 0)[1].tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 0, 1, -1]
    assert fr.parse(raw, 1)[1].tolist() == [-1, -1, -1, -1, -1, 1, 2, 3, 0, 1, -1]
    assert fr.parse(raw, 93)[1].tolist() == [-1, -1, -1, -1, -1, 1, 2, 3, -1, -1, -1]


@pytest.mark.parametrize("case", fc.refusal_cases(), ids=lambda c: c[0])
def test_refusals_name_cause_and_place(case):
    name, raw, cause, where = case
    assert fr.parse(raw)[:2] == (cause, where), "the restatement and the case disagree"
    for thr in THREADS:
        for q in (0, 20):
            rc, got_where, arrays = fc.host_parse(raw, q, thr)
            assert arrays is None and (fc.CAUSES.get(rc), got_where) == (cause, where), f"{name} ({thr} threads): rc {rc}, where {got_where}"


@pytest.mark.parametrize("case", fc.seam_cases(), ids=lambda c: c[0])
def test_tile_seams(case):
    assert fr.parse(case[1])[0] == "ok"
    _held(case[1], case[0])


def test_random_texts():
    verdicts = set()
    for i, raw in enumerate(fc.random_texts()):
        verdicts.add(fr.parse(raw)[0])
        _held(raw, f"random text {i}", threads=(1, 3) if i % 2 else (16,))
    assert verdicts == {"ok", "no_at", "no_plus", "truncated", "lengths"}


def test_more_than_one_block_of_the_tile_scan():
    raw = fc.scan_block_case()
    assert len(raw) > fc.SCAN_TILES * fc.T
    _held(raw, "scan blocks", min_quals=(20,), threads=(1, 16))
    # the default thread count (this text is large enough to be threaded without being told to)
    rc, _, got = fc.host_parse(raw, 20, 0)
    assert rc == 0
    _same_arrays(got, fr.parse(raw, 20)[1:], "scan blocks, default threads")


def test_min_qual_outside_its_range(host):
    for q in (-1, 94, 1000):
        rc, where, arrays = fc.host_parse(b"@a\nA\n+\nI\n", q)
        assert (rc, arrays) == (fc.MIN_QUAL, None) and fr.parse(b"@a\nA\n+\nI\n", q) == ("min_qual", 0)
    assert fc.host_parse(b"@a\nA\n+\nI\n", 93)[0] == 0


def test_messages(host):
    buf = fc.C.create_string_buffer(200)
    texts = {}
    for rc in fc.CAUSES:
        n = host.cfrk_host_fastq_message(rc, 12, buf, 200)
        assert n == len(buf.value) > 0
        texts[rc] = buf.value.decode()
    assert texts[fc.NO_AT] == "FASTQ: line 12 does not begin with '@'" and texts[fc.NO_PLUS] == "FASTQ: line 12 does not begin with '+'"
    assert texts[fc.TRUNCATED] == "FASTQ: 12 lines, not a multiple of four"
    assert texts[fc.LENGTHS] == "FASTQ: record 12 has sequence and quality lines of different lengths"
    assert host.cfrk_host_fastq_message(0, 0, buf, 200) == 0 and host.cfrk_host_fastq_message(-1, 0, buf, 200) == 0


def test_sniffer(host):
    FASTA, FASTQ = 0, 1
    for raw, want in ((b"", FASTA), (b"@", FASTQ), (b"@r\nA\n+\nI\n", FASTQ), (b">r\nA\n", FASTA), (b"\n@r\n", FASTA), (b"A", FASTA), (b"+", FASTA)):
        assert host.cfrk_host_sniff_format(raw, len(raw)) == want, raw


def test_read_fastq_reads_a_file(host, tmp_path):
    raw = fc.seam_cases()[0][1]
    p = tmp_path / "reads.fastq"
    p.write_bytes(raw)
    b, where = fc.Batch(), fc.C.c_uint64()
    assert host.cfrk_host_read_fastq(str(p).encode(), 20, fc.C.byref(b), fc.C.byref(where)) == 0
    _same_arrays(fc._take(host, b), fr.parse(raw, 20)[1:], "cfrk_host_read_fastq")
    assert host.cfrk_host_read_fastq(str(tmp_path / "missing").encode(), 0, fc.C.byref(b), None) == -1
    (tmp_path / "bad.fastq").write_bytes(b"@a\nAC\n+\nI\n")
    assert host.cfrk_host_read_fastq(str(tmp_path / "bad.fastq").encode(), 0, fc.C.byref(b), fc.C.byref(where)) == fc.LENGTHS and where.value == 0


FASTQ_TEXT = b"@a\nACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIII\n"
FASTA_TEXT = b">a\nACGTACGTACGTACGTACGT\n"


@pytest.mark.parametrize("text, args, msg", [
    (FASTQ_TEXT, [], b"is FASTQ: the default per-read mode is the reference's, which reads FASTA only; FASTQ is taken by --native, --global and --sparse"),
    (FASTQ_TEXT, ["--all-chunks"], b"FASTQ is taken by --native, --global and --sparse"),
    (FASTA_TEXT, ["--format", "fastq"], b"FASTQ is taken by --native, --global and --sparse"),
    (FASTA_TEXT, ["--global", "--min-qual", "20"], b"--min-qual applies to FASTQ input"),
    (FASTQ_TEXT, ["--global", "--format", "fasta", "--min-qual", "20"], b"--min-qual applies to FASTQ input"),
    (b"", ["--global", "--min-qual", "20"], b"--min-qual applies to FASTQ input"),
    (FASTQ_TEXT, ["--global", "--min-qual", "94"], b"--min-qual needs an integer from 0 to 93"),
    (FASTQ_TEXT, ["--global", "--min-qual", "-1"], b"--min-qual needs an integer from 0 to 93"),
    (FASTQ_TEXT, ["--global", "--min-qual", "2x"], b"--min-qual needs an integer from 0 to 93"),
    (FASTQ_TEXT, ["--global", "--format", "sam"], b"--format takes fasta, fastq or auto"),
])
def test_cli_refuses_before_a_device_is_opened(cli, tmp_path, text, args, msg):
    """one line on stderr, status 1, no output file: the format is known from the first byte, nothing is parsed"""
    src, out = tmp_path / "in.txt", tmp_path / "out.txt"
    src.write_bytes(text)
    p = subprocess.run([cli, str(src), str(out), "15"] + args, cwd=tmp_path, capture_output=True, timeout=60)
    assert p.returncode == 1 and msg in p.stderr and p.stderr.count(b"\n") == 1
    assert not out.exists()
