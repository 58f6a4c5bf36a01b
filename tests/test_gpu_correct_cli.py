"""GPU: the CLI's --correct-out against tests/correct_ref.py: after a --global count and after --query-db, FASTA in with
FASTA out (records named by number, or by QFILE's names), FASTQ in with FASTQ out (names kept, quality lines byte for
byte), and the --correct-report file.  The expected text is the reference's corrected buffer written by the restated
writers of tests/filter_ref.py and tests/text_out_ref.py.  (The refusals are raised before a device is opened and are
in tests/test_correct_cpu.py.)"""
import subprocess

import numpy as np
import pytest

from . import correct_ref as cr
from . import fastq_cases as fc
from . import filter_ref as fr
from . import ingest_cases as ic
from . import text_out_ref as tr
from .test_gpu_query import _cli
from .test_gpu_text_out import _fastq_of

pytestmark = pytest.mark.gpu

LETTERS = np.frombuffer(b"ACGT", np.uint8)


def test_cli_correct(tmp_path):
    cli = _cli()
    k, mn = 31, 2
    rng = np.random.default_rng(3301)
    genome = rng.integers(0, 4, 6000).astype(np.int8)
    fa = tmp_path / "g.fasta"
    fa.write_bytes(b">g1\n%s\n>g2\n%s\n" % (LETTERS[genome].tobytes(), LETTERS[genome].tobytes()))
    counts = cr.count_reads(*cr.flatten([genome, genome]), k, True)
    qs = []
    for i in range(120):
        L = int(rng.integers(40, 400))
        a = int(rng.integers(0, len(genome) - L))
        r = genome[a:a + L].copy()
        if i % 2:
            r = cr.revcomp(r)
        for p in np.nonzero(rng.random(L) < 0.01)[0]:
            r = cr.substitute(r, int(p), rng)
        qs.append(LETTERS[r].tobytes())
    qs += [b"ACGT", qs[0][:k - 1], qs[1][:40] + b"N" + qs[1][40:], qs[2].lower(), LETTERS[genome[:3000]].tobytes()]
    names = [b"q%d extra words" % i for i in range(len(qs))]
    fq_text = _fastq_of(qs, names, rng)
    fa_text = b"".join(b">" + n + b"\n" + s + b"\n" for s, n in zip(qs, names))
    qfq, qfa = tmp_path / "q.fastq", tmp_path / "q.fasta"
    qfq.write_bytes(fq_text)
    qfa.write_bytes(fa_text)
    rc, _, (qd, qst, qln) = fc.host_parse(fq_text, 0)
    assert rc == 0
    fixed_data, fix = cr.correct(qd, qst, qln, k, True, counts, mn)
    assert fix["fixed"].sum() > 150 and fix["left"].sum() > 20 and (fixed_data != qd).sum() == fix["fixed"].sum()
    rec_q, rec_a = tr.index_ref(fq_text, tr.TEXT_FASTQ), tr.index_ref(fa_text, tr.TEXT_FASTA)
    numbered = fr.fasta_text(fixed_data, qst, qln, np.arange(len(qst), dtype=np.int64))
    named = tr.emit_ref(fixed_data, qst, qln, fa_text, rec_a, None, None, 0, tr.TEXT_FASTA)[0]
    as_fastq = tr.emit_ref(fixed_data, qst, qln, fq_text, rec_q, None, None, 0, tr.TEXT_FASTQ)[0]
    assert numbered.count(b">") == len(qs) == as_fastq.count(b"\n") // 4                      # ALL reads are written
    report = b"".join(b"%d\t%d\n" % (f, l) for f, l in fix.tolist())

    glob = [cli, str(fa), str(tmp_path / "none.cfrk"), str(k), "--global", "--canonical", "--query-only"]
    full = tmp_path / "full.bin"
    subprocess.run([cli, str(fa), str(full), str(k), "--global", "--canonical", "--binary"], check=True, timeout=300)
    db = [cli, "--query-db", str(full)]

    def run(base, q, out, *more):
        subprocess.run(base + ["--query", str(q), "--correct-out", str(out), "--correct-min-count", str(mn)] + list(more),
                       check=True, timeout=300)
        return out.read_bytes()

    for tag, base in (("g", glob), ("d", db)):
        rep = tmp_path / (tag + "_report.txt")
        assert run(base, qfa, tmp_path / (tag + "1.fa"), "--correct-report", str(rep)) == numbered
        assert rep.read_bytes() == report
        assert run(base, qfq, tmp_path / (tag + "2.fa")) == numbered                         # FASTQ in, FASTA by number
        assert run(base, qfa, tmp_path / (tag + "3.fa"), "--correct-names") == named
        assert run(base, qfq, tmp_path / (tag + "4.fa"), "--correct-names", "--correct-format", "fasta") == named
        assert run(base, qfq, tmp_path / (tag + "5.fq"), "--correct-format", "fastq") == as_fastq
    # the quality lines are QFILE's, byte for byte
    assert as_fastq.split(b"\n")[3::4] == [fq_text[r["qual_off"]:r["qual_off"] + r["qual_len"]] for r in rec_q]
    assert not (tmp_path / "none.cfrk").exists()
    # min_count 0: the reads as they are
    same = fr.fasta_text(qd, qst, qln, np.arange(len(qst), dtype=np.int64))
    out0 = tmp_path / "same.fa"
    subprocess.run(glob + ["--query", str(qfa), "--correct-out", str(out0), "--correct-min-count", "0"], check=True, timeout=300)
    assert out0.read_bytes() == same
