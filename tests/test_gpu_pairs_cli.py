"""GPU: the command line's --paired / --query2 / --filter-out2 / --filter-orphans / --correct-out2 / --pair-check against
the plain-Python references: tests/pair_ref.py for the pairing, filter_ref / text_out_ref / normalize_ref for what the
unpaired runs write.  The library's own calls are never the reference."""
import subprocess

import numpy as np
import pytest

from . import fastq_cases as fc
from . import filter_ref as fr
from . import ingest_cases as ic
from . import normalize_ref as nr
from . import pair_ref as pr
from . import text_out_ref as tr
from .test_gpu_filter import _noisy_reads
from .test_gpu_query import _cli, _oracle

pytestmark = pytest.mark.gpu

COUNT_MAX = 0xFFFFFFFE
K = 21
LETTERS = np.frombuffer(b"ACGT", np.uint8)


def _fastq(seqs, names, rng):
    return b"".join(b"@" + n + b"\n" + s + b"\n+\n" + fc._qual(rng, len(s), 33, 127) + b"\n" for s, n in zip(seqs, names))


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """a counted FASTA file and 160 pairs of noisy query reads: as one interleaved FASTQ file and as two files; the
    spans and the survival of every read by the references"""
    d = tmp_path_factory.mktemp("pairs_cli")
    rng = np.random.default_rng(4242)
    genome = rng.integers(0, 4, 8000).astype(np.int8)
    fa = d / "g.fasta"
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, LETTERS[r].tobytes()) for i, r in enumerate(_noisy_reads(rng, genome, 1200, 60, 220, 0.0))))
    seqs = [LETTERS[r].tobytes() for r in _noisy_reads(rng, genome, 320, 15, 120, 0.05)]
    seqs[6], seqs[11], seqs[40] = b"ACGT", seqs[11][:K - 1], seqs[40][:50] + b"N" + seqs[40][50:]
    # every third pair is named in the Casava-1.8 style, the others by /1 and /2
    names = [b"pair%d %d:N:0:ACGT" % (i // 2, i % 2 + 1) if (i // 2) % 3 == 0 else b"pair%d/%d" % (i // 2, i % 2 + 1) for i in range(len(seqs))]
    both = _fastq(seqs, names, rng)
    rc, _, (qd, qst, qln) = fc.host_parse(both, 0)
    assert rc == 0 and len(qln) == len(seqs)
    rec = tr.index_ref(both, tr.TEXT_FASTQ)
    assert pr.check_pairs(both, rec[0::2], both, rec[1::2]) == (-1, 0)
    creads = ic.host_parse(fa.read_bytes(), ic.NATIVE)[1]
    counts, valid = fr.window_counts(qd, K, True, _oracle(creads[0], K, True))
    spans = fr.ref_spans(qd, qst, qln, K, 2, COUNT_MAX, fr.SPAN_LONGEST, counts, valid)
    sv = pr.survive_all(len(seqs), None, spans, qln, K)
    pair, oa, ob, pc = pr.join(sv[0::2], sv[1::2], pr.BOTH)
    assert pc[0] > 10 and pc[1] > 10 and pc[2] > 10 and pc[3] > 2, pc
    qi = d / "q.fastq"
    qi.write_bytes(both)
    recs = [both[int(r["head_off"]):int(e)] for r, e in zip(rec, list(rec["head_off"][1:]) + [len(both)])]
    q1, q2 = d / "q_1.fastq", d / "q_2.fastq"
    q1.write_bytes(b"".join(recs[0::2]))
    q2.write_bytes(b"".join(recs[1::2]))
    return dict(dir=d, fa=fa, qi=qi, q1=q1, q2=q2, both=both, rec=rec, qd=qd, qst=qst, qln=qln, spans=spans, pair=pair, oa=oa, ob=ob, pc=pc,
                recs=recs, seqs=seqs)


def _records(text):
    """the four-line records of a FASTQ text"""
    lines = text.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    return [b"\n".join(lines[i:i + 4]) + b"\n" for i in range(0, len(lines) - 1, 4)]


def _base(w, out="none.cfrk"):
    return [_cli(), str(w["fa"]), str(w["dir"] / out), str(K), "--global", "--canonical", "--query-only"]


def test_interleaved_fastq_through_the_filter(world):
    w, d = world, world["dir"]
    f, o, plain = d / "f.fq", d / "o.fq", d / "plain.fq"
    run = _base(w) + ["--query", str(w["qi"]), "--filter-format", "fastq"]
    r = subprocess.run(run + ["--filter-out", str(f), "--paired", "--filter-orphans", str(o)], check=True, timeout=300, stderr=subprocess.PIPE)
    subprocess.run(run + ["--filter-out", str(plain)], check=True, timeout=300)
    keep2 = np.repeat(w["pair"], 2)
    orphan = np.zeros(len(keep2), np.uint8)
    orphan[0::2], orphan[1::2] = w["oa"], w["ob"]
    emit = lambda keep: tr.emit_ref(w["qd"], w["qst"], w["qln"], w["both"], w["rec"], w["spans"], keep, K, tr.TEXT_FASTQ)[0]
    got_f, got_o = f.read_bytes(), o.read_bytes()
    assert got_f == emit(keep2) and got_o == emit(orphan)
    recs_f, recs_o = _records(got_f), _records(got_o)
    assert len(recs_f) % 2 == 0 and len(recs_f) == 2 * w["pc"][0] and len(recs_o) == w["pc"][1] + w["pc"][2]
    idx = tr.index_ref(got_f, tr.TEXT_FASTQ)
    assert pr.check_pairs(got_f, idx[0::2], got_f, idx[1::2]) == (-1, 0)
    # FFILE and OFILE together hold exactly the reads the unpaired run writes
    unpaired = _records(plain.read_bytes())
    assert plain.read_bytes() == emit(None) and sorted(recs_f + recs_o) == sorted(unpaired) and len(set(unpaired)) == len(unpaired)
    assert (b"%d pairs kept, %d orphans (%d + %d) written, %d pairs dropped" % (w["pc"][0], w["pc"][1] + w["pc"][2], w["pc"][1], w["pc"][2], w["pc"][3])) in r.stderr
    # without OFILE the orphans are dropped and still counted; FASTA by number goes through the select
    f2 = d / "f2.fa"
    r = subprocess.run(_base(w) + ["--query", str(w["qi"]), "--filter-out", str(f2), "--paired"], check=True, timeout=300, stderr=subprocess.PIPE)
    assert f2.read_bytes() == fr.fasta_text(*fr.ref_select(w["qd"], w["qst"], w["qln"], w["spans"], keep2, K))
    assert b"orphans (%d + %d) dropped" % (w["pc"][1], w["pc"][2]) in r.stderr
    # the median keep bytes are an input of the join
    f3, o3, p3 = d / "f3.fq", d / "o3.fq", d / "p3.fq"
    subprocess.run(run + ["--filter-out", str(f3), "--paired", "--filter-orphans", str(o3), "--filter-min-median", "3"], check=True, timeout=300)
    subprocess.run(run + ["--filter-out", str(p3), "--filter-min-median", "3"], check=True, timeout=300)
    r3, ro3 = _records(f3.read_bytes()), _records(o3.read_bytes())
    assert sorted(r3 + ro3) == sorted(_records(p3.read_bytes())) and len(r3) % 2 == 0 and 0 < len(r3) <= len(recs_f)
    i3 = tr.index_ref(f3.read_bytes(), tr.TEXT_FASTQ)
    assert pr.check_pairs(f3.read_bytes(), i3[0::2], f3.read_bytes(), i3[1::2]) == (-1, 0)


def test_two_files_through_the_filter(world):
    w, d = world, world["dir"]
    f1, f2, o = d / "s1.fq", d / "s2.fq", d / "so.fq"
    subprocess.run(_base(w) + ["--query", str(w["q1"]), "--query2", str(w["q2"]), "--filter-format", "fastq", "--filter-out", str(f1),
                               "--filter-out2", str(f2), "--filter-orphans", str(o)], check=True, timeout=300)
    t1, t2 = w["q1"].read_bytes(), w["q2"].read_bytes()

    def emit(text, half, keep):
        rc, _, (qd, qst, qln) = fc.host_parse(text, 0)
        assert rc == 0
        return tr.emit_ref(qd, qst, qln, text, tr.index_ref(text, tr.TEXT_FASTQ), w["spans"][half::2], keep, K, tr.TEXT_FASTQ)[0]

    assert f1.read_bytes() == emit(t1, 0, w["pair"]) and f2.read_bytes() == emit(t2, 1, w["pair"])
    assert o.read_bytes() == emit(t1, 0, w["oa"]) + emit(t2, 1, w["ob"])
    r1, r2 = _records(f1.read_bytes()), _records(f2.read_bytes())
    assert len(r1) == len(r2) == w["pc"][0]
    i1, i2 = tr.index_ref(f1.read_bytes(), tr.TEXT_FASTQ), tr.index_ref(f2.read_bytes(), tr.TEXT_FASTQ)
    assert pr.check_pairs(f1.read_bytes(), i1, f2.read_bytes(), i2) == (-1, 0)
    assert sorted(r1 + r2 + _records(o.read_bytes())) == sorted(_records(emit(t1, 0, None)) + _records(emit(t2, 1, None)))


def test_correct_out_checks_the_pairing_only(world):
    w, d = world, world["dir"]
    base = _base(w) + ["--correct-min-count", "2", "--correct-format", "fastq"]
    c0, c1 = d / "c0.fq", d / "c1.fq"
    subprocess.run(base + ["--query", str(w["qi"]), "--correct-out", str(c0)], check=True, timeout=300)
    subprocess.run(base + ["--query", str(w["qi"]), "--correct-out", str(c1), "--paired"], check=True, timeout=300)
    assert c1.read_bytes() == c0.read_bytes() and len(_records(c0.read_bytes())) == len(w["recs"])
    # a planted mismatch: the mate of pair 17 gets another pair's name
    recs = list(w["recs"])
    head = recs[35].split(b"\n", 1)
    recs[35] = b"@pair99/2\n" + head[1]
    recs[80] = b"@" + recs[80][2:]                                 # ... and pair 40's first mate loses a byte
    bad = d / "bad.fastq"
    bad.write_bytes(b"".join(recs))
    c2 = d / "c2.fq"
    r = subprocess.run(base + ["--query", str(bad), "--correct-out", str(c2), "--paired"], stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 1 and not c2.exists()
    assert b"pair 17" in r.stderr and recs[34].split(b"\n")[0] in r.stderr and b"@pair99/2" in r.stderr and b"2 pair(s)" in r.stderr
    subprocess.run(base + ["--query", str(bad), "--correct-out", str(c2), "--paired", "--pair-check", "off"], check=True, timeout=300)
    assert len(_records(c2.read_bytes())) == len(recs)
    # two files: each to its own output; the names are checked across the files
    c3, c4, rep = d / "c3.fq", d / "c4.fq", d / "rep.txt"
    subprocess.run(base + ["--query", str(w["q1"]), "--query2", str(w["q2"]), "--correct-out", str(c3), "--correct-out2", str(c4),
                           "--correct-report", str(rep)], check=True, timeout=300)
    both = _records(c0.read_bytes())
    assert _records(c3.read_bytes()) == both[0::2] and _records(c4.read_bytes()) == both[1::2]
    assert len(rep.read_bytes().split(b"\n")) - 1 == len(both)
    b2 = d / "bad_2.fastq"
    b2.write_bytes(b"".join(recs[1::2]))
    r = subprocess.run(base + ["--query", str(w["q1"]), "--query2", str(b2), "--correct-out", str(c3), "--correct-out2", str(c4)],
                       stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 1 and b"pair 17" in r.stderr and b"bad_2.fastq" in r.stderr and b"q_1.fastq" in r.stderr


@pytest.fixture(scope="module")
def norm_world(tmp_path_factory):
    """120 interleaved pairs at coverage ~ 18 of a 2 kb genome, a few mates of Ns only or too short for a window"""
    d = tmp_path_factory.mktemp("pairs_cli_norm")
    rng = np.random.default_rng(99)
    genome = rng.integers(0, 4, 2000).astype(np.int8)
    seqs = []
    for j in range(120):
        for m in range(2):
            L = 150 if (j, m) not in ((5, 1), (40, 0)) else 12
            p = int(rng.integers(0, len(genome) - L))
            r = genome[p:p + L]
            seqs.append(LETTERS[r if rng.integers(0, 2) else (3 - r[::-1])].tobytes())
    seqs[21], seqs[60] = b"N" * 150, b"N" * 90
    names = [b"frag%d/%d" % (i // 2, i % 2 + 1) for i in range(len(seqs))]
    records = [b"@" + n + b"\n" + s + b"\n+\n" + fc._qual(rng, len(s), 35, 74) + b"\n" for s, n in zip(seqs, names)]
    fq = d / "in.fastq"
    fq.write_bytes(b"".join(records))
    rc, _, (data, start, length) = fc.host_parse(fq.read_bytes(), 0)
    assert rc == 0
    keys = nr.all_read_keys(data, start, length, K, True)
    return dict(dir=d, fq=fq, records=records, seqs=seqs, keys=keys)


@pytest.mark.parametrize("mode", ["either", "both", None])
def test_normalize_out_paired(norm_world, mode):
    from .test_gpu_spectrum import _read_glb1
    w, d = norm_world, norm_world["dir"]
    cutoff, batch = 4, 16
    m = pr.BOTH if mode == "both" else pr.EITHER
    want = pr.normalize_pairs_keys(w["keys"], cutoff, batch, m)
    assert 0 < want[1] < len(w["records"]) and want[1] % 2 == 0
    nf, out = d / f"kept_{mode}.fastq", d / f"out_{mode}.bin"
    cmd = [_cli(), str(w["fq"]), str(out), str(K), "--global", "--canonical", "--binary", "--normalize-cutoff", str(cutoff), "--normalize-batch", str(batch),
           "--normalize-out", str(nf), "--paired", "--normalize-format", "fastq"] + (["--pair-mode", mode] if mode else [])
    subprocess.run(cmd, check=True, timeout=300)
    assert nf.read_bytes() == b"".join(r for r, kp in zip(w["records"], want[0]) if kp)
    wlo, _, wcnt = nr.export_arrays(want[2])
    rec = _read_glb1(out.read_bytes())
    assert (rec["lo"] == wlo).all() and (rec["c"] == wcnt).all()
    if mode is None:
        empty = np.array([len(x) == 0 for x in w["keys"]])
        assert want[0][empty].any()
        # an odd number of records, and a name that does not match
        odd = d / "odd.fastq"
        odd.write_bytes(b"".join(w["records"][:-1]))
        r = subprocess.run([c if c != str(w["fq"]) else str(odd) for c in cmd], stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 1 and b"odd.fastq holds 239 records" in r.stderr
        recs = list(w["records"])
        recs[7] = b"@other/2\n" + recs[7].split(b"\n", 1)[1]
        bad = d / "bad.fastq"
        bad.write_bytes(b"".join(recs))
        r = subprocess.run([c if c != str(w["fq"]) else str(bad) for c in cmd], stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 1 and b"pair 3" in r.stderr and b"@frag3/1" in r.stderr and b"@other/2" in r.stderr
        subprocess.run([c if c != str(w["fq"]) else str(bad) for c in cmd] + ["--pair-check", "off"], check=True, timeout=300)
        assert len(_records(nf.read_bytes())) == want[1]


def test_without_the_new_options_the_files_are_the_parents(world, norm_world):
    """one filter run and one normalise run, expected bytes from the references of the merged features"""
    w, d = world, world["dir"]
    f = d / "numbered.fa"
    subprocess.run(_base(w) + ["--query", str(w["qi"]), "--filter-out", str(f)], check=True, timeout=300)
    assert f.read_bytes() == fr.fasta_text(*fr.ref_select(w["qd"], w["qst"], w["qln"], w["spans"], None, K))
    n, nd = norm_world, norm_world["dir"]
    want = nr.normalize_keys(n["keys"], 4, 16)
    nf = nd / "plain_kept.fa"
    subprocess.run([_cli(), str(n["fq"]), str(nd / "plain.bin"), str(K), "--global", "--canonical", "--binary", "--normalize-cutoff", "4",
                    "--normalize-batch", "16", "--normalize-out", str(nf)], check=True, timeout=300)
    assert nf.read_bytes() == b"".join(b">%d\n%s\n" % (i, s) for i, (s, kp) in enumerate(zip(n["seqs"], want[0])) if kp)
    assert (want[0][0::2] != want[0][1::2]).any(), "the unpaired rule never splits a pair here: the paired test shows nothing"
