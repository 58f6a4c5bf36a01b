"""CPU-side checks of the graph mask and the tip rule: the C ABI declares and exports the calls, the bound of ratio_q8 is
documented and mirrored; the plain-Python reference of tests/tips_ref.py gives the hand-worked answers on graphs small
enough to draw, and keeps its invariants on random inputs (tips are candidates, the mirror symmetry, the clip loop
ends); the CLI's refusals; the kernels of unitig_tips.hip and unitig_mask.hip use no scratch memory."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from . import tips_ref as tr
from . import unitig_ref as ur
from .test_kernel_resources import CSRC, HIPCC, ROOT, _functions
from .test_unitigs_cpu import _random_input

NEW_CALLS = ("cfrk_global_mask_keys", "cfrk_global_mask_keys_device", "cfrk_global_mask_unitigs", "cfrk_global_mask_unitigs_device",
             "cfrk_global_mask_clear", "cfrk_global_mask_count", "cfrk_global_unitig_tips", "cfrk_global_unitig_tips_device")


@pytest.fixture(scope="module")
def built():
    import cfrk_amd
    if not os.path.exists(cfrk_amd.library_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return cfrk_amd


@pytest.fixture(scope="module")
def cli(built):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "cfrk_amd", "cfrk")


def test_abi_declares_and_exports_the_mask_and_tip_calls(built):
    syms = built.abi_symbols()
    L = C.CDLL(built.library_path())
    for s in NEW_CALLS:
        assert s in syms
        assert hasattr(L, s)
    header = open(os.path.join(ROOT, "include", "cfrk_abi.h")).read()
    m = re.search(r"#define CFRK_TIP_RATIO_Q8_MAX\s+(\d+)\b", header)
    assert m and int(m.group(1)) == built.CFRK_TIP_RATIO_Q8_MAX == tr.RATIO_Q8_MAX == 65536
    assert re.search(r"ratio_q8 > CFRK_TIP_RATIO_Q8_MAX \(65536\) is CFRK_ERR_ARG", header)      # the bound is documented
    assert "that are not masked" in header
    for name in ("mask_keys", "mask_unitigs", "mask_clear", "mask_count", "unitig_tips", "clip_tips"):
        assert callable(getattr(built.GlobalCounter, name))
    for name in ("mask_keys_device", "mask_unitigs_device", "unitig_tips_device"):
        assert callable(getattr(built.GlobalCounter, name))


# ------------------------------------------------------------------ the reference on graphs one can draw

def _table(seqs, k, canonical):
    table = {}
    for s, t in seqs:
        ur.count_kmers([s], k, canonical, t, table)
    return table


def _tip_seqs(seqs, k, canonical, max_kmers, ratio_q8):
    table = _table(seqs, k, canonical)
    units, link_ptr, links = tr.graph(table, k, canonical)
    tip = tr.tips(units, link_ptr, links, canonical, max_kmers, ratio_q8)
    return [u[0] for u in units], sorted(units[j][0] for j in np.flatnonzero(tip))


CHAIN = "AACCGGTATCT"       # k = 4: AACC ACCG CCGG CGGT GGTA GTAT TATC ATCT, no 3-mer twice


def test_right_and_left_tip_on_a_chain():
    """k = 4, plain strands, the chain counted twice, the branches once, max_kmers 2:

        GACC \\                       / GGTC - GTCA
               ACCG - CCGG - CGGT  <
        AACC /                       \\ GGTA - GTAT - TATC - ATCT

    GGTCA hangs off CGGT beside the chain's continuation GGTATCT (4 k-mers: no candidate): a right tip.  GACC enters
    ACCG beside AACC; both are candidates (one k-mer, the left end dead), AACC has the higher mean (2 against 1) and
    stays: a left tip, and the fork at the chain's very beginning keeps one arm."""
    units, tips = _tip_seqs([(CHAIN, 2), ("CGGTCA", 1), ("GACCGG", 1)], 4, False, 2, 0)
    assert units == ["AACC", "ACCGGT", "GACC", "GGTATCT", "GGTCA"]
    assert tips == ["GACC", "GGTCA"]
    assert _tip_seqs([(CHAIN, 2), ("CGGTCA", 1), ("GACCGG", 1)], 4, False, 2, 512)[1] == ["GACC", "GGTCA"]


def test_two_tips_on_one_anchor_end():
    """AACCGGT (4 k-mers, counted 3 times) ends in a fork of GGTAT and GGTCA and nothing else.  Counted 2 and 1: the lower
    mean goes.  Counted 1 and 1: the means tie and the higher index goes, GGTCA again (the list ascends by first
    k-mer).  One arm always stays."""
    for t in (2, 1):
        units, tips = _tip_seqs([("AACCGGT", 3), ("CGGTAT", t), ("CGGTCA", 1)], 4, False, 2, 0)
        assert units == ["AACCGGT", "GGTAT", "GGTCA"]
        assert tips == ["GGTCA"]
    # the other way round: the lower mean goes, not the higher index
    assert _tip_seqs([("AACCGGT", 3), ("CGGTAT", 1), ("CGGTCA", 2)], 4, False, 2, 0)[1] == ["GGTAT"]
    # asked for twice the coverage, neither arm is beaten by the other at 2 : 1 ... but exactly twice is enough
    assert _tip_seqs([("AACCGGT", 3), ("CGGTAT", 2), ("CGGTCA", 1)], 4, False, 2, 512)[1] == ["GGTCA"]
    assert _tip_seqs([("AACCGGT", 3), ("CGGTAT", 2), ("CGGTCA", 1)], 4, False, 2, 513)[1] == []


def test_what_stays():
    """a tip longer than max_kmers; a bubble (both branches rejoin: no dead end); an isolated k-mer (both ends dead)"""
    units, tips = _tip_seqs([(CHAIN, 2), ("CGGTCAG", 1)], 4, False, 2, 0)
    assert "GGTCAG" in units and tips == []
    assert _tip_seqs([(CHAIN, 2), ("CGGTCAG", 1)], 4, False, 3, 0)[1] == ["GGTCAG"]
    units, tips = _tip_seqs([(CHAIN, 2), ("CCGGAATC", 1)], 4, False, 4, 0)      # CGGT GGTA GTAT TATC | CGGA GGAA GAAT AATC
    assert "CGGAATC" in units and "CGGTATC" in units and tips == []
    units, tips = _tip_seqs([(CHAIN, 2), ("TTTG", 1)], 4, False, 4, 0)
    assert units == [CHAIN, "TTTG"] and tips == []
    assert _tip_seqs([(CHAIN, 2), ("CGGTCA", 1)], 4, False, 0, 0)[1] == []      # max_kmers 0: nothing is a tip


def test_tip_on_a_circle():
    """the circle ACGGTCTA (8 k-mers, counted twice) with the branch GGTC -> GTCA -> TCAA: the branch cuts the circle
    open at GGTC, the tip GTCAA goes, and the re-compacted graph is one circular unitig"""
    c = "ACGGTCTA"
    table = _table([(c + c[:3], 2), ("GGTCAA", 1)], 4, False)
    units, link_ptr, links = tr.graph(table, 4, False)
    assert [(u[0], u[3]) for u in units] == [("GTCAA", False), ("GTCTAACGGTC", False)]
    assert tr.tips(units, link_ptr, links, False, 2, 0).tolist() == [1, 0]
    clipped, report, reduced = tr.clip(table, 4, False, 1, 2, 0)
    assert [(u[0], u[2], u[3]) for u in clipped] == [("AACGGTCTAAC", 8, True)]
    assert report == [(2, 1, 2), (1, 0, 2)]
    assert len(reduced) == len(table) - 2


def test_a_well_covered_tip_stays():
    """GGTCA counted 6 times beside a chain counted twice: at ratio_q8 256 the chain (mean 2) does not reach the tip's
    mean (6) and the tip stays; the topological rule (0) removes it"""
    seqs = [(CHAIN, 2), ("GGTCA", 6)]
    assert _tip_seqs(seqs, 4, False, 2, 256)[1] == []
    assert _tip_seqs(seqs, 4, False, 2, 0)[1] == ["GGTCA"]
    assert _tip_seqs(seqs, 4, False, 2, 85)[1] == ["GGTCA"]     # 256 * 2 >= 85 * 6
    assert _tip_seqs(seqs, 4, False, 2, 86)[1] == []


def test_hairpin_next_to_a_tip():
    """k = 5, both strands.  The stem CCAAGATTCAC runs into the hairpin GATTCAC + rc(GATTCAC): its loop ACGTGA follows the
    stem and leads back into the stem's mirror image, so both of its ends are attached and it is no candidate.  The
    branch TCACC -> CACCA leaves the stem at the same end: a tip, beaten by the loop (mean 4 against 1)."""
    seqs = [("CCAAGATTCAC" + ur.rc("GATTCAC"), 2), ("ATTCACCA", 1)]
    units, tips = _tip_seqs(seqs, 5, True, 3, 0)
    assert units == ["ACGTGA", "CCAAGATTCAC", "TCACCA"]
    assert tips == ["TCACCA"]
    assert _tip_seqs(seqs, 5, True, 3, 512)[1] == ["TCACCA"]
    assert _tip_seqs(seqs[:1], 5, True, 3, 0)[1] == []          # the hairpin alone folds into one unitig: nothing to clip


def test_even_k_palindrome():
    """k = 4, both strands: ACGT is its own reverse complement, a single-node unitig both of whose orientations are link
    targets.  GACCAACGTATCGG passes through it; its flanks CCGATACG and CGTTGGTC (5 k-mers each) are no candidates.  The
    branch ACGT -> CGTC is one: one k-mer, one end dead, and at the palindrome the flanks beat it."""
    seqs = [("GACCAACGTATCGG", 2), ("ACGTC", 1)]
    units, tips = _tip_seqs(seqs, 4, True, 3, 0)
    assert units == ["ACGT", "CCGATACG", "CGTC", "CGTTGGTC"]
    assert tips == ["CGTC"]
    assert _tip_seqs(seqs[:1], 4, True, 3, 0) == (["ACGT", "CCGATACG", "CGTTGGTC"], [])


# ------------------------------------------------------------------ invariants on random inputs

@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [3, 4, 12, 21])
def test_reference_invariants(k, canonical):
    rng = np.random.default_rng(900 + 2 * k + canonical)
    seen_tips = 0
    for _ in range(12):
        table = {}
        for s in _random_input(rng, k):
            ur.count_kmers([s], k, canonical, 1, table)
        units, link_ptr, links = tr.graph(table, k, canonical)
        for max_kmers, ratio_q8 in ((k, 0), (k, 512), (1, 256), (3 * k, 0)):
            tip = tr.tips(units, link_ptr, links, canonical, max_kmers, ratio_q8)       # (asserts the mirror symmetry)
            cand = tr.candidates(units, link_ptr, links, canonical, max_kmers)
            assert all(cand[j] for j in np.flatnonzero(tip))
            seen_tips += int(tip.sum())
        assert not tr.tips(units, link_ptr, links, canonical, 0, 0).any()
        # clip and re-compact until a round finds nothing: within n_unitigs rounds
        clipped, report, reduced = tr.clip(table, k, canonical, 1, 3 * k, 0, rounds=len(units) + 1)
        assert report[-1][1] == 0 and len(report) <= len(units) + 1
        assert report[-1][2] == len(table) - len(reduced)
        assert [u[0] for u in clipped] == [u[0] for u in ur.unitigs(reduced, k, canonical)]
    assert seen_tips > 0 or k <= 4       # (at k = 3 and 4 nearly every k-mer is there: a graph without dead ends)


def test_masked_table():
    table = {"ACG": 2, "CGT": 1, "AAA": 5}
    assert tr.masked_table(table, ["CGT", "TTT", "GGG"]) == {"ACG": 2, "AAA": 5}
    assert tr.masked_table(table, ["TTT"], canonical=True) == {"ACG": 2, "CGT": 1}
    assert table == {"ACG": 2, "CGT": 1, "AAA": 5}
    assert tr.report_text([(5, 2, 3), (3, 0, 3)]) == b"1\t5\t2\t3\n2\t3\t0\t3\n"


# ------------------------------------------------------------------ the CLI's refusals, the kernels' resources

@pytest.mark.parametrize("args, msg", [
    (["--global", "--unitigs-clip-tips"], b"--unitigs-clip-tips needs --unitigs-out UFILE, --unitigs-gfa GFILE or --unitigs-map QFILE"),
    (["--global", "--unitigs-gfa", "g.gfa", "--tip-max-kmers", "5"], b"need --unitigs-clip-tips"),
    (["--global", "--unitigs-gfa", "g.gfa", "--tip-ratio", "1.5"], b"need --unitigs-clip-tips"),
    (["--global", "--unitigs-gfa", "g.gfa", "--tip-rounds", "2"], b"need --unitigs-clip-tips"),
    (["--global", "--unitigs-gfa", "g.gfa", "--tip-report", "r.tsv"], b"need --unitigs-clip-tips"),
    (["--global", "--unitigs-gfa", "g.gfa", "--unitigs-clip-tips", "--tip-ratio", "-0.5"], b"--tip-ratio needs a number from 0 to 256"),
    (["--global", "--unitigs-gfa", "g.gfa", "--unitigs-clip-tips", "--tip-ratio", "256.5"], b"--tip-ratio needs a number from 0 to 256"),
    (["--global", "--unitigs-gfa", "g.gfa", "--unitigs-clip-tips", "--tip-ratio", "two"], b"--tip-ratio needs a number from 0 to 256"),
    (["--global", "--unitigs-gfa", "g.gfa", "--unitigs-clip-tips", "--tip-rounds", "0"], b"--tip-rounds needs a count"),
    (["--global", "--unitigs-gfa", "g.gfa", "--unitigs-clip-tips", "--tip-max-kmers", "x"], b"--tip-max-kmers needs a count"),
    (["--global", "--unitigs-gfa", "g.gfa", "--unitigs-clip-tips", "--tip-report"], b"--tip-report needs a value"),
    (["--unitigs-gfa", "g.gfa", "--unitigs-clip-tips"], b"--unitigs-gfa needs --global"),
])
def test_cli_refuses_bad_tip_options_before_reading_input(cli, tmp_path, args, msg):
    out = tmp_path / "o.txt"
    p = subprocess.run([cli, str(tmp_path / "missing.fasta"), str(out), "15"] + args, cwd=tmp_path, capture_output=True, timeout=60)
    assert p.returncode == 1
    assert msg in p.stderr
    assert not out.exists() and not (tmp_path / "g.gfa").exists() and not (tmp_path / "r.tsv").exists()


@pytest.mark.parametrize("source, pattern, kernels", [
    ("unitig_tips.hip", r"\dut_[a-z_]+_kernel", {"ut_check_kernel": 2, "ut_cand_kernel": 2, "ut_decide_kernel": 2, "ut_indeg_kernel": 1,
                                                  "ut_in_fill_kernel": 1}),
    ("unitig_mask.hip", r"\dum_[a-z_]+_kernel", {"um_keys_kernel": 6, "um_unitigs_kernel": 6, "um_count_kernel": 6}),
])
def test_tip_and_mask_kernels_use_no_scratch(tmp_path, source, pattern, kernels):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path / (source + ".s")
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(CSRC, source), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = []
    for name, ops, size in _functions(out.read_text()):
        if not re.search(pattern, name):                        # (the library scan is not this project's kernel)
            continue
        names.append(name)
        assert ops == 0, f"{name} has {ops} scratch instructions"
        assert not size, f"{name} reserves {size} bytes of scratch per thread"
    for kern, n in kernels.items():
        assert sum(kern in x for x in names) == n, kern
