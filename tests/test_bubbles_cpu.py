"""CPU-side checks of the bubble rule: the C ABI declares and exports the two calls and the Python mirror exists; the
plain-Python reference of tests/bubbles_ref.py gives the hand-worked answers on graphs small enough to draw and keeps its
invariants on random inputs; the planted inputs of the GPU tests have what those tests need; the report formatter of
libcfrk_host.so against the reference text; the host-check program under the sanitizers; the CLI's refusals; the
kernels of unitig_bubbles.hip use no scratch memory."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from . import bubbles_ref as br
from . import tips_ref as tr
from . import unitig_links_ref as lr
from . import unitig_ref as ur
from .test_gpu_bubbles import KS, _bubble_input, _ref
from .test_kernel_resources import CSRC, HIPCC, ROOT, _functions
from .test_unitigs_cpu import _random_input

NEW_CALLS = ("cfrk_global_unitig_bubbles", "cfrk_global_unitig_bubbles_device")


@pytest.fixture(scope="module")
def built():
    import cfrk_amd
    if not os.path.exists(cfrk_amd.library_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return cfrk_amd


@pytest.fixture(scope="module")
def host():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host"), "../libcfrk_host.so"], stdout=subprocess.DEVNULL)
    L = C.CDLL(os.path.join(ROOT, "cfrk_amd", "libcfrk_host.so"))
    vp = C.c_void_p
    L.cfrk_host_format_bubbles.argtypes = [C.c_uint32, vp, vp, vp, vp, C.c_int64, vp, vp, C.c_char_p, C.c_size_t]
    L.cfrk_host_format_bubbles.restype = C.c_size_t
    return L


@pytest.fixture(scope="module")
def cli(built):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "cfrk_amd", "cfrk")


def test_abi_declares_and_exports_the_bubble_calls(built):
    syms = built.abi_symbols()
    L = C.CDLL(built.library_path())
    for s in NEW_CALLS:
        assert s in syms
        assert hasattr(L, s)
    header = open(os.path.join(ROOT, "include", "cfrk_abi.h")).read()
    m = re.search(r"#define CFRK_BUBBLE_NONE\s+(0x[0-9a-fA-F]+)\b", header)
    assert m and int(m.group(1), 0) == built.CFRK_BUBBLE_NONE == br.NONE == 0xFFFFFFFF
    for text in ("Unitig bubbles", "The best-ranked arm of any (src, dst)", "it is never also a tip", "max_kmers = 0 pops nothing",
                 "depends on no order"):
        assert text in header, text
    for name in ("unitig_bubbles", "unitig_bubbles_device", "simplify", "clip_tips"):
        assert callable(getattr(built.GlobalCounter, name))
    assert built.UNITIG_DTYPE.itemsize == 16 and built.UNITIG_LINK_DTYPE.itemsize == 8
    assert "bubble_ratio" in built.GlobalCounter.simplify.__doc__ and "not a measured" in built.GlobalCounter.simplify.__doc__


# ------------------------------------------------------------------ the reference on graphs one can draw

def _table(seqs, k, canonical):
    table = {}
    for s, t in seqs:
        ur.count_kmers([s], k, canonical, t, table)
    return table


def _pop_seqs(seqs, k, canonical, *params):
    table = _table(seqs, k, canonical)
    units, link_ptr, links = tr.graph(table, k, canonical)
    pop, partner = br.bubbles(units, link_ptr, links, canonical, *params)
    return [u[0] for u in units], {units[j][0]: (units[int(partner[j]) >> 1][0], int(partner[j]) & 1) for j in np.flatnonzero(pop)}


CHAIN = "AACCGGTATCTGA"     # k = 4: no 3-mer twice.  Replacing the T of GGTA by C gives the k-mers CGGC GGCA GCAT CATC.
SNP_C, SNP_G, DEL = "CGGCATC", "CGGGATC", "CGGATC"


def test_a_substitution_bubble():
    """k = 4, plain strands, the chain counted twice, the substitution once:

                  / GGTA - GTAT - TATC \\
        .. - CGG <                      > ATC - ..        unitigs AACCGG, ATCTGA, CGGCATC, CGGTATC
                  \\ GGCA - GCAT - CATC /                 (the arms spelled with their k - 1 shared bases)

    both arms have one link in and one out, from AACCGG and into ATCTGA; the mean coverages are 1 and 2: the
    substitution is popped, its partner is the chain's arm"""
    units, popped = _pop_seqs([(CHAIN, 2), (SNP_C, 1)], 4, False, 4, 0, 0)
    assert units == ["AACCGG", "ATCTGA", "CGGCATC", "CGGTATC"]
    assert popped == {"CGGCATC": ("CGGTATC", 0)}
    # equal means: the index decides, and the list ascends by first k-mer
    assert _pop_seqs([(CHAIN, 2), (SNP_C, 2)], 4, False, 4, 0, 0)[1] == {"CGGTATC": ("CGGCATC", 0)}
    # asked for twice the coverage: exactly twice is enough, a 256th more is not
    assert _pop_seqs([(CHAIN, 2), (SNP_C, 1)], 4, False, 4, 0, 512)[1] == {"CGGCATC": ("CGGTATC", 0)}
    assert _pop_seqs([(CHAIN, 2), (SNP_C, 1)], 4, False, 4, 0, 513)[1] == {}
    assert _pop_seqs([(CHAIN, 2), (SNP_C, 2)], 4, False, 4, 0, 512)[1] == {}        # a balanced site stays
    # an arm longer than max_kmers is no arm; max_kmers 0 pops nothing
    assert _pop_seqs([(CHAIN, 2), (SNP_C, 1)], 4, False, 3, 0, 0)[1] == {}
    assert _pop_seqs([(CHAIN, 2), (SNP_C, 1)], 4, False, 0, 0, 0)[1] == {}


def test_three_alleles_and_a_deletion():
    """three arms between the same ends, counted 1, 2 and 3: the two weaker ones go, both name the best as their partner.  A
    deletion's arm has k - 1 k-mers beside k: parallel at max_diff 1 only"""
    units, popped = _pop_seqs([(CHAIN, 2), (SNP_C, 1), (SNP_G, 3)], 4, False, 4, 0, 0)
    assert units == ["AACCGG", "ATCTGA", "CGGCATC", "CGGGATC", "CGGTATC"]
    assert popped == {"CGGCATC": ("CGGGATC", 0), "CGGTATC": ("CGGGATC", 0)}
    units, popped = _pop_seqs([(CHAIN, 2), (DEL, 1)], 4, False, 4, 0, 0)
    assert units == ["AACCGG", "ATCTGA", "CGGATC", "CGGTATC"] and popped == {}
    assert _pop_seqs([(CHAIN, 2), (DEL, 1)], 4, False, 4, 1, 0)[1] == {"CGGATC": ("CGGTATC", 0)}
    # 10, 12 and 14 k-mers at max_diff 2: the shortest and the longest are not parallel (records and rows, no k-mers)
    units = [("", 50, 5, False), ("", 10, 10, False), ("", 24, 12, False), ("", 42, 14, False), ("", 50, 5, False)]
    link_ptr = np.array([0, 3, 4, 5, 6, 6], np.int64)
    links = np.array([(1, 0), (2, 0), (3, 0), (4, 0), (4, 0), (4, 0)], lr.UNITIG_LINK_DTYPE)
    pop, partner = br.bubbles(units, link_ptr, links, False, 20, 2, 0)
    assert pop.tolist() == [0, 1, 1, 0, 0] and partner.tolist() == [br.NONE, 2 << 1, 3 << 1, br.NONE, br.NONE]
    pop, partner = br.bubbles(units, link_ptr, links, False, 20, 4, 0)
    assert pop.tolist() == [0, 1, 1, 0, 0] and partner.tolist() == [br.NONE, 3 << 1, 3 << 1, br.NONE, br.NONE]


def test_what_stays():
    """an arm that carries a tip has two links out and is no arm; a tip is no arm; arms between different ends are not
    parallel"""
    units, popped = _pop_seqs([(CHAIN, 2), (SNP_C, 1), ("GGCAA", 1)], 4, False, 4, 1, 0)
    assert "GCAA" in units and popped == {}
    units, popped = _pop_seqs([(CHAIN, 2), ("CGGTCA", 1)], 4, False, 4, 1, 0)
    assert "GGTCA" in units and popped == {}


def test_the_loop_and_the_report_text():
    table = _table([(CHAIN, 2), (SNP_C, 1)], 4, False)
    units, report, reduced, rows = br.simplify(table, 4, False)
    assert [(u[0], u[1], u[2]) for u in units] == [(CHAIN, 20, 10)]
    assert report == [(4, 0, 1, 4), (1, 0, 0, 4)] and len(reduced) == len(table) - 4
    assert br.report_text(report) == b"1\t4\t0\t1\t4\n2\t1\t0\t0\t4\n"
    assert br.bubble_lines(rows) == b"1\t2\t3\t+\t7\t7\t1.0\t2.0\tsnp\tCGGCATC\tCGGTATC\n"
    # tips only: the tip loop's numbers
    for canonical in (False, True):
        table = _table([(CHAIN, 2), (SNP_C, 1), ("CTGAC", 1), ("TCTGG", 1)], 4, canonical)
        units, report, reduced, rows = br.simplify(table, 4, canonical, 1, True, False)
        clipped, clip_report, clip_reduced = tr.clip(table, 4, canonical)
        assert units == clipped and reduced == clip_reduced and rows == []
        assert [(u, t, m) for u, t, b, m in report] == clip_report


# ------------------------------------------------------------------ invariants on random inputs, the planted inputs

@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [3, 4, 12, 21])
def test_reference_invariants(k, canonical):
    rng = np.random.default_rng(1900 + 2 * k + canonical)
    for _ in range(8):
        table = {}
        for s in _random_input(rng, k):
            ur.count_kmers([s], k, canonical, int(rng.integers(1, 4)), table)
        units, link_ptr, links = tr.graph(table, k, canonical)
        for params in ((k, 0, 0), (k, 1, 0), (3 * k, 2, 512), (k, 1, 513)):
            pop, partner = br.bubbles(units, link_ptr, links, canonical, *params)   # (asserts the header's properties)
            arms = br.arms(units, link_ptr, links, canonical, params[0])
            assert all(arms[j] for j in np.flatnonzero(pop))
        assert not br.bubbles(units, link_ptr, links, canonical, 0, 0, 0)[0].any()
        final, report, reduced, rows = br.simplify(table, k, canonical, 1, True, True, len(units) + 1, 3 * k, 0, 3 * k, 2, 0)
        assert report[-1][1:3] == (0, 0) and report[-1][3] == len(table) - len(reduced)
        assert [u[0] for u in final] == [u[0] for u in ur.unitigs(reduced, k, canonical)]
        assert len(rows) == sum(r[2] for r in report)


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", KS)
def test_the_input_has_bubbles_and_survivors(k, canonical):
    """on the reference alone: every point of the grid has at least three popped arms and an arm that stays; from k = 12 on
    each planted structure does what it was planted for.

    One point has two popped arms, not three: k = 3 with both strands.  That graph has 32 nodes in all; an arm needs
    every one of its k-mers to have a single successor and a single predecessor in both readings, three popped arms and
    the arm that beats them are at least 11 nodes (one arm of k - 1 k-mers, the others of k), and their 22 oriented
    k-mers leave too few of the 64 oriented 3-mers absent.  A search over 3.4 million planted inputs and an annealing
    over the 4^32 count tables themselves (counts 0 .. 3 per node) found 2 at best; without the canonical rule the
    search finds 3.  The input committed for that point is one of those with 2."""
    table, units, link_ptr, links = _ref(k, canonical)
    pop, partner = br.bubbles(units, link_ptr, links, canonical, k, 1, 0)
    arms = br.arms(units, link_ptr, links, canonical, k)
    assert pop.sum() >= (2 if (k, canonical) == (3, True) else 3), (k, canonical)
    assert sum(arms) - pop.sum() >= 1, (k, canonical)
    if k < 12:
        return
    n = lambda *params: int(br.bubbles(units, link_ptr, links, canonical, *params)[0].sum())
    assert n(k, 1, 0) >= n(k, 0, 0) + 2                 # the deletion and the insertion
    assert n(k, 1, 0) == n(k, 1, 512) + 1               # the arm counted as often as the genome: the index decides, or nothing does
    assert n(k, 1, 512) >= n(k, 1, 513) + 2             # the arm counted twice beside the genome's 4, and the one beside the circle
    assert n(k + 1, 1, 0) > n(k, 1, 0)                  # the arm of k + 1 k-mers
    tip = tr.tips(units, link_ptr, links, canonical, k, 512)
    assert tip.sum() >= 3 and not (tip & pop).any()


# ------------------------------------------------------------------ the formatter

def _format(L, rnd, units, pop, partner):
    data, start, length, rec = ur.layout(units)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if len(a) else None
    args = (rnd, vp(data), vp(start), vp(length), vp(rec), len(units), vp(pop), vp(partner))
    n = L.cfrk_host_format_bubbles(*args, None, 0)
    buf = C.create_string_buffer(n + 1)
    assert L.cfrk_host_format_bubbles(*args, buf, n) == n
    assert buf.raw[n:] == b"\0"                                  # nothing behind the size it asked for
    return buf.raw[:n]


def test_bubble_report_formatter(host):
    lines = 0
    kinds = set()
    for k, canonical in ((12, False), (12, True), (21, True), (33, False), (64, True)):
        table, units, link_ptr, links = _ref(k, canonical)
        for rnd, params in ((1, (k, 1, 0)), (7, (k + 1, 1, 0)), (4000000000, (k, 0, 512))):
            pop, partner = br.bubbles(units, link_ptr, links, canonical, *params)
            rows = [(rnd, j, int(partner[j]), units[j], units[int(partner[j]) >> 1]) for j in np.flatnonzero(pop).tolist()]
            want = br.bubble_lines(rows)
            assert _format(host, rnd, units, pop, partner) == want
            lines += want.count(b"\n")
            kinds |= {l.split(b"\t")[8] for l in want.splitlines()}
    assert lines > 60 and kinds == {b"snp", b"indel"}
    units = [("ACGTT", 7, 2, False), ("AACGA", 3, 2, False), ("ACGT", 1, 1, False), ("ACGAA", 4, 2, False)]
    pop, partner = np.array([0, 1, 1, 1], np.uint8), np.array([br.NONE, 0 << 1 | 1, 0 << 1, 0 << 1], np.uint32)
    want = (b"2\t1\t0\t-\t5\t5\t1.5\t3.5\tsnp\tAACGA\tAACGT\n2\t2\t0\t+\t4\t5\t1.0\t3.5\tindel\tACGT\tACGTT\n"
            b"2\t3\t0\t+\t5\t5\t2.0\t3.5\tmnp\tACGAA\tACGTT\n")
    assert _format(host, 2, units, pop, partner) == want
    rows = [(2, j, int(partner[j]), units[j], units[0]) for j in (1, 2, 3)]
    assert br.bubble_lines(rows) == want
    assert _format(host, 1, [], np.zeros(0, np.uint8), np.zeros(0, np.uint32)) == b""


def test_host_check_program_under_sanitizers(tmp_path):
    """tools/bubbles_host_check.cpp: the formatter into buffers of exactly the size it asked for, under ASan and UBSan"""
    exe = tmp_path / "bubbles_host_check"
    # (the runtimes linked into the program itself: it is a stand-alone program, whatever else the process loads)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-o", str(exe), os.path.join(ROOT, "tools", "bubbles_host_check.cpp"),
                           os.path.join(ROOT, "cfrk_amd", "host", "cfrk_host.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "formatter and restatement agree" in p.stdout


# ------------------------------------------------------------------ the CLI's refusals, the kernels' resources

@pytest.mark.parametrize("args, msg", [
    (["--global", "--unitigs-pop-bubbles"], b"--unitigs-pop-bubbles needs --unitigs-out UFILE, --unitigs-gfa GFILE or --unitigs-map QFILE"),
    (["--global", "--unitigs-gfa", "g.gfa", "--bubble-max-kmers", "5"], b"need --unitigs-pop-bubbles"),
    (["--global", "--unitigs-gfa", "g.gfa", "--bubble-max-diff", "1"], b"need --unitigs-pop-bubbles"),
    (["--global", "--unitigs-gfa", "g.gfa", "--bubble-ratio", "1.5"], b"need --unitigs-pop-bubbles"),
    (["--global", "--unitigs-gfa", "g.gfa", "--bubble-report", "b.tsv"], b"need --unitigs-pop-bubbles"),
    (["--global", "--unitigs-gfa", "g.gfa", "--simplify-rounds", "2"], b"need --unitigs-pop-bubbles"),
    (["--global", "--unitigs-gfa", "g.gfa", "--unitigs-clip-tips", "--simplify-rounds", "2"], b"need --unitigs-pop-bubbles"),
    (["--global", "--unitigs-gfa", "g.gfa", "--unitigs-pop-bubbles", "--unitigs-clip-tips", "--tip-rounds", "2"], b"--simplify-rounds"),
    (["--global", "--unitigs-gfa", "g.gfa", "--unitigs-pop-bubbles", "--tip-ratio", "1.5"], b"need --unitigs-clip-tips"),
    (["--global", "--unitigs-gfa", "g.gfa", "--tip-report", "r.tsv"], b"need --unitigs-clip-tips"),
    (["--global", "--unitigs-gfa", "g.gfa", "--unitigs-pop-bubbles", "--bubble-ratio", "-0.5"], b"--bubble-ratio needs a number from 0 to 256"),
    (["--global", "--unitigs-gfa", "g.gfa", "--unitigs-pop-bubbles", "--bubble-ratio", "257"], b"--bubble-ratio needs a number from 0 to 256"),
    (["--global", "--unitigs-gfa", "g.gfa", "--unitigs-pop-bubbles", "--simplify-rounds", "0"], b"--simplify-rounds needs a count"),
    (["--global", "--unitigs-gfa", "g.gfa", "--unitigs-pop-bubbles", "--bubble-max-kmers", "0"], b"--bubble-max-kmers needs a count"),
    (["--global", "--unitigs-gfa", "g.gfa", "--unitigs-pop-bubbles", "--bubble-max-diff", "x"], b"--bubble-max-diff needs a count"),
    (["--global", "--unitigs-gfa", "g.gfa", "--unitigs-pop-bubbles", "--bubble-report"], b"--bubble-report needs a value"),
    (["--unitigs-gfa", "g.gfa", "--unitigs-pop-bubbles"], b"--unitigs-gfa needs --global"),
])
def test_cli_refuses_bad_bubble_options_before_reading_input(cli, tmp_path, args, msg):
    out = tmp_path / "o.txt"
    p = subprocess.run([cli, str(tmp_path / "missing.fasta"), str(out), "15"] + args, cwd=tmp_path, capture_output=True, timeout=60)
    assert p.returncode == 1
    assert msg in p.stderr
    assert not out.exists() and not (tmp_path / "g.gfa").exists() and not (tmp_path / "r.tsv").exists() and not (tmp_path / "b.tsv").exists()


def test_bubble_kernels_use_no_scratch(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path / "unitig_bubbles.hip.s"
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(CSRC, "unitig_bubbles.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = []
    for name, ops, size in _functions(out.read_text()):
        if not re.search(r"\du[bt]_[a-z_]+_kernel", name):       # (the library scan is not this project's kernel)
            continue
        names.append(name)
        assert ops == 0, f"{name} has {ops} scratch instructions"
        assert not size, f"{name} reserves {size} bytes of scratch per thread"
    for kern, n in {"ut_check_kernel": 2, "ut_indeg_kernel": 1, "ut_in_fill_kernel": 1, "ub_arm_kernel": 2, "ub_decide_kernel": 2}.items():
        assert sum(kern in x for x in names) == n, kern
