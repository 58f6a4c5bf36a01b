"""CPU-side checks of the weak rule: the C ABI declares and exports the two calls and the Python mirror exists; the
plain-Python reference of tests/weak_ref.py gives the hand-worked answers on graphs small enough to draw and keeps the
header's four properties on random inputs under both strand rules; masking what the rule says and recomputing the
unitigs is the reference loop; the planted inputs of the GPU tests have what those tests need; the report formatter of
libcfrk_host.so against the reference text; the host-check program under the sanitizers; the CLI's refusals; the kernels
of unitig_weak.hip use no scratch memory and no LDS."""
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
from . import weak_ref as wr
from .test_kernel_resources import CSRC, HIPCC, ROOT, _functions
from .test_unitigs_cpu import _random_input
from .weak_cases import KS, PARAMS, ref

NEW_CALLS = ("cfrk_global_unitig_weak", "cfrk_global_unitig_weak_device")
FM, TM = lr.FROM_MINUS, lr.TO_MINUS


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
    L.cfrk_host_format_weak.argtypes = [C.c_uint32, vp, vp, vp, vp, C.c_int64, vp, C.c_char_p, C.c_size_t]
    L.cfrk_host_format_weak.restype = C.c_size_t
    return L


@pytest.fixture(scope="module")
def cli(built):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "cfrk_amd", "cfrk")


def test_abi_declares_and_exports_the_weak_calls(built):
    syms = built.abi_symbols()
    L = C.CDLL(built.library_path())
    for s in NEW_CALLS:
        assert s in syms
        assert hasattr(L, s)
    header = open(os.path.join(ROOT, "include", "cfrk_abi.h")).read()
    for name, value in (("CFRK_WEAK_CONNECTION", 1), ("CFRK_WEAK_ISOLATED", 2)):
        m = re.search(r"#define %s\s+(\d+)\b" % name, header)
        assert m and int(m.group(1)) == getattr(built, name) == value
    assert (wr.CONNECTION, wr.ISOLATED) == (1, 2)
    for text in ("Weak unitigs", "SELF-FREE", "ISOLATED", "WEAK CONNECTION", "depends on no order", "never leaves a neighbour with a",
                 "weak[] and tip[] of one graph are disjoint", "every unitig the bubble rule pops", "The converse is false",
                 "max_kmers = 0 makes no connection"):
        assert text in header, text
    assert header.index("Unitig bulges") < header.index("Weak unitigs") < header.index("Unitig compaction")
    for name in ("unitig_weak", "unitig_weak_device", "simplify"):
        assert callable(getattr(built.GlobalCounter, name))
    assert built.WEAK_STATS_DTYPE.itemsize == 24 and built.WEAK_STATS_DTYPE.names == ("connections", "isolated", "candidates")
    doc = built.GlobalCounter.simplify.__doc__
    assert "weak_ratio" in doc and "choices, not measured optima" in doc
    assert "not a measured optimum" in built.GlobalCounter.unitig_weak.__doc__


# ------------------------------------------------------------------ the reference on graphs one can draw

THICK, THIN = (200, 10), (3, 3)         # (kc, n_kmers): means 20 and 1


def _graph(recs, edges, canonical):
    """records [(kc, n) or (kc, n, circular)] and oriented links [(u, ou, v, ov)] -> (units, link_ptr, links); a canonical
    graph gets every link's mirror"""
    nS = len(recs)
    L = set(edges)
    if canonical:
        L |= {(v, 1 - ov, u, 1 - ou) for u, ou, v, ov in edges}
    L = sorted(L)
    links = np.array([(v, (FM if ou else 0) | (TM if ov else 0)) for u, ou, v, ov in L], lr.UNITIG_LINK_DTYPE).reshape(len(L))
    link_ptr = np.zeros(nS + 1, np.int64)
    np.cumsum(np.bincount(np.array([e[0] for e in L], np.int64), minlength=nS), out=link_ptr[1:])
    units = [("", r[0], r[1], len(r) > 2 and r[2]) for r in recs]
    return units, link_ptr, links


def _weak(recs, edges, canonical, *params):
    weak, stats = wr.weak(*_graph(recs, edges, canonical), canonical, *params)
    assert stats["connections"] == int((weak == 1).sum()) and stats["isolated"] == int((weak == 2).sum())
    return weak.tolist(), stats["candidates"]


PLUS = lambda pairs: [(u, 0, v, 0) for u, v in pairs]
# two thick paths a0 -> a1 and b0 -> b1, and x from a0 to b1:  a0 = 0, a1 = 1, b0 = 2, b1 = 3, x = 4
BRIDGE = PLUS([(0, 1), (2, 3), (0, 4), (4, 3)])


@pytest.mark.parametrize("canonical", [False, True])
def test_a_thin_bridge_between_two_thick_paths(canonical):
    """
        a0 ---- a1            x has a link at both ends, so it is no tip; at a0 its sibling is a1, at b1 its sibling is b0,
          \\                  both of 20 times its coverage: a weak connection.  The thick unitigs have a dead end each
           x                  and 10 k-mers: no candidates at max_kmers 5
            \\
        b0 ---- b1
    """
    recs = [THICK, THICK, THICK, THICK, THIN]
    assert _weak(recs, BRIDGE, canonical, 5, 1024) == ([0, 0, 0, 0, 1], 1)
    assert _weak(recs, BRIDGE, canonical, 3, 20 * 256) == ([0, 0, 0, 0, 1], 1)          # exactly 20 times is enough ...
    assert _weak(recs, BRIDGE, canonical, 3, 20 * 256 + 1) == ([0, 0, 0, 0, 0], 1)      # ... a 256th more is not
    assert _weak(recs, BRIDGE, canonical, 2, 0) == ([0, 0, 0, 0, 0], 0)                 # longer than max_kmers: no candidate
    assert _weak(recs, BRIDGE, canonical, 0, 0) == ([0, 0, 0, 0, 0], 0)
    # a circular record is no candidate, whatever its rows say
    assert _weak(recs[:4] + [THIN + (True,)], BRIDGE, canonical, 5, 0) == ([0, 0, 0, 0, 0], 0)
    # with every unitig short enough the thick ones are candidates only where both ends are linked: none here
    assert _weak(recs, BRIDGE, canonical, 10, 0) == ([0, 0, 0, 0, 1], 1)
    if canonical:   # x stored the other way round: entered and left as (x,-)
        flipped = PLUS([(0, 1), (2, 3)]) + [(0, 0, 4, 1), (4, 1, 3, 0)]
        assert _weak(recs, flipped, True, 5, 1024) == ([0, 0, 0, 0, 1], 1)


@pytest.mark.parametrize("canonical", [False, True])
def test_a_bridge_that_is_the_best_neighbour_at_one_attachment_stays(canonical):
    """b0 thinner than x: at b1 no sibling beats x, and "every attachment" fails.  b1 keeps its best way in"""
    recs = [THICK, THICK, (1, 2), THICK, THIN]                                          # b0: mean 0.5
    assert _weak(recs, BRIDGE, canonical, 5, 0) == ([0, 0, 0, 0, 0], 1)
    # b0 of twice x's coverage: enough at ratio 2, not at the default 4
    recs[2] = (20, 10)
    assert _weak(recs, BRIDGE, canonical, 5, 512) == ([0, 0, 0, 0, 1], 1)
    assert _weak(recs, BRIDGE, canonical, 5, 1024) == ([0, 0, 0, 0, 0], 1)
    # equal means: the index decides.  b0 = 2 < x = 4 ranks above x; with the indices swapped it does not
    recs[2] = (10, 10)
    assert _weak(recs, BRIDGE, canonical, 5, 256) == ([0, 0, 0, 0, 1], 1)
    swapped = PLUS([(0, 1), (4, 3), (0, 2), (2, 3)])                                    # x = 2, b0 = 4
    assert _weak([THICK, THICK, THIN, THICK, (10, 10)], swapped, canonical, 5, 256) == ([0, 0, 0, 0, 0], 1)


@pytest.mark.parametrize("canonical", [False, True])
def test_two_bridges_side_by_side(canonical):
    """x (mean 1) and y (mean 2) both from a0 to b1.  Beside the thick paths both go.  Without them they are the two arms of
    a bubble: the better one is the best neighbour of both ends and stays, the other is what the bubble rule pops"""
    edges = BRIDGE + PLUS([(0, 5), (5, 3)])
    recs = [THICK, THICK, THICK, THICK, THIN, (6, 3)]
    assert _weak(recs, edges, canonical, 5, 1024) == ([0, 0, 0, 0, 1, 1], 2)
    alone = PLUS([(0, 4), (4, 3), (0, 5), (5, 3)])
    assert _weak(recs, alone, canonical, 5, 512) == ([0, 0, 0, 0, 1, 0], 2)
    assert _weak(recs, alone, canonical, 5, 513) == ([0, 0, 0, 0, 0, 0], 2)
    units, link_ptr, links = _graph(recs, alone, canonical)
    assert br.bubbles(units, link_ptr, links, canonical, 5, 0, 512)[0].tolist() == [0, 0, 0, 0, 1, 0]
    # the converse is false: x and y between DIFFERENT ends on one side are no bubble, and still connections
    apart = BRIDGE + PLUS([(0, 5), (5, 1)])                                             # y: a0 -> a1's other way in
    assert _weak(recs, apart, canonical, 5, 1024) == ([0, 0, 0, 0, 1, 1], 2)
    units, link_ptr, links = _graph(recs, apart, canonical)
    assert not br.bubbles(units, link_ptr, links, canonical, 5, 3, 0)[0].any()


@pytest.mark.parametrize("canonical", [False, True])
def test_a_bridge_whose_sibling_is_a_tip(canonical):
    """at a0 the only sibling of x is t, a dead end (a candidate of the tip rule).  BEATS does not ask what the sibling is: a
    thick t beats x.  The tip rule leaves t alone (x does not beat it), and the two results are disjoint"""
    edges = PLUS([(2, 3), (0, 4), (4, 3), (0, 1)])                                      # 1 = t: a0 -> t and nothing behind it
    recs = [THICK, (40, 2), THICK, THICK, THIN]
    assert _weak(recs, edges, canonical, 5, 1024) == ([0, 0, 0, 0, 1], 1)
    units, link_ptr, links = _graph(recs, edges, canonical)
    assert tr.candidates(units, link_ptr, links, canonical, 5)[1] and not tr.tips(units, link_ptr, links, canonical, 5, 512).any()
    # a tip thinner than the bridge: the bridge is a0's best way out and stays; the tip rule takes the tip
    recs[1] = (1, 2)
    assert _weak(recs, edges, canonical, 5, 0) == ([0, 0, 0, 0, 0], 1)
    assert tr.tips(units[:1] + [("", 1, 2, False)] + units[2:], link_ptr, links, canonical, 5, 512).tolist() == [0, 1, 0, 0, 0]


def test_hairpin_self_link_and_palindrome():
    """a unitig with a link to itself, in either orientation, is not self-free: no candidate, although both its ends are
    linked and thick siblings stand by"""
    recs = [THICK, THICK, THICK, THICK, THIN]
    # a hairpin (x,+) -> (x,-) in a canonical job (its own mirror): a0 -> x -> rc(x) -> rc(a0)
    hairpin = PLUS([(0, 1), (0, 4)]) + [(4, 0, 4, 1)]
    assert _weak(recs, hairpin, True, 5, 0) == ([0, 0, 0, 0, 0], 0)
    # a self-link (x,+) -> (x,+): a homopolymer node between a0 and b1
    for canonical in (False, True):
        assert _weak(recs, BRIDGE + PLUS([(4, 4)]), canonical, 5, 0) == ([0, 0, 0, 0, 0], 0)
    # (x,-) -> (x,+), the other hairpin
    assert _weak(recs, PLUS([(2, 3), (4, 3)]) + [(4, 1, 4, 0)], True, 5, 0) == ([0, 0, 0, 0, 0], 0)
    # a palindromic single node at even k, from k-mers: ACGT between thick flanks.  (ACGT,+) and (ACGT,-) are one
    # oriented node; whatever the rows hold, the properties hold and the palindrome is not dropped
    for k, mid in ((4, "ACGT"), (6, "ACGCGT")):
        table = {}
        ur.count_kmers(["GGTTC" + mid + "TCCAA"], k, True, 5, table)
        ur.count_kmers(["CATTC"[-(k - 1):] + mid + "GAGTA"[:k - 1]], k, True, 1, table)
        units, link_ptr, links = tr.graph(table, k, True)
        weak, stats = wr.weak(units, link_ptr, links, True, 3 * k, 0, 3 * k, 1 << 20)
        j = next(i for i, u in enumerate(units) if u[0] == mid)
        assert weak[j] == 0 and (link_ptr[j + 1] > link_ptr[j])


def test_an_isolated_unitig_at_its_thresholds():
    """no link at all: dropped iff not circular, n <= iso_max_kmers and 256 kc < iso_mean_q8 n"""
    recs = [(19, 10), (20, 10), (21, 10), (19, 11), (19, 10, True), (0, 1)]
    for canonical in (False, True):
        # mean below 2.0: 1.9 goes, 2.0 and 2.1 stay; 11 k-mers are one too many; a circle stays
        assert _weak(recs, [], canonical, 5, 0, 10, 512) == ([2, 0, 0, 0, 0, 2], 0)
        assert _weak(recs, [], canonical, 5, 0, 11, 512) == ([2, 0, 0, 2, 0, 2], 0)
        assert _weak(recs, [], canonical, 5, 0, 9, 512) == ([0, 0, 0, 0, 0, 2], 0)
        assert _weak(recs, [], canonical, 5, 0, 10, 513) == ([2, 2, 0, 0, 0, 2], 0)       # 256 * 20 < 513 * 10
        assert _weak(recs, [], canonical, 5, 0, 10, 486) == ([0, 0, 0, 0, 0, 2], 0)       # 256 * 19 = 4864 > 4860
        assert _weak(recs, [], canonical, 5, 0, 10, 487) == ([2, 0, 0, 0, 0, 2], 0)       # ... < 4870
        assert _weak(recs, [], canonical, 5, 0, 0, 512) == ([0] * 6, 0)
        assert _weak(recs, [], canonical, 5, 0, 10, 0) == ([0] * 6, 0)
        # one link is enough to be no isolated unitig (and a dead end is no connection either)
        assert _weak(recs, PLUS([(0, 1)]), canonical, 20, 0, 10, 512) == ([0, 0, 0, 0, 0, 2], 0)


# ------------------------------------------------------------------ the properties on random inputs, the loop

@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [3, 4, 12, 21])
def test_reference_properties_on_random_jobs(k, canonical):
    rng = np.random.default_rng(2700 + 2 * k + canonical)
    found = 0
    for _ in range(8):
        table = {}
        for s in _random_input(rng, k):
            ur.count_kmers([s], k, canonical, int(rng.integers(1, 4)), table)
        units, link_ptr, links = tr.graph(table, k, canonical)
        for params in ((k, 1024, 0, 0), (k, 0, 2 * k, 512), (3 * k, 256, 3 * k, 1 << 16), (3 * k, 512, 0, 0), (0, 1024, 2 * k, 0)):
            weak, stats = wr.weak(units, link_ptr, links, canonical, *params)       # (asserts the header's properties)
            cand = wr.candidates(units, link_ptr, links, canonical, params[0])
            assert all(cand[j] for j in np.flatnonzero(weak == 1)) and stats["candidates"] == sum(cand)
            found += int((weak != 0).sum())
        # the loop: every round masks what the rules say, and the end is the unitigs of the reduced dictionary
        final, report, reduced, rows, _, wrows = wr.simplify(table, k, canonical, 1, True, True, False, True, len(units) + 1, 3 * k, 0, 3 * k, 2, 0,
                                                             weak_max_kmers=3 * k, weak_ratio_q8=0, weak_iso_max_kmers=3 * k, weak_iso_mean_q8=512)
        assert report[-1][1:4] == (0, 0, 0) and report[-1][5:] == (0, 0) and report[-1][4] == len(table) - len(reduced)
        assert [u[0] for u in final] == [u[0] for u in ur.unitigs(reduced, k, canonical)]
        assert len(wrows) == sum(r[5] + r[6] for r in report) and len(rows) == sum(r[2] for r in report)
    assert found > 0


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [5, 12])
def test_masking_and_recomputing_is_the_loop(k, canonical):
    """one round by hand: the rule on the graph, its unitigs' k-mers out of the dictionary, the unitigs again -- that is
    round 2 of the reference loop; weak alone, and the loop without it is the loop there was"""
    table, units, link_ptr, links = ref(k, canonical)
    weak, stats = wr.weak(units, link_ptr, links, canonical, k, 1024, 2 * k, 512)
    gone = set()
    for j in np.flatnonzero(weak):
        gone.update(tr.unit_kmers(units[j][0], k, canonical))
    reduced = tr.masked_table(table, gone)
    final, report, _, _, _, wrows = wr.simplify(table, k, canonical, 1, False, False, False, True, rounds=2)
    assert report[0] == (len(units), 0, 0, 0, len(gone), stats["connections"], stats["isolated"])
    assert [(j, kind) for rnd, j, kind, _ in wrows if rnd == 1] == [(int(j), int(weak[j])) for j in np.flatnonzero(weak)]
    after = ur.unitigs(reduced, k, canonical)
    assert len(report) == 2 and report[1][0] == len(after)
    if report[1][5:] == (0, 0):
        assert final == after
    old = br.simplify(table, k, canonical, 1, True, True, 4)
    new = wr.simplify(table, k, canonical, 1, True, True, False, False, 4)
    assert new[0] == old[0] and new[2] == old[2] and new[3] == old[3] and new[5] == []
    assert wr.report_rows(new[1], True, False, False) == old[1]
    assert wr.report_text(new[1], True, False, False) == br.report_text(old[1])
    assert wr.report_text(new[1], False, False, False) == tr.report_text([(u, t, m) for u, t, b, m in old[1]])


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", KS)
def test_the_input_has_what_the_gpu_tests_need(k, canonical):
    """on the reference alone: every point of the grid has a connection that the bubble rule does not pop and a candidate
    that stays, from k = 12 on an isolated unitig that goes and one that stays; the parameter sets differ in what they find"""
    table, units, link_ptr, links = ref(k, canonical)
    n = lambda *p: wr.weak(units, link_ptr, links, canonical, *p)
    weak, stats = n(k, 1024, 2 * k, 512)
    pop = br.bubbles(units, link_ptr, links, canonical, k, 1 << 32, 1024)[0]
    assert ((weak == 1) & (pop == 0)).sum() >= 1, (k, canonical)
    assert stats["candidates"] > stats["connections"] >= 2
    entered = set(links["to"].tolist())
    none = sum(1 for j in range(len(units)) if link_ptr[j + 1] == link_ptr[j] and j not in entered and not units[j][3])
    if k >= 12:             # (at k = 5 the 1024 5-mers are too few for a random piece to float free of a genome of 170 bases)
        assert 1 <= stats["isolated"] < none
    # every ratio_q8 <= 256 is "whoever ranks above": the same; the default 1024 finds fewer
    assert n(k, 0, 0, 0)[1]["connections"] == n(k, 256, 0, 0)[1]["connections"] > stats["connections"]
    assert n(0, 1024, 0, 0)[1] == {"connections": 0, "isolated": 0, "candidates": 0}
    assert len(PARAMS(k)) == 6


# ------------------------------------------------------------------ the formatter

def _format(L, rnd, units, weak):
    data, start, length, rec = ur.layout(units)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if len(a) else None
    args = (rnd, vp(data), vp(start), vp(length), vp(rec), len(units), vp(weak))
    n = L.cfrk_host_format_weak(*args, None, 0)
    buf = C.create_string_buffer(n + 1)
    assert L.cfrk_host_format_weak(*args, buf, n) == n
    assert buf.raw[n:] == b"\0"                                  # nothing behind the size it asked for
    return buf.raw[:n]


def test_weak_report_formatter(host):
    lines = 0
    for k, canonical in ((12, False), (12, True), (21, True), (33, False)):
        table, units, link_ptr, links = ref(k, canonical)
        weak, _ = wr.weak(units, link_ptr, links, canonical, k, 256, 2 * k, 512)
        rows = [(3, int(j), int(weak[j]), units[j]) for j in np.flatnonzero(weak)]
        want = wr.weak_lines(rows)
        assert {1, 2} <= set(weak.tolist())
        assert _format(host, 3, units, weak) == want
        lines += len(rows)
        odd = weak.copy()                                         # any other byte: no line
        odd[odd == 0] = 3
        assert _format(host, 3, units, odd) == want
    assert lines >= 8
    assert wr.weak_lines([(1, 7, 1, ("ACGTA", 3, 2, False)), (2, 0, 2, ("ACGT", 1, 1, False))]) == \
        b"1\t7\tconnection\t5\t3\t1.5\tACGTA\n2\t0\tisolated\t4\t1\t1.0\tACGT\n"
    assert _format(host, 1, [], np.zeros(0, np.uint8)) == b""


def test_host_check_program_under_sanitizers(tmp_path):
    """tools/weak_host_check.cpp: the formatter into buffers of exactly the size it asked for, under ASan and UBSan"""
    exe = tmp_path / "weak_host_check"
    # (the runtimes linked into the program itself: it is a stand-alone program, whatever else the process loads)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-o", str(exe), os.path.join(ROOT, "tools", "weak_host_check.cpp"),
                           os.path.join(ROOT, "cfrk_amd", "host", "cfrk_host.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "formatter and restatement agree" in p.stdout


# ------------------------------------------------------------------ the CLI's refusals, the kernels' resources

G = ["--global", "--unitigs-gfa", "g.gfa"]


@pytest.mark.parametrize("args, msg", [
    (["--global", "--unitigs-drop-weak"], b"--unitigs-drop-weak needs --unitigs-out UFILE, --unitigs-gfa GFILE or --unitigs-map QFILE"),
    (G + ["--weak-max-kmers", "5"], b"need --unitigs-drop-weak"),
    (G + ["--weak-ratio", "1.5"], b"need --unitigs-drop-weak"),
    (G + ["--weak-iso-max-kmers", "5"], b"need --unitigs-drop-weak"),
    (G + ["--weak-iso-mean", "1.5"], b"need --unitigs-drop-weak"),
    (G + ["--weak-report", "w.tsv"], b"need --unitigs-drop-weak"),
    (G + ["--unitigs-pop-bubbles", "--weak-report", "w.tsv"], b"--weak-max-kmers, --weak-ratio, --weak-iso-max-kmers, --weak-iso-mean and --weak-report need"),
    (G + ["--unitigs-drop-weak", "--tip-rounds", "2", "--unitigs-clip-tips"], b"with --unitigs-drop-weak the rounds are set by --simplify-rounds N"),
    (G + ["--unitigs-drop-weak", "--tip-ratio", "1.5"], b"need --unitigs-clip-tips"),
    (G + ["--unitigs-drop-weak", "--bubble-ratio", "1.5"], b"need --unitigs-pop-bubbles"),
    (G + ["--unitigs-drop-weak", "--bulge-ratio", "1.5"], b"need --unitigs-pop-bulges"),
    (G + ["--unitigs-drop-weak", "--weak-ratio", "-0.5"], b"--weak-ratio needs a number from 0 to 256"),
    (G + ["--unitigs-drop-weak", "--weak-ratio", "257"], b"--weak-ratio needs a number from 0 to 256"),
    (G + ["--unitigs-drop-weak", "--weak-iso-mean", "x"], b"--weak-iso-mean needs a number from 0 to 256"),
    (G + ["--unitigs-drop-weak", "--weak-max-kmers", "0"], b"--weak-max-kmers needs a count"),
    (G + ["--unitigs-drop-weak", "--weak-iso-max-kmers", "-1"], b"--weak-iso-max-kmers needs a count"),
    (G + ["--unitigs-drop-weak", "--simplify-rounds", "0"], b"--simplify-rounds needs a count"),
    (G + ["--unitigs-drop-weak", "--weak-report"], b"--weak-report needs a value"),
    (["--unitigs-gfa", "g.gfa", "--unitigs-drop-weak"], b"--unitigs-gfa needs --global on one device"),
    (G + ["--simplify-rounds", "2"], b"need --unitigs-pop-bubbles"),                    # (as it was)
    (G + ["--simplify-recompact"], b"--simplify-recompact needs --unitigs-clip-tips, --unitigs-pop-bubbles or --unitigs-pop-bulges"),
])
def test_cli_refusals(cli, tmp_path, args, msg):
    p = subprocess.run([cli, str(tmp_path / "absent.fa"), str(tmp_path / "out"), "21"] + args, capture_output=True, timeout=60)
    assert p.returncode == 1 and msg in p.stderr, p.stderr
    assert not (tmp_path / "out").exists()


@pytest.mark.parametrize("args", [
    G + ["--unitigs-drop-weak"],
    G + ["--unitigs-drop-weak", "--simplify-rounds", "2", "--simplify-recompact", "--tip-report", "r.tsv", "--weak-report", "w.tsv"],
    G + ["--unitigs-drop-weak", "--weak-max-kmers", "9", "--weak-ratio", "3", "--weak-iso-max-kmers", "0", "--weak-iso-mean", "0"],
    G + ["--unitigs-drop-weak", "--unitigs-clip-tips", "--unitigs-pop-bubbles", "--unitigs-pop-bulges", "--tip-ratio", "1"],
])
def test_cli_accepts(cli, tmp_path, args):
    """accepted: the command gets as far as its input, which does not exist"""
    p = subprocess.run([cli, str(tmp_path / "absent.fa"), str(tmp_path / "out"), "21"] + args, capture_output=True, timeout=60)
    assert p.returncode != 0 and b"absent.fa" in p.stderr and b"needs" not in p.stderr and b"need " not in p.stderr, p.stderr


def test_weak_kernels_use_no_scratch_and_no_lds(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path / "unitig_weak.hip.s"
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(CSRC, "unitig_weak.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = out.read_text()
    names = []
    for name, ops, size in _functions(asm):
        if not re.search(r"\du[wt]_[a-z_]+_kernel", name):       # (the library scan is not this project's kernel)
            continue
        names.append(name)
        assert ops == 0, f"{name} has {ops} scratch instructions"
        assert not size, f"{name} reserves {size} bytes of scratch per thread"
    for kern, n in {"ut_check_kernel": 2, "ut_indeg_kernel": 1, "ut_in_fill_kernel": 1, "uw_decide_kernel": 2}.items():
        assert sum(kern in x for x in names) == n, kern
    # the decide kernel: no LDS, and below 64 VGPRs (the compiler's own remarks behind each function)
    for name in (x for x in names if "uw_decide_kernel" in x):
        tail = asm[asm.index("\n%s:" % name):]
        tail = tail[:tail.index(".Lfunc_end") + 4000]
        lds = re.search(r"; LDSByteSize: ?(\d+)", tail)
        vgprs = re.search(r"; NumVgprs: ?(\d+)", tail)
        assert lds and int(lds.group(1)) == 0, name
        assert vgprs and int(vgprs.group(1)) < 64, (name, vgprs and vgprs.group(1))
