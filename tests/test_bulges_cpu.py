"""CPU-side checks of the bulge rule: the C ABI declares and exports the two calls and the Python mirror exists; the
plain-Python reference of tests/bulges_ref.py gives the hand-worked answers on graphs small enough to draw, counts the
links it looks at in the order the header fixes, and keeps its invariants on random inputs; the inputs of the GPU tests
have what those tests need; the report formatter of libcfrk_host.so against the reference text; the host-check program
under the sanitizers; the CLI's refusals; the kernels of unitig_bulges.hip use no scratch memory and keep their stack in
LDS."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from . import bubbles_ref as br
from . import bulges_ref as gr
from . import tips_ref as tr
from . import unitig_ref as ur
from .test_gpu_bulges import P, fuzz_case, hand_cases, ladder, real_graph, real_input, records, rows_of, units_of
from .test_kernel_resources import CSRC, HIPCC, ROOT, _functions
from .test_unitigs_cpu import _random_input

NEW_CALLS = ("cfrk_global_unitig_bulges", "cfrk_global_unitig_bulges_device")


@pytest.fixture(scope="module")
def built():
    import cfrk_amd
    if not os.path.exists(cfrk_amd.library_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return cfrk_amd


def test_abi_declares_and_exports_the_bulge_calls(built):
    syms = built.abi_symbols()
    L = C.CDLL(built.library_path())
    for s in NEW_CALLS:
        assert s in syms
        assert hasattr(L, s)
    header = open(os.path.join(ROOT, "include", "cfrk_abi.h")).read()
    for name, value in (("CFRK_BULGE_MAX_HOPS", 64), ("CFRK_BULGE_MAX_VISITS", 65536)):
        m = re.search(r"#define %s\s+(\d+)\b" % name, header)
        assert m and int(m.group(1)) == getattr(built, name) == value
    assert (gr.MAX_HOPS, gr.MAX_VISITS) == (64, 65536)
    for text in ("Unitig bulges", "ranks strictly above the arm", "disjoint from tip[]", "popped here or undecided",
                 "max_hops = 0 pops nothing", "visits[j] = max_visits + 1", "decides the same"):
        assert re.sub(r"\s+\*?\s*", " ", text) in re.sub(r"\s+\*?\s*", " ", header), text
    for name in ("unitig_bulges", "unitig_bulges_device", "simplify"):
        assert callable(getattr(built.GlobalCounter, name))
    assert built.BULGE_STATS_DTYPE.itemsize == 24 and built.BULGE_STATS_DTYPE.names == ("arms", "popped", "undecided")
    for doc in (built.GlobalCounter.unitig_bulges.__doc__, built.GlobalCounter.simplify.__doc__):
        assert "1024" in doc and "not a measured optimum" in doc


# ------------------------------------------------------------------ the reference on graphs one can draw

@pytest.mark.parametrize("canonical", [False, True])
def test_hand_made_graphs(canonical):
    names = set()
    for name, units, ptr, rows, params, popped in hand_cases(canonical):
        pop, visits, path_ptr, path, stats = gr.bulges(units, ptr, rows, canonical, *params)      # (asserts the header's properties)
        assert set(np.flatnonzero(pop).tolist()) == popped, (name, params)
        assert stats[1] == len(popped) and path_ptr[-1] == len(path)
        rec = records(units)
        again = gr.bulges_rows(rec, ptr, rows, canonical, *params)                                  # the bare statement agrees
        assert all(a.tolist() == b.tolist() for a, b in zip(again[:4], (pop, visits, path_ptr, path))) and again[4] == stats
        names.add(name)
    assert len(names) >= (16 if canonical else 14)


def test_the_search_order_and_its_count():
    """S -> {arm, 3}, 3 -> 4, 4 -> T.  The search looks at S -> arm (itself: skipped), S -> 3 (descends), 3 -> 4 (descends) and
    4 -> T (found): 4 links.  With a dead end 5 listed in front of 3 in S's row it looks at two more: S -> 5 and 5's one
    link; listed behind 3 it is never looked at."""
    n, kc = [5, 5, 4, 2, 2, 1, 9], [50, 50, 4, 6, 6, 3, 90]
    base = [(0, 2), (2, 1)]
    chain = [(3, 4), (4, 1), (5, 6)]
    for canonical in (False, True):
        for first, visits in (([(0, 5), (0, 3)], 6), ([(0, 3), (0, 5)], 4)):
            ptr, rows = rows_of(7, P(*(base + first + chain)), canonical)
            pop, v, path_ptr, path, stats = gr.bulges(units_of(n, kc), ptr, rows, canonical, 4, 0, 4, 1024, 0)
            assert pop.tolist() == [0, 0, 1, 0, 0, 0, 0] and v[2] == visits
            assert path.tolist() == [3 << 1, 4 << 1] and path_ptr.tolist() == [0, 0, 0, 2, 2, 2, 2, 2]
            # the budget: exactly `visits` links are enough, one fewer leaves the arm undecided
            assert gr.bulges(units_of(n, kc), ptr, rows, canonical, 4, 0, 4, visits, 0)[0][2] == 1
            short = gr.bulges(units_of(n, kc), ptr, rows, canonical, 4, 0, 4, visits - 1, 0)
            assert short[0][2] == 0 and short[1][2] == visits and short[4][2] >= 1


@pytest.mark.parametrize("canonical", [False, True])
def test_the_ladder(canonical):
    units, ptr, rows = ladder(6, canonical)
    assert len(units) == 21
    pop, visits, _, _, stats = gr.bulges(units, ptr, rows, canonical, 14, 0, 12, 64, 0)
    assert pop[2] == 0 and visits[2] == 65 and stats[2] == 1
    pop, visits, _, _, stats = gr.bulges(units, ptr, rows, canonical, 14, 0, 12, 65536, 0)
    assert pop[2] == 0 and 64 < visits[2] <= 65536 and stats[2] == 0
    # two k-mers more on the way and the first way through is the path
    units[3] = ("", 9, 3, False)
    pop, visits, path_ptr, path, _ = gr.bulges(units, ptr, rows, canonical, 14, 0, 12, 64, 0)
    assert pop[2] == 1 and path_ptr[3] - path_ptr[2] == 12


# ------------------------------------------------------------------ invariants on random inputs, the GPU tests' inputs

@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [4, 12, 21])
def test_reference_invariants(k, canonical):
    rng = np.random.default_rng(2900 + 2 * k + canonical)
    for _ in range(6):
        table = {}
        for s in _random_input(rng, k):
            ur.count_kmers([s], k, canonical, int(rng.integers(1, 4)), table)
        units, link_ptr, links = tr.graph(table, k, canonical)
        for params in ((k, 0, k, 1024, 0), (k, 1, 3, 64, 0), (3 * k, 2, 64, 16, 512), (k, 1, 64, 0, 0)):
            gr.bulges(units, link_ptr, links, canonical, *params)           # (asserts the header's properties)
        assert not gr.bulges(units, link_ptr, links, canonical, 0, 0, 8, 1024, 0)[0].any()
        assert not gr.bulges(units, link_ptr, links, canonical, k, 0, 0, 1024, 0)[0].any()
        final, report, reduced, rows, bulges = gr.simplify(table, k, canonical, 1, rounds=len(units) + 1, tip_max_kmers=3 * k, tip_ratio_q8=0,
                                                           bubble_max_kmers=3 * k, bubble_max_diff=2, bulge_max_kmers=3 * k, bulge_max_diff=2)
        assert report[-1][1:4] == (0, 0, 0) and report[-1][4] == len(table) - len(reduced)
        assert [u[0] for u in final] == [u[0] for u in ur.unitigs(reduced, k, canonical)]
        assert len(rows) == sum(r[2] for r in report) and len(bulges) == sum(r[3] for r in report)


@pytest.mark.parametrize("min_count", [1, 2])
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [5, 15, 21, 31, 33, 63])
def test_the_real_inputs_have_chains_and_no_undecided_arm(k, canonical, min_count):
    genome, cov, length, _ = real_input(k, canonical, min_count)
    assert 300 <= genome <= 1500 and 30 <= cov <= 40
    _, units, ptr, rows = real_graph(k, canonical, min_count)
    pop, visits, path_ptr, path, stats = gr.bulges(units, ptr, rows, canonical, k, 1, min(k + 1, 64), 1024, 0)
    assert stats[2] == 0 and (np.diff(path_ptr) >= 2).any()
    bpop = br.bubbles(units, ptr, rows, canonical, k, 1, 0)[0]
    assert not (bpop & ~pop).any()


def test_the_fuzz_inputs_pop_and_run_out_of_budget():
    for canonical in (False, True):
        rng = np.random.default_rng(31 + canonical)
        popped = undecided = 0
        for _ in range(100):
            rec, ptr, rows, params = fuzz_case(rng, canonical)
            assert len(rec) <= 200
            want = gr.bulges_rows(rec, ptr, rows, canonical, *params)
            popped, undecided = popped + want[4][1], undecided + want[4][2]
        assert popped > 20 and undecided > 20


def test_the_loop_and_the_report_text():
    k, canonical, min_count = 15, True, 1
    table = real_graph(k, canonical, min_count)[0]
    units, report, reduced, rows, bulges = gr.simplify(table, k, canonical, min_count, rounds=3, bubble_max_diff=1, bulge_max_diff=1)
    assert len(report) >= 2 and report[0][3] >= 50 and len(bulges) == sum(r[3] for r in report)
    assert gr.report_text(report).splitlines()[0] == ("1\t%d\t%d\t%d\t%d\t%d" % report[0]).encode()
    for rnd, j, path, (seq, kc, n, circ), spelled in bulges:
        assert len(path) >= 1 and abs(len(spelled) - len(seq)) <= 1 and spelled[:k - 1] != "" and not circ
    # bulges off: the bubble loop's numbers
    units2, report2, reduced2, rows2, none = gr.simplify(table, k, canonical, min_count, bulges_=False, rounds=3, bubble_max_diff=1)
    want = br.simplify(table, k, canonical, min_count, rounds=3, bubble_max_diff=1)
    assert (units2, reduced2, rows2, none) == (want[0], want[2], want[3], []) and [r[:3] + r[4:] for r in report2] == want[1]
    assert len(units) < len(units2)                                     # the chains were what was left


# ------------------------------------------------------------------ the kernels' resources

def test_bulge_kernels_use_no_scratch(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path / "unitig_bulges.hip.s"
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(CSRC, "unitig_bulges.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()
    names = []
    for name, ops, size in _functions(text):
        if not re.search(r"\du[gt]_[a-z_]+_kernel", name):          # (the library scan is not this project's kernel)
            continue
        names.append(name)
        assert ops == 0, f"{name} has {ops} scratch instructions"
        assert not size, f"{name} reserves {size} bytes of scratch per thread"
    for kern, n in {"ut_check_kernel": 2, "ut_indeg_kernel": 1, "ut_in_fill_kernel": 1, "ug_arm_list_kernel": 2, "ug_bulge_search_kernel": 2,
                    "ug_bulge_fill_kernel": 2}.items():
        assert sum(kern in x for x in names) == n, kern
    # the stack of 64 levels x 64 lanes x (4 + 1) bytes is the search kernels' LDS
    lds = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.amdhsa_kernel (\S+).*?\.amdhsa_group_segment_fixed_size (\d+)", text, re.S)}
    for name, size in lds.items():
        if "ug_bulge_search_kernel" in name or "ug_bulge_fill_kernel" in name:
            assert size == 64 * 64 * 5, (name, size)


# ------------------------------------------------------------------ the formatter, the host check, the CLI's refusals

@pytest.fixture(scope="module")
def host():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host"), "../libcfrk_host.so"], stdout=subprocess.DEVNULL)
    L = C.CDLL(os.path.join(ROOT, "cfrk_amd", "libcfrk_host.so"))
    vp = C.c_void_p
    L.cfrk_host_format_bulges.argtypes = [C.c_uint32, vp, vp, vp, vp, C.c_int64, vp, vp, vp, C.c_int, C.c_char_p, C.c_size_t]
    L.cfrk_host_format_bulges.restype = C.c_size_t
    return L


@pytest.fixture(scope="module")
def cli(built):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "cfrk_amd", "cfrk")


def _format(L, rnd, units, k, pop, path_ptr, path):
    data, start, length, rec = ur.layout(units)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if len(a) else None
    args = (rnd, vp(data), vp(start), vp(length), vp(rec), len(units), vp(pop), vp(path_ptr), vp(path), k)
    n = L.cfrk_host_format_bulges(*args, None, 0)
    buf = C.create_string_buffer(n + 1)
    assert L.cfrk_host_format_bulges(*args, buf, n) == n
    assert buf.raw[n:] == b"\0"                                  # nothing behind the size it asked for
    return buf.raw[:n]


def test_bulge_report_formatter(host):
    lines, kinds, hops = 0, set(), set()
    for k, canonical, min_count in ((15, False, 1), (15, True, 1), (31, True, 1), (33, False, 1), (63, True, 1), (5, True, 2)):
        _, units, ptr, rows = real_graph(k, canonical, min_count)
        for rnd, params in ((1, (k, 1, min(k + 1, 64), 1024, 0)), (4000000000, (k, 0, 8, 64, 300))):
            pop, _, path_ptr, path, _ = gr.bulges(units, ptr, rows, canonical, *params)
            want_rows = []
            for j in np.flatnonzero(pop).tolist():
                p = path[path_ptr[j]:path_ptr[j + 1]].tolist()
                want_rows.append((rnd, j, p, units[j], gr.spell(units, p, k)))
                hops.add(len(p))
            want = gr.bulge_lines(want_rows, k)
            assert _format(host, rnd, units, k, pop, path_ptr, path) == want
            lines += want.count(b"\n")
            kinds |= {l.split(b"\t")[7] for l in want.splitlines()}
    assert lines > 150 and kinds >= {b"snp", b"indel"} and len(hops) > 5 and 1 in hops
    # by hand, k = 3: ACGTT beside >1<2 = ACG + (rc(AACG) = CGTT)[2:] = ACGTT ... and one base off
    units = [("ACGAT", 7, 3, False), ("ACG", 6, 1, False), ("AACG", 9, 2, False)]
    pop, path_ptr, path = np.array([1, 0, 0], np.uint8), np.array([0, 2, 2, 2], np.int64), np.array([1 << 1, 2 << 1 | 1], np.uint32)
    assert _format(host, 2, units, 3, pop, path_ptr, path) == b"2\t0\t5\t2.3\t2\t3\t>1<2\tsnp\tACGAT\tACGTT\n"
    assert gr.bulge_lines([(2, 0, path.tolist(), units[0], gr.spell(units, path.tolist(), 3))], 3) == b"2\t0\t5\t2.3\t2\t3\t>1<2\tsnp\tACGAT\tACGTT\n"
    units[0] = ("AGGAT", 7, 3, False)                             # two bases off: mnp
    assert _format(host, 2, units, 3, pop, path_ptr, path) == b"2\t0\t5\t2.3\t2\t3\t>1<2\tmnp\tAGGAT\tACGTT\n"
    assert _format(host, 1, [], 3, np.zeros(0, np.uint8), np.zeros(1, np.int64), np.zeros(0, np.uint32)) == b""


def test_host_check_program_under_sanitizers(tmp_path):
    """tools/bulges_host_check.cpp: the formatter into buffers of exactly the size it asked for, under ASan and UBSan"""
    exe = tmp_path / "bulges_host_check"
    # (the runtimes linked into the program itself: it is a stand-alone program, whatever else the process loads)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-o", str(exe), os.path.join(ROOT, "tools", "bulges_host_check.cpp"),
                           os.path.join(ROOT, "cfrk_amd", "host", "cfrk_host.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "formatter and restatement agree" in p.stdout


G = ["--global", "--unitigs-gfa", "g.gfa"]
NEED = b"--bulge-max-kmers, --bulge-max-diff, --bulge-max-hops, --bulge-max-visits, --bulge-ratio and --bulge-report need --unitigs-pop-bulges"


@pytest.mark.parametrize("args, msg", [
    (["--global", "--unitigs-pop-bulges"], b"--unitigs-pop-bulges needs --unitigs-out UFILE, --unitigs-gfa GFILE or --unitigs-map QFILE"),
    (G + ["--bulge-max-kmers", "5"], NEED),
    (G + ["--bulge-max-diff", "1"], NEED),
    (G + ["--bulge-max-hops", "5"], NEED),
    (G + ["--bulge-max-visits", "100"], NEED),
    (G + ["--bulge-ratio", "1.5"], NEED),
    (G + ["--bulge-report", "b.tsv"], NEED),
    (G + ["--unitigs-pop-bubbles", "--bulge-report", "b.tsv"], NEED),
    (G + ["--unitigs-pop-bulges", "--bubble-max-diff", "1"], b"need --unitigs-pop-bubbles"),
    (G + ["--simplify-rounds", "2"], b"--bubble-report and --simplify-rounds need --unitigs-pop-bubbles"),
    (G + ["--unitigs-pop-bulges", "--unitigs-clip-tips", "--tip-rounds", "2"], b"with --unitigs-pop-bulges the rounds are set by --simplify-rounds N"),
    (G + ["--unitigs-pop-bulges", "--tip-ratio", "1.5"], b"need --unitigs-clip-tips"),
    (G + ["--unitigs-pop-bulges", "--bulge-ratio", "257"], b"--bulge-ratio needs a number from 0 to 256"),
    (G + ["--unitigs-pop-bulges", "--bulge-max-kmers", "0"], b"--bulge-max-kmers needs a count"),
    (G + ["--unitigs-pop-bulges", "--bulge-max-hops", "0"], b"--bulge-max-hops needs a count"),
    (G + ["--unitigs-pop-bulges", "--bulge-max-hops", "65"], b"--bulge-max-hops needs a count from 1 to 64"),
    (G + ["--unitigs-pop-bulges", "--bulge-max-visits", "65537"], b"--bulge-max-visits needs a count from 0 to 65536"),
    (G + ["--unitigs-pop-bulges", "--bulge-max-diff", "x"], b"--bulge-max-diff needs a count"),
    (G + ["--unitigs-pop-bulges", "--bulge-report"], b"--bulge-report needs a value"),
    (["--unitigs-gfa", "g.gfa", "--unitigs-pop-bulges"], b"--unitigs-gfa needs --global"),
])
def test_cli_refuses_bad_bulge_options_before_reading_input(cli, tmp_path, args, msg):
    out = tmp_path / "o.txt"
    p = subprocess.run([cli, str(tmp_path / "missing.fasta"), str(out), "15"] + args, cwd=tmp_path, capture_output=True, timeout=60)
    assert p.returncode == 1
    assert msg in p.stderr
    assert not out.exists() and not (tmp_path / "g.gfa").exists() and not (tmp_path / "b.tsv").exists()


@pytest.mark.parametrize("args", [
    G + ["--unitigs-pop-bulges", "--simplify-rounds", "2", "--tip-report", "r.tsv", "--bulge-max-hops", "64", "--bulge-max-visits", "65536"],
    G + ["--unitigs-pop-bulges", "--unitigs-pop-bubbles", "--unitigs-clip-tips", "--bulge-report", "b.tsv", "--bubble-report", "c.tsv"],
])
def test_cli_accepts_the_bulge_options(cli, tmp_path, args):
    """these pass every rule between options: what is refused is the input that is not there"""
    p = subprocess.run([cli, str(tmp_path / "missing.fasta"), str(tmp_path / "o.txt"), "15"] + args, cwd=tmp_path, capture_output=True, timeout=60)
    assert p.returncode != 0 and b"needs" not in p.stderr and b"need " not in p.stderr and b"missing.fasta" in p.stderr
