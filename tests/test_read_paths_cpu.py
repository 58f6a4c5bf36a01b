"""CPU-side checks of the read paths and the link support: the C ABI declares and exports the two calls, the two structs
have the documented sizes and offsets (compiled in C), the Python mirror exists; the plain-Python reference of
tests/read_paths_ref.py gives the hand-worked answers (a fork walked on both strands, a circle crossed twice, a hairpin,
an even-k palindromic node, a read with an N in the middle) and keeps the contract's consequences on the unitig tests' k
grid under both strand rules; the two formatters of libcfrk_host.so against the reference texts; the host-check program
under the sanitizers; the CLI's refusals; the kernels of read_paths.hip use no scratch memory.  The reference tests
exercise tests/read_paths_ref.py alone, so they hold whatever the product is; the boundary, formatter, host-check, CLI
and resource tests need the feature."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from . import read_hits_ref as hr
from . import read_paths_ref as pr
from . import unitig_links_ref as ulr
from . import unitig_ref as ur
from .test_kernel_resources import CSRC, HIPCC, ROOT, _functions
from .test_unitigs_cpu import _rand, _random_input

KS = [3, 4, 12, 13, 16, 21, 31, 32, 33, 47, 64]       # the k grid of tests/test_gpu_unitigs.py (importing it would need a device)
PATH_CALLS = ("cfrk_global_read_paths", "cfrk_global_read_paths_device")


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
    L.cfrk_host_format_gaf_paths.argtypes = [vp, C.c_int64, vp, vp, vp, vp, vp, C.c_int, C.c_char_p, C.c_size_t]
    L.cfrk_host_format_gaf_paths.restype = C.c_size_t
    L.cfrk_host_format_gfa_support.argtypes = [vp, vp, vp, vp, C.c_int64, vp, vp, vp, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    L.cfrk_host_format_gfa_support.restype = C.c_size_t
    L.cfrk_host_format_gaf.argtypes = [vp, C.c_int64, vp, vp, vp, C.c_int, C.c_char_p, C.c_size_t]
    L.cfrk_host_format_gaf.restype = C.c_size_t
    return L


@pytest.fixture(scope="module")
def cli(built):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "cfrk_amd", "cfrk")


# ------------------------------------------------------------------ the boundary

def test_abi_declares_and_exports_the_path_calls(built):
    syms = built.abi_symbols()
    L = C.CDLL(built.library_path())
    for s in PATH_CALLS:
        assert s in syms
        assert hasattr(L, s)
    dt = built.READ_PATH_DTYPE
    assert dt == pr.READ_PATH_DTYPE and dt.itemsize == 16
    assert [dt.fields[n][1] for n in ("hit_first", "n_hits", "read_off", "n_windows")] == [0, 4, 8, 12]
    dt = built.PATH_STATS_DTYPE
    assert dt.itemsize == 32 and dt.names == pr.STAT_NAMES and [dt.fields[n][1] for n in dt.names] == [0, 8, 16, 24]
    for name in ("read_paths", "read_paths_device"):
        assert callable(getattr(built.GlobalCounter, name))


def test_struct_sizes_and_offsets_in_c(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "cfrk_abi.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(cfrk_read_path), offsetof(cfrk_read_path, hit_first), offsetof(cfrk_read_path, n_hits),\n'
                   "         offsetof(cfrk_read_path, read_off), offsetof(cfrk_read_path, n_windows));\n"
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(cfrk_path_stats), offsetof(cfrk_path_stats, n_paths), offsetof(cfrk_path_stats, n_steps),\n'
                   "         offsetof(cfrk_path_stats, n_gaps), offsetof(cfrk_path_stats, n_unlinked));\n"
                   "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0] == "16 0 4 8 12" and out[1] == "32 0 8 16 24"


# ------------------------------------------------------------------ the reference, hand-worked

def _case(seqs, k, canonical, reads):
    table = ur.count_kmers(seqs, k, canonical)
    G = hr.Graph(table, k, canonical)
    link_ptr, links = ulr.links(G.units, table, k, canonical)
    return (G, link_ptr, links) + pr.graph_paths(G, link_ptr, links, reads)


TRUNK, ARM_A, ARM_B = "GAAGAGTC", "AGTCATT", "AGTCCAA"       # the arms begin with the trunk's last k - 1 bases
WALK_A, WALK_B = TRUNK + ARM_A[4:], TRUNK + ARM_B[4:]


def test_reference_fork_on_both_strands():
    """a trunk that forks into two arms, k = 5.  Canonical: the unitigs sort as 0 = AATGACT (arm A reverse-complemented),
    1 = AGTCCAA (arm B), 2 = the trunk; rows 0: (0,+)->(2,-); 1: (1,-)->(2,-); 2: (2,+)->(0,-), (2,+)->(1,+)"""
    reads = [WALK_A, ur.rc(WALK_B), WALK_B, ur.rc(WALK_A)]
    G, link_ptr, links, hit_ptr, hits, path_ptr, paths, support, st = _case([TRUNK, ARM_A, ARM_B], 5, True, reads)
    assert G.seqs == ["AATGACT", "AGTCCAA", "GAAGAGTC"]
    assert link_ptr.tolist() == [0, 1, 2, 4] and links.tolist() == [(2, 2), (2, 3), (0, 2), (1, 0)]
    assert hits.tolist() == [(2, 0, 0, 4), (0, 1, 4, 3), (1, 1, 0, 3), (2, 1, 3, 4), (2, 0, 0, 4), (1, 0, 4, 3), (0, 0, 0, 3), (2, 1, 3, 4)]
    assert path_ptr.tolist() == [0, 1, 2, 3, 4] and paths.tolist() == [(0, 2, 0, 7)] * 4
    assert support.tolist() == [1, 1, 1, 1]                     # directional: each read walks its own row
    assert st == {"n_paths": 4, "n_steps": 4, "n_gaps": 0, "n_unlinked": 0}
    lens = [len(s) for s in G.seqs]
    assert pr.gaf_paths_text(lens, 5, [11] * 4, hit_ptr, hits, path_ptr, paths) == (
        b"0\t11\t0\t11\t+\t>2<0\t11\t0\t11\t11\t11\t255\tcg:Z:11=\n1\t11\t0\t11\t+\t<1<2\t11\t0\t11\t11\t11\t255\tcg:Z:11=\n"
        b"2\t11\t0\t11\t+\t>2>1\t11\t0\t11\t11\t11\t255\tcg:Z:11=\n3\t11\t0\t11\t+\t>0<2\t11\t0\t11\t11\t11\t255\tcg:Z:11=\n")
    # a read and its reverse complement tag a link and its mirror alike
    text = pr.gfa_support_text(G.units, 5, link_ptr, links, support, True).decode()
    assert text.endswith("L\t0\t+\t2\t-\t4M\tRC:i:2\nL\t1\t-\t2\t-\t4M\tRC:i:2\nL\t2\t+\t0\t-\t4M\tRC:i:2\nL\t2\t+\t1\t+\t4M\tRC:i:2\n")
    assert pr.gfa_support_text(G.units, 5, link_ptr, links, support, False).decode().count("RC:i:1\n") == 4
    # not canonical: the reverse complement of a walk is not in the graph at all
    G, link_ptr, links, hit_ptr, hits, path_ptr, paths, support, st = _case([TRUNK, ARM_A, ARM_B], 5, False, [WALK_A, WALK_B, ur.rc(WALK_B)])
    assert G.seqs == ["AGTCATT", "AGTCCAA", "GAAGAGTC"] and links.tolist() == [(0, 0), (1, 0)]
    assert path_ptr.tolist() == [0, 1, 2, 2] and paths.tolist() == [(0, 2, 0, 7)] * 2 and support.tolist() == [1, 1]


def test_reference_sub_csr_breaks_the_walks():
    """the fork without the row (2,+)->(0,-): the walk onto arm A breaks there and counts as unlinked"""
    reads = [WALK_A, WALK_B]
    table = ur.count_kmers([TRUNK, ARM_A, ARM_B], 5, True)
    G = hr.Graph(table, 5, True)
    link_ptr, links = ulr.links(G.units, table, 5, True)
    keep = np.array([True, True, False, True])
    sub_ptr = np.array([0, 1, 2, 3], np.int64)
    _, _, path_ptr, paths, support, st = pr.graph_paths(G, sub_ptr, links[keep], reads, complete=False)
    assert path_ptr.tolist() == [0, 2, 3] and paths.tolist() == [(0, 1, 0, 4), (1, 1, 4, 3), (0, 2, 0, 7)]
    assert support.tolist() == [0, 0, 1] and st == {"n_paths": 3, "n_steps": 1, "n_gaps": 0, "n_unlinked": 1}


def test_reference_circle_crossed_twice():
    """ACGGTACG closes on itself (5 3-mers, cut at ACG): a read that goes round it crosses the cut through (0,+)->(0,+)"""
    G, link_ptr, links, hit_ptr, hits, path_ptr, paths, support, st = _case(["ACGGTACG"], 3, False, ["ACGGTACGGTACGG", "GTACGG"])
    assert G.units == [("ACGGTAC", 6, 5, True)] and links.tolist() == [(0, 0)]
    assert hits.tolist() == [(0, 0, 0, 5), (0, 0, 5, 5), (0, 0, 10, 2), (0, 6, 0, 2), (0, 0, 2, 2)]
    assert paths.tolist() == [(0, 3, 0, 12), (0, 2, 0, 4)] and support.tolist() == [3]
    assert st == {"n_paths": 2, "n_steps": 3, "n_gaps": 0, "n_unlinked": 0}
    # PL: three times LN 7 minus two overlaps of 2; ps of the second read: its first hit begins at base 3
    assert pr.gaf_paths_text([7], 3, [14, 6], hit_ptr, hits, path_ptr, paths) == (
        b"0\t14\t0\t14\t+\t>0>0>0\t17\t0\t14\t14\t14\t255\tcg:Z:14=\n1\t6\t0\t6\t+\t>0>0\t12\t3\t9\t6\t6\t255\tcg:Z:6=\n")


def test_reference_hairpin():
    """AACGT + its reverse complement, k = 5: the walk turns round through (1,+)->(1,-)"""
    h = "AACGT"
    G, link_ptr, links, hit_ptr, hits, path_ptr, paths, support, st = _case([h + ur.rc(h)], 5, True, [h + ur.rc(h)])
    assert G.seqs == ["AACGT", "ACGTAC"]
    assert links.tolist() == [(1, 0), (0, 2), (1, 2), (1, 1), (0, 3)]
    assert hits.tolist() == [(0, 0, 0, 1), (1, 0, 1, 2), (1, 1, 3, 2), (0, 1, 5, 1)]
    assert paths.tolist() == [(0, 4, 0, 6)] and support.tolist() == [1, 0, 1, 0, 1]
    # (1,+)->(1,-) is its own mirror: counted once; (0,+)->(1,+) and its mirror (1,-)->(0,-) share 2
    text = pr.gfa_support_text(G.units, 5, link_ptr, links, support, True).decode()
    assert "L\t1\t+\t1\t-\t4M\tRC:i:1\n" in text and "L\t0\t+\t1\t+\t4M\tRC:i:2\n" in text and "L\t1\t-\t0\t-\t4M\tRC:i:2\n" in text


def test_reference_even_k_palindromic_node():
    """ACGT at k = 4 is a single-node unitig that is always entered and left as (0,+): a read and its reverse complement
    use different rows that are not each other's mirrors"""
    G, link_ptr, links, hit_ptr, hits, path_ptr, paths, support, st = _case(["TTACGTCC"], 4, True, ["TTACGTCC", "GGACGTAA"])
    assert G.seqs == ["ACGT", "CGTAA", "CGTCC"]
    assert hits.tolist() == [(1, 1, 0, 2), (0, 0, 2, 1), (2, 0, 3, 2), (2, 1, 0, 2), (0, 0, 2, 1), (1, 0, 3, 2)]
    assert paths.tolist() == [(0, 3, 0, 5), (0, 3, 0, 5)] and st["n_steps"] == 4 and st["n_unlinked"] == 0
    assert links.tolist() == [(1, 0), (2, 0), (1, 1), (2, 1), (0, 1), (0, 3), (0, 1), (0, 3)]
    assert support.tolist() == [1, 1, 0, 0, 1, 0, 1, 0]          # (0,-) is never left, (0,-) never entered


def test_reference_read_with_an_n():
    """the windows over the N are not located: two paths and a gap between them"""
    G, link_ptr, links, hit_ptr, hits, path_ptr, paths, support, st = _case([TRUNK, ARM_A, ARM_B], 5, True, ["GAAGANTCATT", "ACGTN", ""])
    assert hits.tolist() == [(2, 0, 0, 1), (0, 1, 6, 1)] and hit_ptr.tolist() == [0, 2, 2, 2]
    assert path_ptr.tolist() == [0, 2, 2, 2] and paths.tolist() == [(0, 1, 0, 1), (1, 1, 6, 1)]
    assert st == {"n_paths": 2, "n_steps": 0, "n_gaps": 1, "n_unlinked": 0} and not support.any()
    assert pr.stats_text(3, 2, st) == b"3\t2\t2\t0\t1\t0\n"


def test_reference_accumulates_into_support():
    G, link_ptr, links, hit_ptr, hits, _, _, support, st = _case([TRUNK, ARM_A, ARM_B], 5, True, [WALK_A, WALK_A, WALK_B])
    n_kmers = [len(s) - 4 for s in G.seqs]
    again = pr.path_rows(hit_ptr, hits, n_kmers, link_ptr, links, support)[2]
    assert support.tolist() == [0, 0, 2, 1] and again.tolist() == [0, 0, 4, 2]


# ------------------------------------------------------------------ the reference, its consequences on the grid

def _reads_for(rng, G, seqs, k):
    """the inputs and their reverse complements, every circle walked 2.5 times, pieces, an N, short reads, noise"""
    reads = list(dict.fromkeys(seqs))
    reads += [ur.rc(s) for s in reads]
    for s, _, n, circ in G.units:
        if circ:
            reads.append(s + (s[k - 1:] * 2)[:n + n // 2])
    g = seqs[0]
    for _ in range(6):
        a = int(rng.integers(0, len(g)))
        reads.append(g[a:a + int(rng.integers(1, 3 * k + 60))])
    mid = len(g) // 2
    reads += [g[:mid] + "N" + g[mid + 1:], g[:k - 1], "", _rand(rng, 3 * k)]
    return reads


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", KS)
def test_reference_consequences(k, canonical):
    """graph_paths() asserts them: every path spells its stretch of the read; on the complete link set nothing is
    unlinked and a read's paths are its maximal runs of located windows; the support sums to the steps"""
    rng = np.random.default_rng(1300 + 2 * k + canonical)
    steps = paths = 0
    for _ in range(3):
        seqs = _random_input(rng, k)
        table = ur.count_kmers(seqs, k, canonical)
        for min_count in (1, 2):
            G = hr.Graph(table, k, canonical, min_count)
            link_ptr, links = ulr.links(G.units, table, k, canonical, min_count)
            reads = _reads_for(rng, G, seqs, k)
            _, hits, _, prow, support, st = pr.graph_paths(G, link_ptr, links, reads)
            steps += st["n_steps"]
            paths += st["n_paths"]
            # every third row removed: the walks break there and nowhere else
            keep = np.ones(len(links), bool)
            keep[::3] = False
            sub_ptr = np.concatenate([[0], np.cumsum(keep)])[link_ptr]
            _, _, _, _, sub, st2 = pr.graph_paths(G, sub_ptr, links[keep], reads, complete=False)
            assert (sub == support[keep]).all()
            assert st2["n_unlinked"] == int(support[~keep].sum()) and st2["n_gaps"] == st["n_gaps"]
            assert st2["n_paths"] == st["n_paths"] + st2["n_unlinked"]
    assert paths > 20 and (steps > 0 or k > 40)


# ------------------------------------------------------------------ the formatters

def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if len(a) else None


def _format(fn, args):
    n = fn(*args, None, 0)
    buf = C.create_string_buffer(n + 1)
    assert fn(*args, buf, n) == n
    assert buf.raw[n:] == b"\0"                                  # nothing behind the size it asked for
    return buf.raw[:n]


def _texts(L, G, link_ptr, links, reads, canonical):
    hit_ptr, hits, path_ptr, prow, support, st = pr.graph_paths(G, link_ptr, links, reads)
    rl = np.array([len(r) for r in reads], np.int32)
    data, start, length, rec = ur.layout(G.units)
    gaf = _format(L.cfrk_host_format_gaf_paths, (_vp(rl), len(reads), _vp(hit_ptr), _vp(hits), _vp(path_ptr), _vp(prow), _vp(length), G.k))
    links = np.ascontiguousarray(links)
    gfa = _format(L.cfrk_host_format_gfa_support, (_vp(data), _vp(start), _vp(length), _vp(rec), len(G.units), _vp(link_ptr), _vp(links),
                                                   _vp(support) if len(support) else _vp(np.zeros(1, np.uint32)), int(canonical), G.k))
    assert gaf == pr.gaf_paths_text([len(s) for s in G.seqs], G.k, [len(r) for r in reads], hit_ptr, hits, path_ptr, prow)
    assert gfa == pr.gfa_support_text(G.units, G.k, link_ptr, links, support, canonical)
    # without the tags: the GFA as it was
    assert re.sub(rb"\tRC:i:\d+\n", b"\n", gfa) == ulr.gfa_text(G.units, G.k, link_ptr, links)
    # every hit a path of its own: the lines of the hit formatter
    one = np.zeros(len(hits), pr.READ_PATH_DTYPE)
    one["hit_first"] = np.arange(len(hits)) - np.repeat(hit_ptr[:-1], np.diff(hit_ptr))
    one["n_hits"], one["read_off"], one["n_windows"] = 1, hits["read_off"], hits["n_windows"]
    assert _format(L.cfrk_host_format_gaf_paths, (_vp(rl), len(reads), _vp(hit_ptr), _vp(hits), _vp(hit_ptr), _vp(one), _vp(length), G.k)) == \
        G.gaf_text(reads) == _format(L.cfrk_host_format_gaf, (_vp(rl), len(reads), _vp(hit_ptr), _vp(hits), _vp(length), G.k))
    return gaf, gfa, st


def test_formatters_against_the_reference(host):
    rng = np.random.default_rng(16)
    cases = [([TRUNK, ARM_A, ARM_B], 5, True), (["ACGGTACG"], 3, False), (["AACGTACGTT"], 5, True), (["TTACGTCC"], 4, True)]
    for k, canonical in ((2, False), (4, True), (5, True), (8, False), (21, True), (33, True), (64, False)):
        cases.append((_random_input(rng, k), k, canonical))
    lines = tagged = 0
    for seqs, k, canonical in cases:
        table = ur.count_kmers(seqs, k, canonical)
        G = hr.Graph(table, k, canonical)
        link_ptr, links = ulr.links(G.units, table, k, canonical)
        gaf, gfa, st = _texts(host, G, link_ptr, links, _reads_for(rng, G, seqs, k), canonical)
        lines += gaf.count(b"\n")
        tagged += len(re.findall(rb"RC:i:[1-9]", gfa))
        assert gaf.count(b"\n") == st["n_paths"]
    assert lines > 100 and tagged > 50
    # the hand-worked lines, and nothing at all
    table = ur.count_kmers([TRUNK, ARM_A, ARM_B], 5, True)
    G = hr.Graph(table, 5, True)
    link_ptr, links = ulr.links(G.units, table, 5, True)
    gaf, gfa, _ = _texts(host, G, link_ptr, links, [WALK_A, ur.rc(WALK_A)], True)
    assert gaf == b"0\t11\t0\t11\t+\t>2<0\t11\t0\t11\t11\t11\t255\tcg:Z:11=\n1\t11\t0\t11\t+\t>0<2\t11\t0\t11\t11\t11\t255\tcg:Z:11=\n"
    assert gfa.endswith(b"L\t0\t+\t2\t-\t4M\tRC:i:2\nL\t1\t-\t2\t-\t4M\tRC:i:0\nL\t2\t+\t0\t-\t4M\tRC:i:2\nL\t2\t+\t1\t+\t4M\tRC:i:0\n")
    assert _texts(host, G, link_ptr, links, [], True)[0] == b""


def test_host_check_program_under_sanitizers(tmp_path):
    """tools/read_paths_host_check.cpp: both formatters into buffers of exactly the size they asked for, under ASan and UBSan"""
    exe = tmp_path / "read_paths_host_check"
    # (the runtimes linked into the program itself: it is a stand-alone program, whatever else the process loads)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-o", str(exe), os.path.join(ROOT, "tools", "read_paths_host_check.cpp"),
                           os.path.join(ROOT, "cfrk_amd", "host", "cfrk_host.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "formatters and restatement agree" in p.stdout


# ------------------------------------------------------------------ the CLI's refusals, the kernels' resources

@pytest.mark.parametrize("args, msg", [
    (["--global", "--unitigs-gfa", "g.gfa", "--unitigs-map-paths"], b"--unitigs-map-paths needs --unitigs-map QFILE"),
    (["--global", "--unitigs-map", "q.fa", "--unitigs-map-out", "m.gaf", "--unitigs-link-support"],
     b"--unitigs-link-support needs --unitigs-map QFILE and --unitigs-gfa GFILE"),
    (["--global", "--unitigs-gfa", "g.gfa", "--unitigs-link-support"], b"--unitigs-link-support needs --unitigs-map QFILE and --unitigs-gfa GFILE"),
    (["--global", "--unitigs-out", "u.fa", "--unitigs-map-stats", "s.txt"], b"--unitigs-map-stats needs --unitigs-map QFILE"),
    (["--global", "--unitigs-map", "q.fa", "--unitigs-map-out", "m.gaf", "--unitigs-map-stats"], b"--unitigs-map-stats needs a value"),
])
def test_cli_refuses_bad_path_options_before_reading_input(cli, tmp_path, args, msg):
    out = tmp_path / "o.txt"
    p = subprocess.run([cli, str(tmp_path / "missing.fasta"), str(out), "15"] + args, cwd=tmp_path, capture_output=True, timeout=60)
    assert p.returncode == 1
    assert msg in p.stderr
    assert not any((tmp_path / f).exists() for f in ("o.txt", "m.gaf", "g.gfa", "s.txt", "u.fa"))


def test_read_paths_kernels_use_no_scratch(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path / "read_paths.s"
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(CSRC, "read_paths.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = []
    for name, ops, size in _functions(out.read_text()):
        if not re.search(r"\d(rp_[a-z_]+_kernel|ut_[a-z_]+_kernel)", name):
            continue                                            # (the library scan is not this project's kernel)
        names.append(name)
        assert ops == 0, f"{name} has {ops} scratch instructions"
        assert not size, f"{name} reserves {size} bytes of scratch per thread"
    for kern, n in (("rp_mark_kernel", 1), ("rp_hits_kernel", 1), ("rp_join_kernel", 1), ("rp_rows_kernel", 1), ("rp_events_kernel", 1),
                    ("rp_finish_kernel", 1), ("ut_check_kernel", 2)):
        assert sum(kern in x for x in names) == n, kern
