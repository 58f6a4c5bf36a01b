"""CPU-side checks of the unitig positions and read hits: the C ABI declares and exports the six calls, the two structs
have the documented sizes and offsets (compiled in C), the Python mirror exists; the plain-Python reference of
tests/read_hits_ref.py keeps its invariants on the unitig tests' k grid and gives the hand-worked answers; the GAF
formatter of libcfrk_host.so against the reference text; the host-check program under the sanitizers; the CLI's refusals;
the kernels of unitig_locate.hip use no scratch memory."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from . import read_hits_ref as hr
from . import unitig_ref as ur
from .test_kernel_resources import CSRC, HIPCC, ROOT, _functions
from .test_unitigs_cpu import _rand, _random_input

HIT_CALLS = ("cfrk_global_unitig_index", "cfrk_global_unitig_index_device", "cfrk_global_locate", "cfrk_global_locate_device",
             "cfrk_global_read_hits", "cfrk_global_read_hits_device")


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
    L.cfrk_host_format_gaf.argtypes = [vp, C.c_int64, vp, vp, vp, C.c_int, C.c_char_p, C.c_size_t]
    L.cfrk_host_format_gaf.restype = C.c_size_t
    return L


@pytest.fixture(scope="module")
def cli(built):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "cfrk_amd", "cfrk")


# ------------------------------------------------------------------ the boundary

def test_abi_declares_and_exports_the_hit_calls(built):
    syms = built.abi_symbols()
    L = C.CDLL(built.library_path())
    for s in HIT_CALLS:
        assert s in syms
        assert hasattr(L, s)
    header = open(os.path.join(ROOT, "include", "cfrk_abi.h")).read()
    m = re.search(r"#define CFRK_POS_NONE\s+(0x[0-9a-fA-F]+|\d+)\b", header)
    assert m and int(m.group(1), 0) == built.CFRK_POS_NONE == hr.POS_NONE == 0xFFFFFFFF
    assert re.search(r"#define CFRK_ABI_VERSION\s+1\b", header)
    dt = built.UNITIG_POS_DTYPE
    assert dt == hr.UNITIG_POS_DTYPE and dt.itemsize == 8 and [dt.fields[n][1] for n in ("unitig", "at")] == [0, 4]
    dt = built.READ_HIT_DTYPE
    assert dt == hr.READ_HIT_DTYPE and dt.itemsize == 16
    assert [dt.fields[n][1] for n in ("unitig", "unitig_at", "read_off", "n_windows")] == [0, 4, 8, 12]
    for name in ("unitig_index", "unitig_index_device", "locate", "locate_device", "read_hits", "read_hits_device"):
        assert callable(getattr(built.GlobalCounter, name))


def test_struct_sizes_and_offsets_in_c(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "cfrk_abi.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %zu %zu\\n", sizeof(cfrk_unitig_pos), offsetof(cfrk_unitig_pos, unitig), offsetof(cfrk_unitig_pos, at));\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(cfrk_read_hit), offsetof(cfrk_read_hit, unitig), offsetof(cfrk_read_hit, unitig_at),\n'
                   "         offsetof(cfrk_read_hit, read_off), offsetof(cfrk_read_hit, n_windows));\n"
                   '  printf("%llu\\n", (unsigned long long)CFRK_POS_NONE);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[0] == "8 0 4" and out[1] == "16 0 4 8 12" and out[2] == "4294967295"


# ------------------------------------------------------------------ the reference

def _reads_for(rng, seqs, k):
    """the inputs, their reverse complements, pieces, a read with an N, short reads"""
    reads = list(dict.fromkeys(seqs))
    reads += [ur.rc(s) for s in reads]
    g = seqs[0]
    for _ in range(6):
        a = int(rng.integers(0, len(g)))
        reads.append(g[a:a + int(rng.integers(1, 60))])
    mid = len(g) // 2
    reads += [g[:mid] + "N" + g[mid + 1:], g[:k - 1], "", _rand(rng, 3 * k)]
    return reads


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [3, 4, 12, 13, 21, 32, 33])
def test_reference_invariants(k, canonical):
    """Graph() and hits() assert the contract's consequences themselves; here every solid window is located, in both
    orientations under the canonical rule, and absent keys are not"""
    rng = np.random.default_rng(900 + 2 * k + canonical)
    two_hits_on_a_circle = 0
    for _ in range(6):
        seqs = _random_input(rng, k)
        table = ur.count_kmers(seqs, k, canonical)
        for min_count in (1, 2):
            g = hr.Graph(table, k, canonical, min_count)
            for x in g.solid:
                j, p, minus = g.locate(x)
                assert g.node(g.seqs[j][p:p + k]) == x
                if canonical:
                    r = g.locate(ur.rc(x))
                    assert r[:2] == (j, p) and (r[2] != minus or x == ur.rc(x))
                    if x == ur.rc(x):
                        assert (p, minus) == (0, 0) and len(g.seqs[j]) == k
                else:
                    assert minus == 0
            for x in (_rand(rng, k) for _ in range(20)):
                assert (g.locate(x) is None) == (x not in g.O)
            for r in _reads_for(rng, seqs, k):
                g.hits(r)
            for (s, kc, n, circ) in g.units:
                if circ:                                        # walked twice: the cut splits the walk
                    h = g.hits(s + s[k - 1:])
                    assert [x[3] for x in h] == [n, n] and [x[2] for x in h] == [0, n]
                    two_hits_on_a_circle += 1
    assert two_hits_on_a_circle > 0 or k < 12      # (at k = 3, 4 the random circles rarely survive as circular unitigs)


def test_reference_hand_worked():
    # a minus-strand hit: the canonical 3-mers of AAGTC form the one unitig AAGTC; its reverse complement GACTT spells
    # GAC, ACT, CTT = rc of k-mers 2, 1, 0
    g = hr.Graph(ur.count_kmers(["AAGTC"], 3, True), 3, True)
    assert g.seqs == ["AAGTC"]
    assert g.hits("GACTT") == [(0, 0 << 1 | 1, 0, 3)]
    assert g.hits("AGTC") == [(0, 1 << 1 | 0, 0, 2)]
    assert g.hits("ACTT") == [(0, 0 << 1 | 1, 0, 2)]
    assert g.locate("ACT") == (0, 1, 1) and g.locate("AGT") == (0, 1, 0) and g.locate("TTT") is None
    assert g.gaf_text(["GACTT", "AGTC"]) == b"0\t5\t0\t5\t+\t<0\t5\t0\t5\t5\t5\t255\tcg:Z:5=\n1\t4\t0\t4\t+\t>0\t5\t1\t5\t4\t4\t255\tcg:Z:4=\n"
    # a circle's cut: ACGGTACG closes on itself (5 k-mers, cut at ACG); walked twice it is two hits
    g = hr.Graph(ur.count_kmers(["ACGGTACG"], 3, False), 3, False)
    assert g.units == [("ACGGTAC", 6, 5, True)]
    assert g.hits("ACGGTACGGTAC") == [(0, 0, 0, 5), (0, 0, 5, 5)]
    assert g.hits("GTACGG") == [(0, 3 << 1, 0, 2), (0, 0, 2, 2)]
    # an N: the three windows over it are not located
    assert g.hits("ACGGNGTAC") == [(0, 0, 0, 2), (0, 3 << 1, 5, 2)]
    assert g.hits("AC") == [] and g.hits("") == []
    # a palindrome is a single node: p = 0, minus = 0
    g = hr.Graph(ur.count_kmers(["ACGT"], 4, True), 4, True)
    assert g.seqs == ["ACGT"] and g.locate("ACGT") == (0, 0, 0)
    assert g.hits("AACGTT") == [(0, 0, 1, 1)]
    # a threshold: the key counted once is not in O at 2
    table = ur.count_kmers(["ACGTT", "ACGT"], 4, False)
    assert hr.Graph(table, 4, False, 1).hits("ACGTT") == [(0, 0, 0, 2)]
    assert hr.Graph(table, 4, False, 2).hits("ACGTT") == [(0, 0, 0, 1)]


def test_reference_every_window_its_own_hit():
    """all 256 4-mers counted once: every unitig is one node under both strand rules, so a read has a hit per window"""
    every = ["".join(ur.BASES[(i >> s) & 3] for s in (6, 4, 2, 0)) for i in range(256)]
    rng = np.random.default_rng(4)
    for canonical in (False, True):
        g = hr.Graph(ur.count_kmers(every, 4, canonical), 4, canonical)
        assert all(len(s) == 4 for s in g.seqs) and len(g.seqs) == (136 if canonical else 256)
        r = _rand(rng, 300)
        assert [h[2:] for h in g.hits(r)] == [(w, 1) for w in range(297)]


def test_reference_rows_and_codes():
    g = hr.Graph(ur.count_kmers(["ACGGTACG"], 3, False), 3, False)
    ptr, rows = g.hit_rows(["ACGGNGTAC", "AC", "GTACGG"])
    assert ptr.tolist() == [0, 2, 2, 4] and rows.dtype == hr.READ_HIT_DTYPE
    assert rows.tolist() == [(0, 0, 0, 2), (0, 6, 5, 2), (0, 6, 0, 2), (0, 0, 2, 2)]
    pos = g.locate_rows(["ACG", "TAC", "TTT"])
    assert pos.tolist() == [(0, 0), (0, 8), (hr.POS_NONE, hr.POS_NONE)]
    data, start, length = hr.read_codes(["ACNG", ""])
    assert data.tolist() == [0, 1, -1, 2, -1, -1] and start.tolist() == [0, 5] and length.tolist() == [4, 0]


# ------------------------------------------------------------------ the GAF formatter

def _gaf(L, g, reads):
    ptr, rows = g.hit_rows(reads)
    rl = np.array([len(r) for r in reads], np.int32)
    ul = np.array([len(s) for s in g.seqs], np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if len(a) else None
    args = (vp(rl), len(reads), vp(ptr), vp(rows), vp(ul), g.k)
    n = L.cfrk_host_format_gaf(*args, None, 0)
    buf = C.create_string_buffer(n + 1)
    assert L.cfrk_host_format_gaf(*args, buf, n) == n
    assert buf.raw[n:] == b"\0"                                  # nothing behind the size it asked for
    return buf.raw[:n]


def test_gaf_formatter(host):
    rng = np.random.default_rng(6)
    cases = [(["AAGTC"], 3, True, ["GACTT", "AGTC", "", "TTTT"]), (["ACGGTACG"], 3, False, ["ACGGTACGGTAC", "ACGGNGTAC"])]
    for k, canonical in ((1, False), (1, True), (5, True), (8, False), (21, True), (33, True), (64, False)):
        seqs = _random_input(rng, k)
        cases.append((seqs, k, canonical, _reads_for(rng, seqs, k)))
    lines = 0
    for seqs, k, canonical, reads in cases:
        g = hr.Graph(ur.count_kmers(seqs, k, canonical), k, canonical)
        want = g.gaf_text(reads)
        assert _gaf(host, g, reads) == want
        lines += want.count(b"\n")
    assert lines > 100
    g = hr.Graph(ur.count_kmers(["AAGTC"], 3, True), 3, True)
    assert _gaf(host, g, ["GACTT"]) == b"0\t5\t0\t5\t+\t<0\t5\t0\t5\t5\t5\t255\tcg:Z:5=\n"
    assert _gaf(host, g, []) == b""


def test_host_check_program_under_sanitizers(tmp_path):
    """tools/read_hits_host_check.cpp: the formatter into buffers of exactly the size it asked for, under ASan and UBSan"""
    exe = tmp_path / "read_hits_host_check"
    # (the runtimes linked into the program itself: it is a stand-alone program, whatever else the process loads)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-o", str(exe), os.path.join(ROOT, "tools", "read_hits_host_check.cpp"),
                           os.path.join(ROOT, "cfrk_amd", "host", "cfrk_host.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "formatter and restatement agree" in p.stdout


# ------------------------------------------------------------------ the CLI's refusals, the kernels' resources

@pytest.mark.parametrize("args, msg", [
    (["--unitigs-map", "q.fa", "--unitigs-map-out", "m.gaf"], b"--unitigs-map needs --global"),
    (["--global", "--unitigs-map", "q.fa", "--unitigs-map-out", "m.gaf", "--gpus", "2"], b"--unitigs-map needs --global on one device"),
    (["--global", "--unitigs-map", "q.fa"], b"--unitigs-map QFILE and --unitigs-map-out MFILE go together"),
    (["--global", "--unitigs-map-out", "m.gaf"], b"--unitigs-map QFILE and --unitigs-map-out MFILE go together"),
    (["--global", "--unitigs-map"], b"--unitigs-map needs a value"),
    (["--global", "--unitigs-map", "q.fa", "--unitigs-map-out", "m.gaf", "--unitigs-min-count", "two"], b"--unitigs-min-count needs a count"),
])
def test_cli_refuses_bad_map_options_before_reading_input(cli, tmp_path, args, msg):
    out = tmp_path / "o.txt"
    p = subprocess.run([cli, str(tmp_path / "missing.fasta"), str(out), "15"] + args, cwd=tmp_path, capture_output=True, timeout=60)
    assert p.returncode == 1
    assert msg in p.stderr
    assert not out.exists() and not (tmp_path / "m.gaf").exists()


def test_locate_kernels_use_no_scratch(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path / "unitig_locate.s"
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(CSRC, "unitig_locate.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = []
    for name, ops, size in _functions(out.read_text()):
        if not re.search(r"\d(up_[a-z_]+_kernel|read_hits_kernel|read_hits_long_kernel|rh_finish_kernel)", name):
            continue                                            # (the library scan is not this project's kernel)
        names.append(name)
        assert ops == 0, f"{name} has {ops} scratch instructions"
        assert not size, f"{name} reserves {size} bytes of scratch per thread"
    # three index modes x both strand rules; the hit kernels also count and fill, at two group widths
    for kern, n in (("up_claim_kernel", 6), ("up_cover_kernel", 6), ("up_locate_kernel", 6), ("read_hits_kernel", 24),
                    ("read_hits_long_kernel", 12), ("up_check_kernel", 1), ("rh_finish_kernel", 1)):
        assert sum(kern in x for x in names) == n, kern
