"""CPU-side checks of the unitig feature: the C ABI declares and exports the calls, cfrk_unitig is 16 bytes with the
documented offsets, the Python mirror exists; the plain-Python reference of tests/unitig_ref.py keeps its invariants on
random inputs (every solid key in exactly one unitig, once; first k-mers distinct and ascending) and gives the
hand-worked answers; the FASTA formatter of libcfrk_host.so; the CLI's refusals; the kernels of unitigs.hip use no
scratch memory."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from . import unitig_ref as ur
from .test_kernel_resources import CSRC, HIPCC, ROOT, _functions

UNITIG_CALLS = ("cfrk_global_neighbors", "cfrk_global_neighbors_device", "cfrk_global_unitigs", "cfrk_global_unitigs_device")


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
    L.cfrk_host_format_unitigs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_char_p, C.c_size_t]
    L.cfrk_host_format_unitigs.restype = C.c_size_t
    return L


@pytest.fixture(scope="module")
def cli(built):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "cfrk_amd", "cfrk")


def test_abi_declares_and_exports_the_unitig_calls(built):
    syms = built.abi_symbols()
    L = C.CDLL(built.library_path())
    for s in UNITIG_CALLS:
        assert s in syms
        assert hasattr(L, s)
    header = open(os.path.join(ROOT, "include", "cfrk_abi.h")).read()
    for name in ("CFRK_UNITIG_CIRCULAR", "CFRK_UNITIG_SPLIT_LOG2_DEFAULT", "CFRK_PARAM_UNITIG_SPLIT_LOG2"):
        m = re.search(r"#define %s\s+(0x[0-9a-fA-F]+|\d+)\b" % name, header)
        assert m and int(m.group(1), 0) == getattr(built, name), name
    assert (built.CFRK_UNITIG_CIRCULAR, built.CFRK_PARAM_UNITIG_SPLIT_LOG2) == (1, 4)
    assert re.search(r"uint64_t kc;.*uint32_t n_kmers;.*uint32_t flags;.*\} cfrk_unitig;", header, re.S)
    dt = built.UNITIG_DTYPE
    assert dt.itemsize == 16 and [dt.fields[n][1] for n in ("kc", "n_kmers", "flags")] == [0, 8, 12]
    assert dt == ur.UNITIG_DTYPE
    for name in ("neighbors", "neighbors_device", "unitigs", "unitigs_device"):
        assert callable(getattr(built.GlobalCounter, name))


# ------------------------------------------------------------------ the reference: invariants

def _rand(rng, n):
    return "".join(ur.BASES[i] for i in rng.integers(0, 4, n))


def _random_input(rng, k):
    g = _rand(rng, int(rng.integers(20, 400)))
    seqs = [g, g]
    for _ in range(int(rng.integers(0, 8))):                    # error reads
        a = int(rng.integers(0, len(g)))
        r = list(g[a:a + 40])
        r[int(rng.integers(0, len(r)))] = ur.BASES[int(rng.integers(0, 4))]
        seqs.append("".join(r))
    for _ in range(int(rng.integers(0, 3))):                    # circles
        c = _rand(rng, int(rng.choice([k + 1, 2 * k, 50])))
        seqs += [c + c[:k - 1]] * 2
    if rng.random() < 0.4:                                      # a hairpin
        h = _rand(rng, k + 3)
        seqs += [h + ur.rc(h)] * 2
    if k % 2 == 0 and rng.random() < 0.5:                       # a palindrome
        h = _rand(rng, k // 2)
        seqs += [_rand(rng, 8) + h + ur.rc(h) + _rand(rng, 8)] * 2
    return seqs


@pytest.mark.parametrize("canonical", [False, True])
def test_reference_invariants(canonical):
    rng = np.random.default_rng(77 + canonical)
    cycles = 0
    for _ in range(120):
        k = int(rng.integers(2, 13))
        min_count = int(rng.integers(1, 3))
        table = ur.count_kmers(_random_input(rng, k), k, canonical)
        units = ur.unitigs(table, k, canonical, min_count)
        solid = {x: c for x, c in table.items() if c >= min_count}
        seen = {}
        firsts = []
        for seq, kc, n, circ in units:
            assert len(seq) == n + k - 1
            firsts.append(seq[:k])
            total = 0
            for i in range(n):
                w = seq[i:i + k]
                node = min(w, ur.rc(w)) if canonical else w
                assert node in solid and node not in seen
                seen[node] = True
                total += solid[node]
            assert total == kc
            if circ:                                            # the cut closes: the last k-mer is followed by the first
                cycles += 1
                assert n >= 2 and seq[n:n + k - 1] + seq[k - 1] == seq[:k]
        assert set(seen) == set(solid)                          # every solid key, exactly once
        assert firsts == sorted(firsts) and len(set(firsts)) == len(firsts)
        assert [u[0] for u in units] == sorted(u[0] for u in units)
    assert cycles > 0


def test_reference_neighbor_mask():
    table = ur.count_kmers(["AACGT", "AACGG"], 3, False)
    # ACG: successors CGG (bit 2) and CGT (bit 3), predecessor AAC (bit 4 + 0)
    assert ur.neighbor_mask(table, "ACG", 3, False) == (1 << 2) | (1 << 3) | (16 << 0)
    assert ur.neighbor_mask(table, "ACG", 3, False, 2) == 16      # CGG and CGT were counted once
    assert ur.neighbor_mask(table, "TTT", 3, False) == 0
    # canonical: the neighbour is canonicalised, the key is taken as given: CGT is stored as ACG
    table = ur.count_kmers(["AACG"], 3, True)
    assert ur.neighbor_mask(table, "CGT", 3, True) == (1 << 3) | (16 << 0)    # CGT -> GTT = rc(AAC); ACG -> CGT
    assert ur.key_of("ACGT") == (0b00011011, 0) and ur.str_of(0b00011011, 0, 4) == "ACGT"
    assert ur.key_of("T" * 33) == (0xFFFFFFFFFFFFFFFF, 3)


# ------------------------------------------------------------------ the reference: hand-worked cases

@pytest.mark.parametrize("seqs, k, canonical, min_count, want", [
    # a Y: AAC -> ACG -> {CGG, CGT}; the branch node ends the unitig, its two successors stand alone
    (["AACGT", "AACGG"], 3, False, 1, [("AACG", 4, 2, False), ("CGG", 1, 1, False), ("CGT", 1, 1, False)]),
    # a tip: CAGG branches into AGGT (the path, counted twice) and AGGA (the tip, once); without the tip one chain
    (["CAGGTCAT", "CAGGTCAT", "AGGA"], 4, False, 1, [("AGGA", 1, 1, False), ("AGGTCAT", 8, 4, False), ("CAGG", 2, 1, False)]),
    (["CAGGTCAT", "CAGGTCAT", "AGGA"], 4, False, 2, [("CAGGTCAT", 10, 5, False)]),
    # a bubble: TCAG opens it, TCAT closes it, the two arms between them
    (["TCAGGTCATC", "TCAGCTCATC"], 4, False, 1,
     [("CAGCTCA", 4, 4, False), ("CAGGTCA", 4, 4, False), ("TCAG", 2, 1, False), ("TCATC", 4, 2, False)]),
    # ACACACAC: ACA <-> CAC, a cycle of two, cut at ACA; in a canonical job its mirror GTG <-> TGT is not written
    (["ACACACAC"], 3, False, 1, [("ACAC", 6, 2, True)]),
    (["ACACACAC"], 3, True, 1, [("ACAC", 6, 2, True)]),
    (["ACACACAC"], 4, False, 1, [("ACACA", 5, 2, True)]),
    # a homopolymer: AAA follows itself, so it has two successors and two predecessors: single nodes
    (["CAAAAAG"], 3, False, 1, [("AAA", 3, 1, False), ("AAG", 1, 1, False), ("CAA", 1, 1, False)]),
    (["CAAAAAG"], 3, True, 1, [("AAA", 3, 1, False), ("AAG", 1, 1, False), ("CAA", 1, 1, False)]),
    # a hairpin at odd k: CAG -> AGC -> GCT = rc(AGC): the link into the own node is none; the mirror half is not written
    (["CAGCTG"], 3, True, 1, [("CAGC", 4, 2, False)]),
    # h + rc(h) at k = 5: AACGT is followed by ACGTC and by its own complement ACGTT: a branch; the chain ends at the
    # hairpin GTCGA -> TCGAC = rc(GTCGA)
    (["AACGTCGACGTT"], 5, True, 1, [("AACGT", 2, 1, False), ("ACGTCGA", 6, 3, False)]),
    # a palindrome at even k: ACGT is its own complement: no link touches it, it is written once
    (["CAACGTTG"], 4, True, 1, [("ACGT", 1, 1, False), ("CAACG", 4, 2, False)]),
    # a circle of five in a job on one strand: cut at its smallest k-mer ACG
    (["ACGGTACG"], 3, False, 1, [("ACGGTAC", 6, 5, True)]),
])
def test_reference_hand_worked(seqs, k, canonical, min_count, want):
    assert ur.unitigs(ur.count_kmers(seqs, k, canonical), k, canonical, min_count) == want


def test_reference_layout_and_text():
    units = [("ACAC", 6, 2, True), ("CGT", 1, 1, False)]
    data, start, length, rec = ur.layout(units)
    assert data.tolist() == [0, 1, 0, 1, -1, 1, 2, 3, -1] and start.tolist() == [0, 5] and length.tolist() == [4, 3]
    assert rec.tolist() == [(6, 2, 1), (1, 1, 0)]
    assert ur.fasta_text(units) == b">0 LN:i:4 KC:i:6 km:f:3.0 CL:i:1\nACAC\n>1 LN:i:3 KC:i:1 km:f:1.0\nCGT\n"


# ------------------------------------------------------------------ the host formatter

def _format(L, data, start, length, rec):
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if len(a) else None
    n = L.cfrk_host_format_unitigs(vp(data), vp(start), vp(length), vp(rec), len(start), None, 0)
    buf = C.create_string_buffer(n + 1)
    assert L.cfrk_host_format_unitigs(vp(data), vp(start), vp(length), vp(rec), len(start), buf, n) == n
    assert buf.raw[n:] == b"\0"                                  # nothing behind the size it asked for
    return buf.raw[:n]


def test_unitig_formatter(host):
    # the mean to one decimal with halves up: 7 / 2 = 3.5, 1 / 3 = 0.3, 2 / 3 = 0.7, 19 / 20 = 0.95 -> 1.0, a sum above 2^63
    units = [("ACGTA", 7, 2, False), ("CCC", 1, 3, True), ("GGGTT", 2, 3, False), ("T" * 23, 19, 20, True),
             ("TTA", (1 << 64) - 1, 1, False)]
    want = (b">0 LN:i:5 KC:i:7 km:f:3.5\nACGTA\n>1 LN:i:3 KC:i:1 km:f:0.3 CL:i:1\nCCC\n>2 LN:i:5 KC:i:2 km:f:0.7\nGGGTT\n"
            b">3 LN:i:23 KC:i:19 km:f:1.0 CL:i:1\n" + b"T" * 23 + b"\n>4 LN:i:3 KC:i:18446744073709551615 km:f:18446744073709551615.0\nTTA\n")
    assert ur.fasta_text(units) == want
    assert _format(host, *ur.layout(units)) == want
    assert _format(host, *ur.layout([])) == b""
    data, start, length, rec = ur.layout([("ACGT", 4, 1, False)])
    data[1] = 9                                                 # any other code reads N
    assert _format(host, data, start, length, rec) == b">0 LN:i:4 KC:i:4 km:f:4.0\nANGT\n"
    rng = np.random.default_rng(3)
    units = [(_rand(rng, int(n) + 4), int(kc), int(n), bool(c)) for n, kc, c in
             zip(rng.integers(1, 300, 200), rng.integers(1, 1 << 40, 200), rng.integers(0, 2, 200))]
    assert _format(host, *ur.layout(units)) == ur.fasta_text(units)


# ------------------------------------------------------------------ the CLI's refusals, the kernels' resources

@pytest.mark.parametrize("args, msg", [
    (["--unitigs-out", "u.fa"], b"--unitigs-out needs --global"),
    (["--global", "--unitigs-out", "u.fa", "--gpus", "2"], b"--unitigs-out needs --global on one device"),
    (["--global", "--unitigs-min-count", "2"], b"--unitigs-min-count needs --unitigs-out UFILE"),
    (["--global", "--unitigs-out", "u.fa", "--unitigs-min-count", "two"], b"--unitigs-min-count needs a count"),
    (["--global", "--unitigs-out"], b"--unitigs-out needs a value"),
])
def test_cli_refuses_bad_unitig_options_before_reading_input(cli, tmp_path, args, msg):
    out = tmp_path / "o.txt"
    p = subprocess.run([cli, str(tmp_path / "missing.fasta"), str(out), "15"] + args, cwd=tmp_path, capture_output=True, timeout=60)
    assert p.returncode == 1
    assert msg in p.stderr
    assert not out.exists() and not (tmp_path / "u.fa").exists()


def test_unitig_kernels_use_no_scratch(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path / "unitigs.s"
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(CSRC, "unitigs.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = []
    for name, ops, size in _functions(out.read_text()):
        if not re.search(r"\du_[a-z_]+_kernel", name):         # (the library sort and scan are not this project's kernels)
            continue
        names.append(name)
        assert ops == 0, f"{name} has {ops} scratch instructions"
        assert not size, f"{name} reserves {size} bytes of scratch per thread"
    # three index modes x both strand rules for each kernel that looks keys up
    for kern in ("u_neighbors_kernel", "u_adj_kernel", "u_link_kernel", "u_walk_kernel", "u_stitch_kernel", "u_ring_kernel",
                 "u_free_ring_kernel", "u_emit_kernel"):
        assert sum(kern in n for n in names) == 6, kern
    assert sum("u_heads_kernel" in n for n in names) == 2
