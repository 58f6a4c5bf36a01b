"""CPU-side checks of the unitig links: the C ABI declares and exports the two calls, cfrk_unitig_link is 8 bytes with the
documented offsets, the Python mirror exists; the plain-Python reference of tests/unitig_links_ref.py keeps its
invariants on random tables and gives the hand-worked answers; the two link formatters of libcfrk_host.so; the CLI's
refusals; the kernels of unitig_links.hip use no scratch memory."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from . import unitig_links_ref as lr
from . import unitig_ref as ur
from .test_kernel_resources import CSRC, HIPCC, ROOT, _functions
from .test_unitigs_cpu import _rand, _random_input

LINK_CALLS = ("cfrk_global_unitig_links", "cfrk_global_unitig_links_device")
F, T = lr.FROM_MINUS, lr.TO_MINUS


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
    L.cfrk_host_format_unitigs_links.argtypes = [vp, vp, vp, vp, C.c_int64, vp, vp, C.c_char_p, C.c_size_t]
    L.cfrk_host_format_unitigs_links.restype = C.c_size_t
    L.cfrk_host_format_gfa.argtypes = [vp, vp, vp, vp, C.c_int64, vp, vp, C.c_int, C.c_char_p, C.c_size_t]
    L.cfrk_host_format_gfa.restype = C.c_size_t
    return L


@pytest.fixture(scope="module")
def cli(built):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "cfrk_amd", "cfrk")


def test_abi_declares_and_exports_the_link_calls(built):
    syms = built.abi_symbols()
    L = C.CDLL(built.library_path())
    for s in LINK_CALLS:
        assert s in syms
        assert hasattr(L, s)
    header = open(os.path.join(ROOT, "include", "cfrk_abi.h")).read()
    for name, value in (("CFRK_LINK_FROM_MINUS", 1), ("CFRK_LINK_TO_MINUS", 2)):
        m = re.search(r"#define %s\s+(0x[0-9a-fA-F]+|\d+)\b" % name, header)
        assert m and int(m.group(1), 0) == getattr(built, name) == value, name
    assert re.search(r"typedef struct cfrk_unitig_link \{[^}]*uint32_t to;[^}]*uint32_t flags;[^}]*\} cfrk_unitig_link;", header, re.S)
    dt = built.UNITIG_LINK_DTYPE
    assert dt.itemsize == 8 and [dt.fields[n][1] for n in ("to", "flags")] == [0, 4]
    assert dt == lr.UNITIG_LINK_DTYPE
    for name in ("unitig_links", "unitig_links_device"):
        assert callable(getattr(built.GlobalCounter, name))


def test_sizeof_link_in_c(tmp_path):
    """the struct as a C compiler lays it out: 8 bytes, to at 0, flags at 4"""
    src = tmp_path / "s.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "cfrk_abi.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(cfrk_unitig_link), offsetof(cfrk_unitig_link, to), '
                   'offsetof(cfrk_unitig_link, flags)); return 0; }\n')
    exe = tmp_path / "s"
    subprocess.check_call(["cc", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)]).split() == [b"8", b"0", b"4"]


# ------------------------------------------------------------------ the reference: invariants

@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [3, 4, 5, 8])
def test_reference_invariants(k, canonical):
    """(the reference itself asserts the head fact, the palindrome fact, no duplicates, the mirror and the bound)"""
    rng = np.random.default_rng(100 * k + canonical)
    circles = selfs = total = 0
    for it in range(50):
        min_count = int(rng.integers(1, 3))
        if it < 40:
            seqs = _random_input(rng, k)
        else:                                                   # a lone circle (small k: the random tables are too full for one)
            c = _rand(rng, int(rng.choice([k + 1, k + 2, 2 * k + 1])))
            seqs = [c + c[:k - 1]] * 2
        table = ur.count_kmers(seqs, k, canonical)
        units = ur.unitigs(table, k, canonical, min_count)
        link_ptr, links = lr.links(units, table, k, canonical, min_count)
        nS = len(units)
        assert link_ptr[0] == 0 and len(link_ptr) == nS + 1 and link_ptr[nS] == len(links) and (np.diff(link_ptr) >= 0).all()
        assert len(links) <= (16 if canonical else 4) * nS
        total += len(links)
        flat = {(j, int(f) & F, int(to), int(f) & T) for j in range(nS) for to, f in links[link_ptr[j]:link_ptr[j + 1]].tolist()}
        assert len(flat) == len(links)
        if canonical:
            for j, f, to, t in flat:                            # the mirror: (v, not ov) -> (u, not ou)
                assert (to, 0 if t else F, j, 0 if f else T) in flat
        else:
            assert all(f == 0 and t == 0 for _, f, _, t in flat)
        for j, (seq, kc, n, circ) in enumerate(units):
            self_link = (j, 0, j, 0) in flat
            if circ:                                            # that is how GFA states a circle
                circles += 1
                assert self_link and (not canonical or (j, F, j, T) in flat)
            elif self_link:
                # the last k-mer is followed by the first without a unitig LINK between them: a homopolymer node, or a
                # branch at the junction (the definition of the unitigs, cfrk_abi.h)
                selfs += 1
                out = ur.neighbor_mask(table, seq[-k:], k, canonical, min_count) & 15
                into = ur.neighbor_mask(table, seq[:k], k, canonical, min_count) >> 4
                assert n == 1 or bin(out).count("1") > 1 or bin(into).count("1") > 1
    assert total > 0 and circles > 0


# ------------------------------------------------------------------ the reference: hand-worked cases

@pytest.mark.parametrize("seqs, k, canonical, units, link_ptr, links", [
    # the Y: AAC -> ACG -> {CGG, CGT}: the unitig AACG is followed by both single nodes, in base order
    (["AACGT", "AACGG"], 3, False, ["AACG", "CGG", "CGT"], [0, 2, 2, 2], [(1, 0), (2, 0)]),
    # a homopolymer: AAA follows itself and is followed by AAG; CAA is followed by both
    (["CAAAAAG"], 3, False, ["AAA", "AAG", "CAA"], [0, 2, 2, 4], [(0, 0), (1, 0), (0, 0), (1, 0)]),
    # the same on both strands: (0,-) = TTT is followed by TTG = (2,-) and by itself; (1,-) = CTT by the same two
    (["CAAAAAG"], 3, True, ["AAA", "AAG", "CAA"], [0, 4, 6, 8],
     [(0, 0), (1, 0), (2, F | T), (0, F | T), (2, F | T), (0, F | T), (0, 0), (1, 0)]),
    # a hairpin: CAGC ends in AGC, followed by GCT = rc(AGC) = head(0,-): its own mirror image, written once
    (["CAGCTG"], 3, True, ["CAGC"], [0, 1], [(0, T)]),
    # an even-k palindrome reached from a neighbour: AACG is followed by ACGT = head(0,+) = head(0,-): two targets;
    # ACGT itself is followed by CGTT = head(1,-), from either of its orientations
    (["CAACGTTG"], 4, True, ["ACGT", "CAACG"], [0, 2, 4], [(1, T), (1, F | T), (0, 0), (0, T)]),
    # a circle on one strand, and one on both: the self links + -> + and - -> -
    (["ACGGTACG"], 3, False, ["ACGGTAC"], [0, 1], [(0, 0)]),
    (["ACACACAC"], 3, True, ["ACAC"], [0, 2], [(0, 0), (0, F | T)]),
])
def test_reference_hand_worked(seqs, k, canonical, units, link_ptr, links):
    table = ur.count_kmers(seqs, k, canonical)
    u = ur.unitigs(table, k, canonical, 1)
    assert [x[0] for x in u] == units
    got_ptr, got = lr.links(u, table, k, canonical, 1)
    assert got_ptr.tolist() == link_ptr and got.tolist() == links


def test_reference_anchors():
    """two totals of the GPU grid's input, from the prototype of the reference"""
    from .test_gpu_unitigs import _input, _table
    for k, n_units, n_links, degree in ((31, 107, 248, None), (4, 136, 1156, 5)):
        table = _table(_input(k), k, True)
        u = ur.unitigs(table, k, True, 1)
        rows = lr.oriented_links(u, table, k, True, 1)
        assert (len(u), sum(len(r) for r in rows)) == (n_units, n_links)
        if degree:                                              # palindromic targets: more than 4 links out of one end
            assert max(sum(1 for x in r if x[0] == o) for r in rows for o in (0, 1)) == degree


def test_reference_texts():
    table = ur.count_kmers(["ACACACAC", "ACACACAC"], 3, True)
    u = ur.unitigs(table, 3, True, 1)
    link_ptr, links = lr.links(u, table, 3, True, 1)
    fa, gfa = lr.fasta_text_links(u, link_ptr, links), lr.gfa_text(u, 3, link_ptr, links)
    assert fa.startswith(b">0 LN:i:4 KC:i:12 km:f:6.0 CL:i:1 L:+:0:+ L:-:0:-\nACAC\n")
    assert gfa.startswith(b"H\tVN:Z:1.0\nS\t0\tACAC\tLN:i:4\tKC:i:12\tkm:f:6.0\n")
    assert b"L\t0\t+\t0\t+\t2M\nL\t0\t-\t0\t-\t2M\n" in gfa
    assert gfa.count(b"\nL\t") == len(links) and gfa.count(b"\nS\t") == len(u)


# ------------------------------------------------------------------ the host formatters

def _texts(L, units, k, link_ptr, links):
    data, start, length, rec = ur.layout(units)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if len(a) else None
    head = (vp(data), vp(start), vp(length), vp(rec), len(start), vp(link_ptr), vp(links))
    out = []
    for fn, args in ((L.cfrk_host_format_unitigs_links, head), (L.cfrk_host_format_gfa, head + (k,))):
        n = fn(*args, None, 0)
        buf = C.create_string_buffer(n + 1)
        assert fn(*args, buf, n) == n
        assert buf.raw[n:] == b"\0"                              # nothing behind the size it asked for
        out.append(buf.raw[:n])
    return out


def test_link_formatters(host):
    rng = np.random.default_rng(5)
    cases = [(["ACACACAC", "ACACACAC", "CAGCTG"], 3, True), (["CAACGTTG", "AACGT", "AACGG"], 4, True), (["ACGT"], 1, False),
             (["ACGT"], 1, True), ([_rand(rng, 300), _rand(rng, 200) + "A" * 20], 8, True), ([_rand(rng, 500)], 5, False)]
    for seqs, k, canonical in cases:
        table = ur.count_kmers(seqs, k, canonical)
        u = ur.unitigs(table, k, canonical, 1)
        link_ptr, links = lr.links(u, table, k, canonical, 1)
        fa, gfa = _texts(host, u, k, link_ptr, links)
        assert fa == lr.fasta_text_links(u, link_ptr, links)
        assert gfa == lr.gfa_text(u, k, link_ptr, links)
        if k == 1:
            assert len(links) > 0 and gfa.count(b"\t0M\n") == len(links)
    # a circular unitig: the L tags stand behind CL:i:1
    table = ur.count_kmers(["ACGGTACG"], 3, False)
    u = ur.unitigs(table, 3, False, 1)
    fa, gfa = _texts(host, u, 3, *lr.links(u, table, 3, False, 1))
    assert fa == b">0 LN:i:7 KC:i:6 km:f:1.2 CL:i:1 L:+:0:+\nACGGTAC\n"
    assert gfa == b"H\tVN:Z:1.0\nS\t0\tACGGTAC\tLN:i:7\tKC:i:6\tkm:f:1.2\nL\t0\t+\t0\t+\t2M\n"
    # the empty list
    fa, gfa = _texts(host, [], 31, np.zeros(1, np.int64), np.zeros(0, lr.UNITIG_LINK_DTYPE))
    assert fa == b"" and gfa == b"H\tVN:Z:1.0\n"
    # an invalid code reads N in the S line as well; targets of ten digits
    data, start, length, rec = ur.layout([("ACGT", 4, 1, False)])
    data[2] = -7
    link_ptr, links = np.array([0, 1], np.int64), np.array([(4294967295, 3)], lr.UNITIG_LINK_DTYPE)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    n = host.cfrk_host_format_gfa(vp(data), vp(start), vp(length), vp(rec), 1, vp(link_ptr), vp(links), 4, None, 0)
    buf = C.create_string_buffer(n)
    assert host.cfrk_host_format_gfa(vp(data), vp(start), vp(length), vp(rec), 1, vp(link_ptr), vp(links), 4, buf, n) == n
    assert buf.raw == b"H\tVN:Z:1.0\nS\t0\tACNT\tLN:i:4\tKC:i:4\tkm:f:4.0\nL\t0\t-\t4294967295\t-\t3M\n"


# ------------------------------------------------------------------ the CLI's refusals, the kernels' resources

@pytest.mark.parametrize("args, msg", [
    (["--unitigs-gfa", "g.gfa"], b"--unitigs-gfa needs --global"),
    (["--global", "--unitigs-gfa", "g.gfa", "--gpus", "2"], b"--unitigs-gfa needs --global on one device"),
    (["--global", "--unitigs-links"], b"--unitigs-links needs --unitigs-out UFILE"),
    (["--global", "--unitigs-links", "--unitigs-gfa", "g.gfa"], b"--unitigs-links needs --unitigs-out UFILE"),
    (["--global", "--unitigs-gfa"], b"--unitigs-gfa needs a value"),
    (["--global", "--unitigs-gfa", "g.gfa", "--unitigs-min-count", "two"], b"--unitigs-min-count needs a count"),
])
def test_cli_refuses_bad_link_options_before_reading_input(cli, tmp_path, args, msg):
    out = tmp_path / "o.txt"
    p = subprocess.run([cli, str(tmp_path / "missing.fasta"), str(out), "15"] + args, cwd=tmp_path, capture_output=True, timeout=60)
    assert p.returncode == 1
    assert msg in p.stderr
    assert not out.exists() and not (tmp_path / "g.gfa").exists()


def test_unitig_link_kernels_use_no_scratch(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path / "unitig_links.s"
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(CSRC, "unitig_links.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = []
    for name, ops, size in _functions(out.read_text()):
        if not re.search(r"\dul_[a-z_]+_kernel", name):        # (the library scan is not this project's kernel)
            continue
        names.append(name)
        assert ops == 0, f"{name} has {ops} scratch instructions"
        assert not size, f"{name} reserves {size} bytes of scratch per thread"
    # three index modes x both strand rules for each kernel that looks keys up
    for kern in ("ul_tag_kernel", "ul_count_kernel", "ul_fill_kernel"):
        assert sum(kern in n for n in names) == 6, kern
    assert sum("ul_ptr_kernel" in n for n in names) == 1
