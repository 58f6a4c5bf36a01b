"""Paired-end reads without a GPU: the plain-Python reference (tests/pair_ref.py) against hand-written expectations,
the resources of the kernels of pairs.hip, and the command line's refusals, which come before a device is opened."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import pair_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC = np.dtype([("head_off", "<i8"), ("qual_off", "<i8"), ("head_len", "<i4"), ("qual_len", "<i4")])


def _reads(seqs):
    """struct-read buffers of strings over ACGTN"""
    code = {"A": 0, "C": 1, "G": 2, "T": 3, "N": -1}
    data, start, length = [], [], []
    for s in seqs:
        start.append(len(data))
        length.append(len(s))
        data += [code[c] for c in s] + [-1]
    return np.array(data, np.int8), np.array(start, np.int64), np.array(length, np.int32)


def _headers(lines):
    """a text made of header lines only, with its records"""
    text, rec = b"", np.zeros(len(lines), REC)
    for i, ln in enumerate(lines):
        rec[i] = (len(text), -1, len(ln), 0)
        text += ln + b"\n"
    return text, rec


def test_either_keeps_a_mate_without_a_valid_window_and_it_inserts_nothing():
    """pair 0: a fresh read and a mate of Ns only; pair 1: the same fresh read again (now at the cutoff) with a mate
    too short for a window"""
    a = "ACGTTGCA"
    d, s, l = _reads([a, "NNNNNNNN", a, "AC"])
    keep, n, counts = pr.normalize_pairs(d, s, l, 5, False, 1, 2, pr.EITHER)
    assert keep.tolist() == [1, 1, 0, 0] and n == 2
    # only the four windows of the first read were inserted, once each
    assert sorted(counts.values()) == [1, 1, 1, 1]
    keep, n, counts = pr.normalize_pairs(d, s, l, 5, False, 1, 2, pr.BOTH)
    assert keep.tolist() == [0, 0, 0, 0] and n == 0 and counts == {}
    # one round of both pairs: the second copy is judged before the first is inserted
    keep, n, counts = pr.normalize_pairs(d, s, l, 5, False, 1, 4, pr.EITHER)
    assert keep.tolist() == [1, 1, 1, 1] and n == 4 and sorted(counts.values()) == [2, 2, 2, 2]


def test_both_yields_the_right_orphan_on_each_side():
    keep_a, keep_b = [1, 1, 0, 0, 255], [1, 0, 1, 0, 7]
    sa = pr.survive_all(5, keep=keep_a)
    sb = pr.survive_all(5, keep=keep_b)
    pair, oa, ob, counts = pr.join(sa, sb, pr.BOTH)
    assert pair.tolist() == [1, 0, 0, 0, 1] and oa.tolist() == [0, 1, 0, 0, 0] and ob.tolist() == [0, 0, 1, 0, 0]
    assert counts == (2, 1, 1, 1)
    pair, oa, ob, counts = pr.join(sa, sb, pr.EITHER)
    assert pair.tolist() == [1, 1, 1, 0, 1] and not oa.any() and not ob.any() and counts == (4, 0, 0, 1)


def test_survive_rule():
    assert pr.survives(None, None, None, 0)
    assert pr.survives(1, (2, 5), 7, 5) and not pr.survives(1, (2, 5), 7, 6)
    assert not pr.survives(1, (3, 5), 7, 0) and not pr.survives(1, (-1, 3), 7, 0) and not pr.survives(1, (0, -1), 7, 0)
    assert not pr.survives(0, (0, 7), 7, 0)
    assert pr.survives(None, None, 7, 7) and not pr.survives(None, None, 6, 7)


def test_mate_names():
    lines = [b"@r1/1", b"@r1/2",                                  # /1 with /2
             b"@M01:8:000-AB:1:1101:15:13 1:N:0:ACGT", b"@M01:8:000-AB:1:1101:15:13 2:N:0:ACGT",   # Casava 1.8
             b"@", b"@",                                          # empty names
             b"@read_17x", b"@read_17y",                          # a mismatch in the last byte
             b"@r5/2", b"@r5/1",                                  # the wrong order
             b"@same\tcomment a", b"@same other",                 # tab and space end the identifier
             b"@/1", b"@/2"]                                      # nothing left once the suffixes are dropped
    text, rec = _headers(lines)
    good = [pr.pair_good(text, rec[2 * j], text, rec[2 * j + 1]) for j in range(len(lines) // 2)]
    assert good == [True, True, False, False, False, True, False]
    assert pr.check_pairs(text, rec[0::2], text, rec[1::2]) == (2, 4)
    assert pr.check_pairs(text, rec[0:4:2], text, rec[1:4:2]) == (-1, 0)
    assert pr.identifier(text, rec[2]) == b"M01:8:000-AB:1:1101:15:13"
    outside = rec[:1].copy()
    outside["head_len"] = len(text) + 1
    assert pr.identifier(text, outside[0]) is None and not pr.pair_good(text, outside[0], text, rec[1])


@pytest.fixture(scope="module")
def built():
    import cfrk_amd
    if not os.path.exists(cfrk_amd.library_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return cfrk_amd


def test_new_symbols_constants_and_dtype(built):
    syms = built.abi_symbols()
    L = ctypes.CDLL(built.library_path())
    for s in ("cfrk_reads_pair_keep", "cfrk_reads_pair_keep_device", "cfrk_text_pair_check", "cfrk_text_pair_check_device",
              "cfrk_global_normalize_pairs", "cfrk_global_normalize_pairs_device"):
        assert s in syms, f"{s} is not declared in include/cfrk_abi.h"
        assert hasattr(L, s), f"{s} is not exported"
    header = open(os.path.join(ROOT, "include", "cfrk_abi.h")).read()
    for name in ("CFRK_PAIR_BOTH", "CFRK_PAIR_EITHER", "CFRK_PAIR_NAME_FAST"):
        m = re.search(r"^#define\s+" + name + r"\s+(\d+)", header, re.M)
        assert m and int(m.group(1)) == getattr(built, name)
    assert (built.CFRK_PAIR_BOTH, built.CFRK_PAIR_EITHER) == (pr.BOTH, pr.EITHER)
    assert built.PAIR_COUNTS_DTYPE.itemsize == 32 and built.PAIR_COUNTS_DTYPE.names == ("pairs", "orphans_a", "orphans_b", "dropped")
    for f in ("pair_keep", "pair_keep_device", "check_pairs", "check_pairs_device"):
        assert callable(getattr(built.Context, f))
    assert callable(built.GlobalCounter.normalize_pairs) and callable(built.GlobalCounter.normalize_pairs_device)


def test_pairs_kernels_use_no_scratch_and_are_built_by_the_makefile(tmp_path):
    from .test_kernel_resources import CSRC, HIPCC, _functions
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "pairs.hip" in re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path / "pairs.s"
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(CSRC, "pairs.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = []
    for name, ops, size in _functions(out.read_text()):
        names.append(name)
        assert ops == 0, f"{name} has {ops} scratch instructions"
        assert not size, f"{name} reserves {size} bytes of scratch per thread"
    for kern in ("pair_join_kernel", "pair_names_kernel", "pair_names_long_kernel"):
        assert sum(kern in n for n in names) == 1, (kern, names)


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(os.path.join(ROOT, "cfrk_amd", "cfrk")):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host"), "-j4"], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "cfrk_amd", "cfrk")


def _fasta(path, n):
    path.write_text("".join(f">r{i // 2}/{i % 2 + 1}\nACGTACGTTGCAACGTAGCTAGCTAGGATC\n" for i in range(n)))
    return str(path)


def test_cli_refusals_come_before_a_device_is_opened(cli, tmp_path):
    """every one ends with exit status 1 and its own message; none opens the (missing) input or a device"""
    odd, even, even2 = _fasta(tmp_path / "odd.fa", 5), _fasta(tmp_path / "even.fa", 6), _fasta(tmp_path / "even2.fa", 4)
    head = [cli, str(tmp_path / "missing.fasta"), str(tmp_path / "out.cfrk"), "15", "--global"]
    f, f2, nf = str(tmp_path / "f.fa"), str(tmp_path / "f2.fa"), str(tmp_path / "n.fa")
    cases = [
        (["--query", odd, "--filter-out", f, "--paired"], ["odd.fa", "5 records", "odd"]),
        (["--query", even, "--query2", even, "--filter-out", f], ["--query2 needs --filter-out2"]),
        (["--query", even, "--filter-out", f, "--paired", "--gpus", "2"], ["--paired", "--gpus above 1"]),
        (["--normalize-out", nf, "--normalize-cutoff", "5", "--query", even, "--query2", even], ["--normalize-out takes ONE input file"]),
        (["--paired", "--batch", "2"], ["--paired", "--batch"]),
        (["--paired"], ["--paired needs --filter-out"]),
        (["--query", even, "--query2", even, "--query-out", str(tmp_path / "q.txt")], ["--query2 needs --filter-out FFILE or --correct-out"]),
        (["--query", even, "--query2", even2, "--filter-out", f, "--filter-out2", f2], ["even.fa holds 6 records", "even2.fa holds 4"]),
        (["--query", even, "--query2", even, "--correct-out", f, "--correct-min-count", "2"], ["--query2 needs --correct-out2"]),
        (["--query", even, "--filter-out", f, "--paired", "--query2", even, "--filter-out2", f2], ["one of them"]),
        (["--query", even, "--filter-out", f, "--filter-orphans", f2], ["--filter-orphans needs --paired or --query2"]),
        (["--normalize-out", nf, "--normalize-cutoff", "5", "--paired", "--normalize-batch", "7"], ["--normalize-batch 7", "even"]),
        (["--query", even, "--filter-out", f, "--pair-check", "off"], ["--pair-check needs --paired or --query2"]),
        (["--query", even, "--filter-out", f, "--paired", "--pair-check", "maybe"], ["--pair-check takes on or off"]),
    ]
    for args, words in cases:
        p = subprocess.run(head + args, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1, (args, p.returncode, p.stderr)
        for w in words:
            assert w in p.stderr, (args, w, p.stderr)
        assert "missing.fasta" not in p.stderr, (args, p.stderr)
        for out in (f, f2, nf, str(tmp_path / "out.cfrk")):
            assert not os.path.exists(out), (args, out)
