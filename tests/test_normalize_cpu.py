"""CPU: the reference of digital normalisation (tests/normalize_ref.py) held to cases worked by hand, the counting
identity the device judge relies on, and the boundary of the new calls (symbols, mirrored constant, Python methods).
The device is held to this reference by tests/test_gpu_normalize.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from . import normalize_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "N": -1}


def _reads(seqs):
    """struct-read layout of the sequences: every read followed by one terminator"""
    data, start, length = [], [], []
    for s in seqs:
        start.append(len(data))
        length.append(len(s))
        data += [CODE[c] for c in s] + [-1]
    return np.array(data, np.int8), np.array(start, np.int64), np.array(length, np.int32)


def _key(s):
    x = 0
    for c in s:
        x = (x << 2) | CODE[c]
    return x


SEQ = "ACGTTGCAAGGCTA"      # 14 bases: 10 windows at k = 5, all different


def test_identical_reads_streaming_keeps_cutoff_many():
    """the first read sees counts 0, the second 1, ...: read number C + 1 is the first whose median is not below C"""
    d, s, l = _reads([SEQ] * 9)
    for cutoff in (1, 3, 8, 9, 20):
        keep, n, counts = nr.normalize(d, s, l, 5, False, cutoff, 1)
        want = min(cutoff, 9)
        assert n == want and keep.tolist() == [1] * want + [0] * (9 - want)
        assert set(counts.values()) == {want} and len(counts) == 10


def test_identical_reads_one_round_keeps_all():
    """every read of a round is judged before any of them is counted"""
    d, s, l = _reads([SEQ] * 9)
    for batch in (9, 10, 1000):
        keep, n, counts = nr.normalize(d, s, l, 5, False, 3, batch)
        assert n == 9 and keep.all() and set(counts.values()) == {9}
    # rounds of 4: the first round (4 reads) is kept whole, then the counts read 4 >= 3
    keep, n, counts = nr.normalize(d, s, l, 5, False, 3, 4)
    assert keep.tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0] and set(counts.values()) == {4}
    # rounds of 2 at cutoff 3: rounds one and two are kept (the counts read 0, then 2), round three sees 4
    keep, n, _ = nr.normalize(d, s, l, 5, False, 3, 2)
    assert keep.tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0]


def test_cutoff_zero_keeps_none_and_max_keeps_all_with_a_window():
    d, s, l = _reads([SEQ, "ACGT", SEQ[::-1], "ACNNTACGNTT", ""])
    keep, n, counts = nr.normalize(d, s, l, 5, False, 0, 2)
    assert n == 0 and not keep.any() and counts == {}
    keep, n, counts = nr.normalize(d, s, l, 5, False, 0xFFFFFFFF, 2)
    assert keep.tolist() == [1, 0, 1, 0, 0]       # shorter than k, no window without an N, empty: dropped
    assert counts == nr.add_keys(nr.all_read_keys(d, s, l, 5, False))


def test_windows_skip_invalid_codes():
    d, s, l = _reads(["ACGTNACGTA"])
    assert nr.read_keys(d, 0, 10, 4, False) == [_key("ACGT"), _key("ACGT"), _key("CGTA")]
    keep, n, counts = nr.normalize(d, s, l, 4, False, 1, 1)
    assert n == 1 and counts == {_key("ACGT"): 2, _key("CGTA"): 1}
    # a range outside the buffer has no windows (the device form's rule)
    assert nr.read_keys(d, -1, 5, 4, False) == [] and nr.read_keys(d, 8, 4, 4, False) == []


def test_canonical_strands_meet():
    """a read and its reverse complement carry the same canonical k-mers: the second is judged against the first"""
    rc = "".join("TGCA"["ACGT".index(c)] for c in reversed(SEQ))
    d, s, l = _reads([SEQ, rc])
    keep, n, counts = nr.normalize(d, s, l, 5, True, 1, 1)
    assert keep.tolist() == [1, 0] and counts == nr.add_keys([nr.read_keys(d, 0, 14, 5, True)])
    assert sorted(nr.read_keys(d, 0, 14, 5, True)) == sorted(nr.read_keys(d, 15, 14, 5, True))
    assert nr.read_keys(d, 0, 14, 5, True)[0] == min(_key("ACGTT"), _key("AACGT")) == _key("AACGT")
    keep, n, counts = nr.normalize(d, s, l, 5, False, 1, 1)
    assert keep.tolist() == [1, 1] and counts == nr.add_keys(nr.all_read_keys(d, s, l, 5, False))
    # the palindrome ACGT is its own reverse complement: counted once per occurrence, not twice
    d, s, l = _reads(["ACGT"])
    assert nr.normalize(d, s, l, 4, True, 1, 1)[2] == {_key("ACGT"): 1}


def test_median_rule_mixed_counts():
    """10 windows, 5 of them pre-counted to 7: the lower median (element 4 of the sorted counts) is 0, the read is kept;
    with 6 pre-counted it is 7"""
    d, s, l = _reads([SEQ])
    keys = nr.read_keys(d, 0, 14, 5, False)
    for pre, want in ((5, 1), (6, 0)):
        counts = {x: 7 for x in keys[:pre]}
        keep, n, _ = nr.normalize(d, s, l, 5, False, 7, 1, counts)
        assert n == want
    assert nr.lower_median([5, 1, 9, 3]) == 3 and nr.lower_median([4]) == 4 and nr.lower_median([2, 8]) == 2


def test_count_below_cutoff_equals_median_below_cutoff():
    """what the device judges by: #{c < cutoff} > (W - 1) // 2  <=>  lower median < cutoff"""
    rng = np.random.default_rng(5)
    for trial in range(3000):
        W = int(rng.integers(1, 40))
        top = int(rng.choice([2, 5, 30, 0xFFFFFFFF]))
        c = rng.integers(0, top, W, dtype=np.uint64)
        cutoff = int(rng.choice([0, 1, 2, 3, 20, top // 2 + 1, 0xFFFFFFFF]))
        median = int(np.sort(c)[(W - 1) // 2])
        assert (int((c < cutoff).sum()) > (W - 1) // 2) == (median < cutoff), (c, cutoff)
        assert median == nr.lower_median(c.tolist())


def test_digest_and_export_of_the_reference():
    counts = {5: 2, (7 << 64) | 3: 1, 1 << 64: 4}
    lo, hi, cnt = nr.export_arrays(counts)
    assert lo.tolist() == [5, 0, 3] and hi.tolist() == [0, 1, 7] and cnt.tolist() == [2, 4, 1]
    d = nr.digest(counts, True)
    assert d[0] == 3 and d[1] == 7
    assert nr.spectrum(counts, 4).tolist() == [0, 1, 1, 1]


@pytest.fixture(scope="module")
def built():
    import cfrk_amd
    if not os.path.exists(cfrk_amd.library_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    return cfrk_amd


def test_new_symbols_and_constant(built):
    syms = built.abi_symbols()
    L = ctypes.CDLL(built.library_path())
    for s in ("cfrk_global_normalize", "cfrk_global_normalize_device"):
        assert s in syms, f"{s} is not declared in include/cfrk_abi.h"
        assert hasattr(L, s), f"{s} is not exported"
    header = open(os.path.join(ROOT, "include", "cfrk_abi.h")).read()
    m = re.search(r"^#define\s+CFRK_NORMALIZE_BATCH\s+(\d+)", header, re.M)
    assert m and int(m.group(1)) == built.CFRK_NORMALIZE_BATCH
    assert callable(built.GlobalCounter.normalize) and callable(built.GlobalCounter.normalize_device)


def test_normalize_kernels_use_no_scratch(tmp_path):
    from .test_kernel_resources import CSRC, HIPCC, _functions
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path / "normalize.s"
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(CSRC, "normalize.hip"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = []
    for name, ops, size in _functions(out.read_text()):
        names.append(name)
        assert ops == 0, f"{name} has {ops} scratch instructions"
        assert not size, f"{name} reserves {size} bytes of scratch per thread"
    # two key widths x two strand rules for the judge and the insert of each of the three size classes
    for kern in ("normalize_judge_kernelILi16E", "normalize_judge_kernelILi64E", "normalize_judge_long_kernel",
                 "normalize_insert_kernelILi16E", "normalize_insert_kernelILi64E", "normalize_insert_long_kernel"):
        assert sum(kern in n for n in names) == 4, kern
