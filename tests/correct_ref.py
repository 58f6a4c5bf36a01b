"""Spectral error correction (cfrk_global_correct_reads) in plain Python -- TEST INFRASTRUCTURE ONLY.

The rule of include/cfrk_abi.h, word for word.  The counts are a dict {key: count} with the key a Python int of 2k bits,
first base most significant (canonical: the smaller of the k-mer and its reverse complement), as tests/normalize_ref.py
builds it.  Every window of a read gets a class (invalid, weak, solid); the weak runs are walked from left to right; a
run is attempted by the table of the rule and every alternative base is tried by looking up the run's windows of the
ORIGINAL read with that one base replaced.  Nothing here knows how the device does it."""
import numpy as np

from . import normalize_ref as nr

FIX_DTYPE = np.dtype([("fixed", "<u4"), ("left", "<u4")])
INVALID, WEAK, SOLID = 0, 1, 2


def window_key(codes, w, k, canonical):
    """key of window w of codes (a list of ints), None when one of its k codes is not 0..3"""
    fwd = rc = 0
    for j in range(k):
        c = codes[w + j]
        if c < 0 or c > 3:
            return None
        fwd = (fwd << 2) | c
        rc |= (3 - c) << (2 * j)
    return min(fwd, rc) if canonical else fwd


def window_classes(codes, k, canonical, counts, min_count):
    """the class of every window of the read, by rolling the key"""
    L = len(codes)
    mask = (1 << (2 * k)) - 1
    fwd = rc = run = 0
    out = []
    for p, c in enumerate(codes):
        if c < 0 or c > 3:
            run = 0
        else:
            fwd = ((fwd << 2) | c) & mask
            rc = (rc >> 2) | ((3 - c) << (2 * (k - 1)))
            run += 1
        if p >= k - 1:
            if run < k:
                out.append(INVALID)
            else:
                out.append(SOLID if counts.get(min(fwd, rc) if canonical else fwd, 0) >= min_count else WEAK)
    assert len(out) == max(L - k + 1, 0)
    return out


def weak_runs(cls):
    """[(a, b)]: the maximal stretches of weak windows"""
    runs, w, W = [], 0, len(cls)
    while w < W:
        if cls[w] != WEAK:
            w += 1
            continue
        a = w
        while w < W and cls[w] == WEAK:
            w += 1
        runs.append((a, w - 1))
    return runs


def attempted_position(cls, a, b, k):
    """the position p of the run [a, b] when it is attempted, None otherwise: the table of the rule"""
    W, n = len(cls), b - a + 1
    left = None if a == 0 else cls[a - 1]
    right = None if b == W - 1 else cls[b + 1]
    if left == SOLID and right == SOLID and n == k:
        return b
    if left is None and right == SOLID and n <= k:
        return b
    if left == SOLID and right is None and n <= k:
        return a + k - 1
    return None


def correct_codes(codes, k, canonical, counts, min_count):
    """one read (a list of ints) -> (corrected list, fixed, left)"""
    out = list(codes)
    if len(codes) < k:
        return out, 0, 0
    cls = window_classes(codes, k, canonical, counts, min_count)
    fixed = left = 0
    for a, b in weak_runs(cls):
        p = attempted_position(cls, a, b, k)
        passing = []
        if p is not None:
            assert all(w <= p < w + k for w in (a, b))
            for x in range(4):
                if x == codes[p]:
                    continue
                trial = list(codes)                      # the ORIGINAL read with one base replaced
                trial[p] = x
                if all(counts.get(window_key(trial, w, k, canonical), 0) >= min_count for w in range(a, b + 1)):
                    passing.append(x)
        if len(passing) == 1:
            out[p] = passing[0]
            fixed += 1
        else:
            left += 1
    return out, fixed, left


def correct(data, start, length, k, canonical, counts, min_count):
    """the call on struct-read buffers -> (data_out, fix); a read whose range does not lie inside the buffer gets {0, 0}
    and its bytes are only copied (the device form's rule for unchecked start / length)"""
    data = np.asarray(data, np.int8)
    out = data.copy()
    fix = np.zeros(len(start), FIX_DTYPE)
    for i, (st, ln) in enumerate(zip(start, length)):
        st, ln = int(st), int(ln)
        if st < 0 or ln < k or st + ln > len(data):
            continue
        codes, f, l = correct_codes(data[st:st + ln].tolist(), k, canonical, counts, min_count)
        out[st:st + ln] = codes
        fix[i] = (f, l)
    return out, fix


def flatten(reads, term=-1):
    """reads (int8 arrays) -> (data, start, length) in the struct-read layout, one terminator byte behind every read"""
    length = np.array([len(r) for r in reads], np.int32)
    start = (np.concatenate([[0], np.cumsum(length.astype(np.int64) + 1)])[:-1]).astype(np.int64)
    data = np.full(int(length.sum()) + len(reads), term, np.int8)
    for s, r in zip(start, reads):
        data[s:s + len(r)] = r
    return data, start, length


def count_reads(data, start, length, k, canonical, counts=None):
    """the job's counts after a plain add of the reads"""
    return nr.add_keys(nr.all_read_keys(data, start, length, k, canonical), counts)


def revcomp(a):
    return (3 - a[::-1]).astype(np.int8)


def substitute(read, p, rng):
    """read with another base at p"""
    r = read.copy()
    r[p] = (int(r[p]) + 1 + int(rng.integers(0, 3))) & 3
    return r
