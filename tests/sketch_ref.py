"""The distinct sketch restated in numpy -- TEST INFRASTRUCTURE ONLY.

The format is the one include/cfrk_abi.h documents: 2^14 one-byte registers, bucket = top 14 bits of the key's hash
(hash_craft.mix: mix(lo) for k <= 32, mix(lo ^ mix(hi)) for k > 32), rank = leading zeros of the remaining 50 bits
+ 1 (51 when they are all zero), register = largest rank seen.  Here: registers from keys, the estimate and the hint
from registers, an enumerator of the valid windows of a code buffer for both key widths, and a generator of read sets
(reads of a random genome, 1 % substitutions, half of them reverse-complemented).
"""
import math

import numpy as np

from . import hash_craft as hc

LOG2M = 14
M = 1 << LOG2M
RANK_MAX = 64 - LOG2M + 1
SIGMA = 1.04 / math.sqrt(M)           # standard error of the estimator
BOUND = 4 * SIGMA                     # what the hint adds and the accuracy tests allow
CANONICAL = 0x2


def clz64(w):
    """leading zeros of every non-zero word"""
    w = np.asarray(w, np.uint64).copy()
    n = np.zeros(len(w), np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        top_clear = (w >> np.uint64(64 - s)) == 0
        n += s * top_clear
        w = np.where(top_clear, w << np.uint64(s), w)
    return n


def registers_from_hashes(h, regs=None):
    h = np.asarray(h, np.uint64)
    regs = np.zeros(M, np.uint8) if regs is None else regs.copy()
    if len(h) == 0:
        return regs
    bucket = (h >> np.uint64(64 - LOG2M)).astype(np.int64)
    w = h << np.uint64(LOG2M)
    rank = np.where(w != 0, clz64(np.where(w != 0, w, np.uint64(1))) + 1, RANK_MAX).astype(np.uint8)
    np.maximum.at(regs, bucket, rank)
    return regs


def registers(lo, hi, k, regs=None):
    """the sketch of the keys (lo, hi) of k bases, already canonical where that is wanted"""
    lo = np.asarray(lo, np.uint64)
    if len(lo) == 0:
        return np.zeros(M, np.uint8) if regs is None else regs.copy()
    hi = np.zeros(len(lo), np.uint64) if hi is None else np.asarray(hi, np.uint64)
    return registers_from_hashes(hc.key_hash(lo, hi, k > 32), regs)


def estimate(regs):
    regs = np.asarray(regs, np.uint8)
    assert regs.shape == (M,)
    hist = np.bincount(regs, minlength=256)
    if hist[0] == M:
        return 0.0
    s = 0.0
    for r in range(255, -1, -1):
        if hist[r]:
            s += math.ldexp(float(hist[r]), -r)
    alpha = 0.7213 / (1.0 + 1.079 / M)
    e = alpha * M * M / s
    if e <= 2.5 * M and hist[0] > 0:
        e = M * math.log(M / float(hist[0]))
    return e


def raw_estimate(regs):
    """the harmonic-mean estimate before the small-range switch (which side of 2.5 m is a sketch on?)"""
    s = float(np.sum(np.ldexp(1.0, -np.asarray(regs, np.int64))))
    return 0.7213 / (1.0 + 1.079 / M) * M * M / s


def hint(regs):
    return int(min(max(math.ceil(estimate(regs) * (1.0 + 4 * 1.04 / math.sqrt(M))), 1 << 20), 1 << 31))


def windows(data, k, canonical=False):
    """every valid window of the code buffer (all k codes 0..3, inside the buffer), in position order
    -> (lo, hi) uint64 arrays; canonical: min(k-mer, reverse complement) as 2k-bit numbers"""
    data = np.asarray(data, np.int8)
    n = len(data) - k + 1
    if n <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint64)
    bad = np.concatenate([[0], np.cumsum((data < 0) | (data > 3))])
    ok = (bad[k:] - bad[:-k]) == 0
    code = np.where((data < 0) | (data > 3), 0, data).astype(np.uint64)
    lo = np.zeros(n, np.uint64)
    hi = np.zeros(n, np.uint64)
    rlo = np.zeros(n, np.uint64)
    rhi = np.zeros(n, np.uint64)
    two, three, s62 = np.uint64(2), np.uint64(3), np.uint64(62)
    for j in range(k):
        c = code[j:j + n]
        if k > 32:
            hi = (hi << two) | (lo >> s62)
        lo = (lo << two) | c
        if canonical:
            if 2 * j < 64:
                rlo |= (three - c) << np.uint64(2 * j)
            else:
                rhi |= (three - c) << np.uint64(2 * j - 64)
    if canonical:
        swap = (rhi < hi) | ((rhi == hi) & (rlo < lo))
        lo, hi = np.where(swap, rlo, lo), np.where(swap, rhi, hi)
    return lo[ok], hi[ok]


def sketch_of_reads(data, k, flags=0, regs=None):
    """-> (registers, valid windows): what cfrk_distinct_sketch must return for the buffer"""
    lo, hi = windows(data, k, bool(flags & CANONICAL))
    return registers(lo, hi, k, regs), len(lo)


def distinct(lo, hi):
    """exact number of distinct keys"""
    if len(lo) == 0:
        return 0
    order = np.lexsort((lo, hi))
    a, b = lo[order], hi[order]
    return 1 + int(np.count_nonzero((a[1:] != a[:-1]) | (b[1:] != b[:-1])))


def layout(reads):
    """struct-read layout of a list of int8 code arrays -> (data, start, length)"""
    length = np.array([len(r) for r in reads], np.int32)
    start = np.concatenate([[0], np.cumsum(length.astype(np.int64) + 1)[:-1]]).astype(np.int64) if len(reads) else np.zeros(0, np.int64)
    data = np.full(int(length.sum()) + len(reads), -1, np.int8)
    for s, r in zip(start, reads):
        data[s:s + len(r)] = r
    return data, start, length


def genome_reads(seed, genome_len, n_reads, read_len, sub_rate=0.01):
    """n_reads reads of read_len bases from a random genome: sub_rate substitutions, every second read
    reverse-complemented, one terminator after each -> data (struct-read layout, fixed length)"""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, genome_len, dtype=np.int8)
    pos = rng.integers(0, genome_len - read_len + 1, n_reads)
    reads = genome[pos[:, None] + np.arange(read_len)[None, :]]
    subs = rng.random(reads.shape) < sub_rate
    reads = np.where(subs, (reads + rng.integers(1, 4, reads.shape, dtype=np.int8)) & 3, reads).astype(np.int8)
    rc = (np.arange(n_reads) & 1) == 1
    reads[rc] = 3 - reads[rc, ::-1]
    data = np.full((n_reads, read_len + 1), -1, np.int8)
    data[:, :read_len] = reads
    return data.reshape(-1)
