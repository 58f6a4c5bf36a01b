"""Digital normalisation (cfrk_global_normalize) in plain Python -- TEST INFRASTRUCTURE ONLY.

The rule of include/cfrk_abi.h, word for word: the reads are taken in rounds of `batch` consecutive reads; every read of
a round is judged against the counts as they stand at the beginning of the round -- kept iff it has a valid window and
the LOWER MEDIAN (element (W - 1) // 2 of the sorted counts of its W valid windows, an absent k-mer counting 0) is below
the cutoff -- and then every valid window of every kept read of the round adds 1 to its key.  The counts are a dict
{key: count} with the key a Python int of 2k bits, first base most significant (canonical: the smaller of the k-mer and
its reverse complement); the median is taken by sorting.  Nothing here knows how the device does it."""
import numpy as np

COUNT_MAX = 0xFFFFFFFE
MASK64 = (1 << 64) - 1


def read_keys(data, st, ln, k, canonical):
    """keys of the valid windows of the read [st, st + ln) of data, in window order; none when the range does not lie
    inside the buffer (the device form's rule for unchecked start / length)"""
    st, ln = int(st), int(ln)
    if st < 0 or ln < k or st + ln > len(data):
        return []
    mask = (1 << (2 * k)) - 1
    fwd = rc = run = 0
    out = []
    for c in data[st:st + ln].tolist():
        if c < 0 or c > 3:
            run = 0
            continue
        fwd = ((fwd << 2) | c) & mask
        rc = (rc >> 2) | ((3 - c) << (2 * (k - 1)))
        run += 1
        if run >= k:
            out.append(min(fwd, rc) if canonical else fwd)
    return out


def all_read_keys(data, start, length, k, canonical):
    data = np.asarray(data, np.int8)
    return [read_keys(data, s, l, k, canonical) for s, l in zip(start, length)]


def lower_median(values):
    s = sorted(values)
    return s[(len(s) - 1) // 2]


def normalize_keys(keys, cutoff, batch, counts=None):
    """the rule on reads given as lists of keys -> (keep uint8[nS], n_kept, counts); `counts` (a dict) is what the job
    held before and is updated in place"""
    counts = {} if counts is None else counts
    nS = len(keys)
    keep = np.zeros(nS, np.uint8)
    assert batch >= 1
    for r0 in range(0, nS, batch):
        r1 = min(r0 + batch, nS)
        for i in range(r0, r1):                                   # judge: the counts are not touched in this loop
            if keys[i] and lower_median([counts.get(x, 0) for x in keys[i]]) < cutoff:
                keep[i] = 1
        for i in range(r0, r1):                                   # insert
            if keep[i]:
                for x in keys[i]:
                    counts[x] = min(counts.get(x, 0) + 1, COUNT_MAX)
    return keep, int(keep.sum()), counts


def normalize(data, start, length, k, canonical, cutoff, batch, counts=None):
    return normalize_keys(all_read_keys(data, start, length, k, canonical), cutoff, batch, counts)


def add_keys(keys, counts=None):
    """a plain add of the reads' windows"""
    counts = {} if counts is None else counts
    for ks in keys:
        for x in ks:
            counts[x] = min(counts.get(x, 0) + 1, COUNT_MAX)
    return counts


def export_arrays(counts):
    """dict -> (lo, hi, count) sorted by (hi, lo), as GlobalCounter.export() orders the result"""
    items = sorted(counts.items())
    lo = np.array([x & MASK64 for x, _ in items], np.uint64)
    hi = np.array([x >> 64 for x, _ in items], np.uint64)
    cnt = np.array([c for _, c in items], np.uint32)
    return lo, hi, cnt


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK64
    return x ^ (x >> 31)


def digest(counts, two_word):
    """cfrk_global_digest of the counts: distinct, sum, sum of count * splitmix64(kh), xor of splitmix64(kh ^ count),
    kh = lo (k <= 32) or lo + splitmix64(hi)"""
    d = s = w = x = 0
    for key, c in counts.items():
        lo, hi = key & MASK64, key >> 64
        kh = (lo + _splitmix64(hi)) & MASK64 if two_word else lo
        d += 1
        s += c
        w = (w + c * _splitmix64(kh)) & MASK64
        x ^= _splitmix64(kh ^ c)
    return d, s & MASK64, w, x


def spectrum(counts, nbins):
    """GlobalCounter.histogram(nbins) of the counts"""
    h = np.zeros(nbins, np.uint64)
    for c in counts.values():
        h[min(c, nbins - 1)] += 1
    return h
