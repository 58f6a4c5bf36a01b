"""The partition rule of the minimizer-partitioned counting paths in plain numpy -- TEST INFRASTRUCTURE ONLY.

Written from the rule as the device code documents it, never from device output:

  msp.hip: msp_params          one-word keys (16 <= k <= 32): window W = min(k - 11 (k <= 26) or k - 12, 49 - k) m-mers of
                               m = k - W + 1 bases, no margin
  msp2.hip: msp2_window,       two-word keys (33 <= k <= 64): m = 13 (even k) / 14 (odd k), window W2 = min(k - m + 1 - 2, 30),
    msp2_count_tiles           margin c = (k - m + 1 - W2) / 2 m-mers on either side of the window
  msp_dev.h: hash_mmer,        ordering value of the m-mer that starts at buffer offset q:
    msp_minimizers, leaf_of      ((min(fwd, revcomp) * 0x9E3779B1) mod 2^32) & ~127 | (q & 31)
                               -- the low bits are the m-mer's position in its 32-byte chunk: equal hashes inside one window
                               (< 32 positions) are told apart by where they lie in the BUFFER (the tie rule);
                               leaf = bits 8..23 of the window's minimum; bits 24..27 and 7 are the five sub-value bits
  msp.hip: p1_tile / build     a run = a maximal stretch of consecutive valid k-mers (all k codes in 0..3) with the same
  msp2.hip: q1_build           minimizer OCCURRENCE; its left (right) end is closed iff the k-mer before (after) it is valid
  msp_runs.h, RunsFmt1/2       the one-shot packed form of a CFRK_RUNS_ONLY job: decode_packed / encode_packed
"""
import collections

import numpy as np

HASH_MUL = 0x9E3779B1
NLEAF = 1 << 16
NOTES_PER_ROW = 8
NO_NOTE = 0xFFFF
LEFT, RIGHT = 64, 128                 # header bits 6 and 7: the run's left / right end is closed

Params = collections.namedtuple("Params", "k m W c two max_bases")


def params(k):
    if 16 <= k <= 32:
        W = min(k - 11 if k <= 26 else k - 12, 49 - k)
        return Params(k, k - W + 1, W, 0, False, 48)
    if 33 <= k <= 64:
        m = 14 if k & 1 else 13
        nm = k - m + 1
        W = min(nm - 2, 30)
        assert (nm - W) % 2 == 0
        return Params(k, m, W, (nm - W) // 2, True, 96)
    raise ValueError("no partitioned path for k=%d" % k)


def ordering_values(data, m):
    """packed ordering value of the m-mer at every offset q <= len(data) - m (uint64, < 2^32); meaningless where the
    m-mer holds an invalid code -- no valid k-mer looks at such a value"""
    data = np.asarray(data, np.int8)
    nq = len(data) - m + 1
    if nq <= 0:
        return np.zeros(0, np.uint64)
    code = (data.astype(np.int64) & 3).astype(np.uint64)
    f = np.zeros(nq, np.uint64)
    r = np.zeros(nq, np.uint64)
    for i in range(m):
        b = code[i:i + nq]
        f = (f << np.uint64(2)) | b
        r |= (np.uint64(3) - b) << np.uint64(2 * i)
    h = (np.minimum(f, r) * np.uint64(HASH_MUL)) & np.uint64(0xFFFFFFFF)
    q = np.arange(nq, dtype=np.uint64)
    return (h & np.uint64(0xFFFFFF80)) | (q & np.uint64(31))


def valid_kmers(data, k):
    """bool per offset s <= len(data) - k: all k codes from s on are in 0..3"""
    data = np.asarray(data, np.int8)
    if len(data) < k:
        return np.zeros(0, bool)
    ok = np.concatenate([[0], np.cumsum((data >= 0) & (data <= 3))])
    return (ok[k:] - ok[:-k]) == k


class Runs:
    """the runs of a buffer: arrays first (offset of the first k-mer), n (k-mers), leaf, left, right (closed ends), sub
    (bits 24..27 and 7 of the minimum, bit 7 lowest), occ (offset of the minimizer occurrence)"""

    def __init__(self, data, k, first, n, leaf, left, right, sub, occ):
        self.data, self.k = data, k
        self.first, self.n, self.leaf, self.left, self.right, self.sub, self.occ = first, n, leaf, left, right, sub, occ

    def __len__(self):
        return len(self.first)

    def bases(self, i):
        """the n + k - 1 bases of run i"""
        a = int(self.first[i])
        return self.data[a:a + int(self.n[i]) + self.k - 1]

    def flags(self):
        return (self.left.astype(np.int64) * LEFT) | (self.right.astype(np.int64) * RIGHT)

    def records(self):
        """[(bases as bytes, n, flags, leaf)] per run"""
        fl = self.flags()
        return [(self.bases(i).tobytes(), int(self.n[i]), int(fl[i]), int(self.leaf[i])) for i in range(len(self))]


def runs(data, k):
    data = np.ascontiguousarray(data, np.int8)
    p = params(k)
    valid = valid_kmers(data, k)
    ns = len(valid)
    empty = np.zeros(0, np.int64)
    if ns == 0 or not valid.any():
        return Runs(data, k, empty, empty, empty, empty.astype(bool), empty.astype(bool), empty, empty)
    h = ordering_values(data, p.m)
    # window of the k-mer at s: the m-mers at s + c .. s + c + W - 1, all inside the k-mer (c + W + m - 1 <= k)
    assert p.c + p.W + p.m - 1 <= k
    key = (h << np.uint64(32)) | np.arange(len(h), dtype=np.uint64)      # minimum by ordering value; it names its offset
    wmin = key[p.c:p.c + ns].copy()
    for j in range(1, p.W):
        np.minimum(wmin, key[p.c + j:p.c + j + ns], out=wmin)
    occ = (wmin & np.uint64(0xFFFFFFFF)).astype(np.int64)
    hmin = (wmin >> np.uint64(32)).astype(np.int64)
    prev_valid = np.concatenate([[False], valid[:-1]])
    next_valid = np.concatenate([valid[1:], [False]])
    prev_occ = np.concatenate([[-1], occ[:-1]])
    start = valid & (~prev_valid | (occ != prev_occ))
    first = np.flatnonzero(start)
    rid = np.cumsum(start) - 1                                            # run of every valid k-mer
    n = np.bincount(rid[valid], minlength=len(first)).astype(np.int64)
    last = first + n - 1
    hm = hmin[first]
    return Runs(data, k, first, n, (hm >> 8) & 0xFFFF, prev_valid[first], next_valid[last],
                (((hm >> 24) & 15) << 1) | ((hm >> 7) & 1), occ[first])


# ---------------------------------------------------------------------------- k-mers of the runs

def kmer_keys(data, k, canonical):
    """(lo, hi) uint64 per offset s <= len(data) - k: the k-mer's key, first base most significant, hi = bits 64..127;
    the smaller of the two strands when canonical"""
    data = np.asarray(data, np.int8)
    ns = len(data) - k + 1
    code = (data.astype(np.int64) & 3).astype(np.uint64)
    two, three, one = np.uint64(2), np.uint64(3), np.uint64(1)
    flo, fhi = np.zeros(ns, np.uint64), np.zeros(ns, np.uint64)
    rlo, rhi = np.zeros(ns, np.uint64), np.zeros(ns, np.uint64)
    for i in range(k):
        b = code[i:i + ns]
        fhi = (fhi << two) | (flo >> np.uint64(62))
        flo = (flo << two) | b
        cb = three - b                                                   # base i of the k-mer is base k - 1 - i of its reverse complement
        if 2 * i < 64:
            rlo |= cb << np.uint64(2 * i)
        else:
            rhi |= cb << np.uint64(2 * i - 64)
    if k < 32:
        flo &= (one << np.uint64(2 * k)) - one
    if 32 < k < 64:
        fhi &= (one << np.uint64(2 * k - 64)) - one
    if k <= 32:
        fhi[:] = 0
    if not canonical:
        return flo, fhi
    take_r = (rhi < fhi) | ((rhi == fhi) & (rlo < flo))
    return np.where(take_r, rlo, flo), np.where(take_r, rhi, fhi)


def expand(rr, canonical):
    """every k-mer of every run, counted -> (lo, hi, count) sorted by (hi, lo), the form of oracle_lib.global_count"""
    if len(rr) == 0:
        z = np.zeros(0, np.uint64)
        return z, z, z
    lo, hi = kmer_keys(rr.data, rr.k, canonical)
    tot = int(rr.n.sum())
    base = np.repeat(rr.first - np.concatenate([[0], np.cumsum(rr.n)[:-1]]), rr.n)
    pos = base + np.arange(tot)
    return count_keys(lo[pos], hi[pos])


def count_keys(lo, hi):
    order = np.lexsort((lo, hi))
    lo, hi = lo[order], hi[order]
    new = np.ones(len(lo), bool)
    new[1:] = (lo[1:] != lo[:-1]) | (hi[1:] != hi[:-1])
    at = np.flatnonzero(new)
    cnt = np.diff(np.concatenate([at, [len(lo)]])).astype(np.uint64)
    return lo[at], hi[at], cnt


def covered_positions(rr):
    """how many runs hold the k-mer at every offset (the partition property: 1 where the k-mer is valid, else 0)"""
    cover = np.zeros(max(len(rr.data) - rr.k + 1, 0) + 1, np.int64)
    np.add.at(cover, rr.first, 1)
    np.add.at(cover, rr.first + rr.n, -1)
    return np.cumsum(cover)[:-1]


# ---------------------------------------------------------------------------- per-leaf view, packed form

def by_leaf(rr):
    """{leaf: (Counter{(bases, n): multiplicity} of the complete runs, Counter{(bases, n, flags): count} of the truncated)}"""
    out = {}
    for bases, n, fl, leaf in rr.records():
        comp, trunc = out.setdefault(leaf, (collections.Counter(), collections.Counter()))
        if fl == (LEFT | RIGHT):
            comp[(bases, n)] += 1
        else:
            trunc[(bases, n, fl)] += 1
    return out


_SHIFTS = (30 - 2 * np.arange(16)).astype(np.uint32)


def _pack_bases(bases, two):
    """2 bits per base, first base in the top bits of word 0; one-word keys: 3 words (48 bases), two-word: 6 (96)"""
    nw = 6 if two else 3
    b = np.frombuffer(bases, np.int8).astype(np.int64)
    assert len(b) <= 16 * nw and ((b >= 0) & (b <= 3)).all()
    w = [0] * nw
    for i, x in enumerate(b):
        w[i >> 4] |= int(x) << (30 - 2 * (i & 15))
    return w


def _unpack_bases(words, nbases):
    """-> bases as bytes; asserts that the bits behind them are clear (equal runs are byte-identical records)"""
    b = ((np.asarray(words, np.uint32)[:, None] >> _SHIFTS) & np.uint32(3)).reshape(-1).astype(np.int8)
    assert not b[nbases:].any(), "bases behind the run's last k-mer are not cleared"
    out = b[:nbases]
    return out.tobytes()


def _record(bases, header, two):
    w = _pack_bases(bases, two)
    return w + [header] if not two else w + [0, header]      # RunsFmt1: {x, y, z, w}; RunsFmt2: a = words 0..3, b = {4, 5, spare, header}


def encode_packed(leaves, k, notes=None):
    """{leaf: (complete Counter, truncated Counter)} -> the one-shot packed segment of ONE owner (parts = 1) as uint32
    [rows, 4] (msp_runs.h): header = (distinct, truncated, noted) per leaf padded to whole 16-byte rows; then leaf after
    leaf its distinct complete runs (header word multiplicity << 6 | n - 1), its truncated runs as records (leaf << 8 |
    flags | n - 1), its notes (16 bits: list position of the twin << 5 | n - 1, eight per row, the last row padded with
    0xFFFF).  notes: {leaf: [(position, n)]} or None.  The complete runs of a leaf are listed in sorted order."""
    two = params(k).two
    rows_per = 2 if two else 1
    hdr = np.zeros((NLEAF, 3), np.uint32)
    body = []
    for leaf in sorted(leaves):
        comp, trunc = leaves[leaf]
        nt = notes.get(leaf, []) if notes else []
        hdr[leaf] = (len(comp), sum(trunc.values()), len(nt))
        for (bases, n), mult in sorted(comp.items()):
            assert 1 <= mult < 1 << 26
            body += _record(bases, (mult << 6) | (n - 1), two)
        for (bases, n, fl), cnt in sorted(trunc.items()):
            assert fl != (LEFT | RIGHT)
            body += _record(bases, (leaf << 8) | fl | (n - 1), two) * cnt
        if nt:
            half = [(pos << 5) | (n - 1) for pos, n in nt]
            half += [NO_NOTE] * (-len(half) % NOTES_PER_ROW)
            body += [half[2 * i] | (half[2 * i + 1] << 16) for i in range(len(half) // 2)]
    hw = hdr.reshape(-1)
    hw = np.concatenate([hw, np.zeros(-len(hw) % 4, np.uint32)])
    assert len(body) % (4 * rows_per) == 0 or notes
    return np.concatenate([hw, np.array(body, np.uint64).astype(np.uint32)]).reshape(-1, 4)


def decode_packed(rows, k):
    """the packed segment of one owner with parts = 1 (uint32 [rows, 4]) -> ({leaf: (complete Counter, truncated Counter)},
    header triples uint32 [65536, 3]).  A note becomes the run it stands for (msp_runs.h: runs_scatter): the first n k-mers
    of the distinct complete run at its list position, closed on the left only."""
    two = params(k).two
    rows = np.ascontiguousarray(rows, np.uint32).reshape(-1, 4)
    hrows = (NLEAF * 12 + 15) // 16
    hdr = rows[:hrows].reshape(-1)[:3 * NLEAF].reshape(NLEAF, 3)
    rper, nw = (2, 6) if two else (1, 3)
    at, out = hrows, {}
    for leaf in np.flatnonzero(hdr.any(axis=1)):
        nd, nu, na = (int(x) for x in hdr[leaf])
        comp, trunc, listed = collections.Counter(), collections.Counter(), []

        def rec(i):
            w = rows[at + rper * i:at + rper * (i + 1)].reshape(-1)
            return w[:nw], int(w[7] if two else w[3])
        for i in range(nd):
            w, h = rec(i)
            n, mult = (h & 63) + 1, h >> 6
            assert mult >= 1
            bases = _unpack_bases(w, n + k - 1)
            listed.append((bases, n))
            comp[(bases, n)] += mult
        at += rper * nd
        for i in range(nu):
            w, h = rec(i)
            n, fl = (h & 63) + 1, h & (LEFT | RIGHT)
            assert (h >> 8) & 0xFFFF == leaf and h >> 24 == 0 and fl != (LEFT | RIGHT)
            trunc[(_unpack_bases(w, n + k - 1), n, fl)] += 1
        at += rper * nu
        nrows = (na + NOTES_PER_ROW - 1) // NOTES_PER_ROW
        half = rows[at:at + nrows].reshape(-1).view(np.uint16)
        for i in range(na):
            note = int(half[i])
            assert note != NO_NOTE and nd > 0
            tb, tn = listed[note >> 5]
            n = (note & 31) + 1
            assert n <= tn
            trunc[(tb[:n + k - 1], n, LEFT)] += 1
        assert (half[na:] == NO_NOTE).all()
        at += nrows
        out[int(leaf)] = (comp, trunc)
    assert at == len(rows), "the header triples do not add up to the segment's rows"
    return out, hdr
