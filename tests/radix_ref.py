"""The radix counting path (cfrk_amd/csrc/radix.hip, global jobs with k <= 16) restated in numpy, with a key crafter and
a read-buffer builder -- TEST INFRASTRUCTURE ONLY; nothing of the product is imported here.

A key is scrambled by one odd multiply mod 4^k; the scrambled key reads, top to bottom,
    bin (b1 = 8 bits) : sub-bin (b2 bits) : counter (idx bits)            leaf = bin : sub-bin = x >> idx
RX1 sorts tiles of 8192 window starts (= bytes of the read buffer) by bin; tile t appends to sub-region t & 31 of each
bin.  RX2 splits every (bin, sub-region) region, in tiles of 8192 of its elements, by sub-bin and appends each
segment, ROUNDED UP TO EIGHT elements with pads, to its leaf.  A leaf's size n is therefore the sum over RX2 tiles of
roundup8(segment): with every region within one RX2 tile, n = sum over the 32 sub-regions of roundup8((leaf, sub)
elements).  RX3 counts a leaf in LDS: mode 1 (idx < 13: replicated 32-bit counters), mode 0 (idx = 13), mode 2 (idx
above the counter words' log2: packed 16-bit counters, only while n < 65536) or mode 3 (two passes, one per half of
the leaf's key range); a workgroup walks leaves w, w + grid, ... and buffers their entries (RX3_OB) before it takes a
range of the result list.

shape() restates the host's choice, place() where a key lands, craft() inverts it, Layout builds a buffer of reads
(k bases and one -1 per occurrence) tile by tile and recounts it from its bytes alone, predict() says what the add must
do with it.  tests/test_radix_ref_cpu.py holds all of this against the product's host function
(cfrk_debug_radix_info) and the oracle; tests/test_gpu_radix_shapes.py drives the kernels with it."""
import concurrent.futures

import numpy as np

from .hash_craft import key_to_read, revcomp_int

MUL = 0x9E3779B1
INV = pow(MUL, -1, 1 << 32)
TILE = 8192                    # RX1: window starts per tile
NREG = 32                      # sub-regions per level-1 bin
RX2_KEYS = 8192                # RX2: elements of a region per tile
GROUP = 8                      # leaf streams move in groups of eight
RX3_OB = 704                   # buffered result entries of a leaf workgroup
IDX_MAX = 13


def mix(x, k):
    """scramble: x * MUL mod 4^k (array or int -> uint64 array)"""
    x = np.atleast_1d(np.asarray(x, dtype=np.uint64))
    return (x * np.uint64(MUL)) & np.uint64((1 << (2 * k)) - 1)


def unmix(x, k):
    x = np.atleast_1d(np.asarray(x, dtype=np.uint64))
    return (x * np.uint64(INV)) & np.uint64((1 << (2 * k)) - 1)


def _pad2(b2):
    return 1.0 + 3.5 * float(1 << b2) / float(RX2_KEYS)


def shape(k, nN):
    """the host's choice for an add of nN bytes at k (radix.hip: rx_shape), same double arithmetic"""
    s = dict(b1=0, b2=0, idx=0, mul=0, inv=0, cap1=0, cap2=0, takes=False, direct=False, hi8=False)
    if k < 1 or k > 16:
        return s
    s["takes"] = True
    if k <= 7:
        s["direct"] = True
        return s
    b1 = 8
    if k == 16:
        idx = 15
        s["takes"] = float(nN) / float(1 << (8 + 9)) * _pad2(9) * 1.5 <= 49152.0
    elif 2 * k - 11 > IDX_MAX:
        b2w = 2 * k - b1 - (IDX_MAX + 1)
        per_leaf = float(nN) / float(1 << (b1 + b2w)) * _pad2(b2w)
        idx = IDX_MAX + 1 if per_leaf * 1.5 <= 49152.0 else IDX_MAX
    else:
        idx = 2 * k - 11
    b2 = 2 * k - b1 - idx
    nleaf = 1 << (b1 + b2)
    s.update(b1=b1, b2=b2, idx=idx, mul=MUL, inv=INV, hi8=2 * k - b1 >= 16)
    s["cap1"] = (int(float(nN) / float((1 << b1) * NREG) * 1.3) + 4096 + 15) & ~15
    s["cap2"] = (int(float(nN) / float(nleaf) * 1.5 * _pad2(b2)) + 1024 + 7) & ~7
    return s


def nclog(k):
    """log2 of the 32-bit counter words of a leaf workgroup"""
    return 14 if k == 16 else 13


def place(keys, k, sh):
    """-> dict of int64 arrays: x (scrambled key), bin, leaf, counter, l1 (the 2k - 8 bits below the bin)"""
    x = mix(keys, k).astype(np.int64)
    low = 2 * k - sh["b1"]
    return dict(x=x, bin=x >> low, l1=x & ((1 << low) - 1), leaf=x >> sh["idx"], counter=x & ((1 << sh["idx"]) - 1))


def canonical_ok(key, k):
    return key <= revcomp_int(key, k)


def craft(k, sh, leaf, counter, canonical=False):
    """the raw key that lands on `counter` of `leaf`; canonical: None unless the key is its own canonical form"""
    assert 0 <= leaf < (1 << (sh["b1"] + sh["b2"])) and 0 <= counter < (1 << sh["idx"])
    key = int(unmix((leaf << sh["idx"]) | counter, k)[0])
    return key if (not canonical or canonical_ok(key, k)) else None


def craft_some(k, sh, leaf, n, rng, canonical=False, avoid=()):
    """n distinct keys of `leaf` on random counters (canonical: only keys that are their own canonical form)"""
    got, seen = [], set(avoid)
    for c in rng.permutation(1 << sh["idx"]):
        key = craft(k, sh, leaf, int(c), canonical)
        if key is not None and key not in seen:
            got.append(key)
            seen.add(key)
            if len(got) == n:
                return got
    raise ValueError(f"leaf {leaf} of k={k} has only {len(got)} such keys")


def _revcomp_arr(x, k):
    x = x.copy()
    r = np.zeros_like(x)
    for _ in range(k):
        r = (r << np.uint64(2)) | (np.uint64(3) - (x & np.uint64(3)))
        x >>= np.uint64(2)
    return r


def kmers_of(data, k, canonical):
    """every k-mer of an int8 buffer from its bytes alone -> (start positions, keys), keys canonical when asked"""
    data = np.asarray(data, np.int8)
    bad = np.concatenate([[0], np.cumsum((data < 0) | (data > 3))])
    if len(data) < k:
        return np.zeros(0, np.int64), np.zeros(0, np.uint64)
    starts = np.nonzero(bad[k:] - bad[:-k] == 0)[0]
    keys = np.zeros(len(starts), np.uint64)
    for j in range(k):
        keys = (keys << np.uint64(2)) | data[starts + j].astype(np.uint64)
    if canonical:
        keys = np.minimum(keys, _revcomp_arr(keys, k))
    return starts, keys


class Built:
    """a finished buffer: data (int8), counts {key: count}, and what its bytes say about where everything lands:
    region {(bin, sub): elements}, seg {(leaf, sub): elements}, leaf_lo / leaf_hi {leaf: bounds of n} (equal while
    every region fits one RX2 tile: n_exact), entries {leaf: distinct keys}"""


class Layout:
    """Reads laid into chosen RX1 tiles: one read of k bases and one -1 per occurrence, the rest of every tile -1."""

    def __init__(self, k, canonical=False):
        self.k, self.canonical = k, canonical
        self.per_tile = TILE // (k + 1)
        self.fill = {}                   # tile -> bytes used
        self.chunks = []                 # (tile, byte offset inside the tile, int8 block)
        self.counts = {}

    def _canon(self, key):
        return min(key, revcomp_int(key, self.k)) if self.canonical else key

    def room(self, tile):
        return (TILE - self.fill.get(tile, 0)) // (self.k + 1)

    def put(self, key, copies, tile):
        """`copies` reads of the key, all starting inside `tile`"""
        assert copies >= 1 and copies <= self.room(tile), (copies, tile, self.room(tile))
        row = np.append(key_to_read(key, 0, self.k), np.int8(-1))
        off = self.fill.get(tile, 0)
        self.chunks.append((tile, off, np.tile(row, copies)))
        self.fill[tile] = off + copies * (self.k + 1)
        c = self._canon(key)
        self.counts[c] = self.counts.get(c, 0) + copies

    def put_sub(self, key, copies, sub):
        """`copies` reads of the key in tiles sub, sub + 32, ... (sub-region `sub` of its bin), first fit"""
        t = sub
        while copies:
            n = min(copies, self.room(t))
            if n:
                self.put(key, n, t)
                copies -= n
            t += NREG

    def put_spread(self, key, copies, multiple=1):
        """over the 32 sub-regions as evenly as whole multiples of `multiple` allow (the remainder on the last)"""
        per = copies // NREG // multiple * multiple
        for s in range(NREG):
            n = per if s < NREG - 1 else copies - per * (NREG - 1)
            if n:
                self.put_sub(key, n, s)

    def put_read(self, bases, tile):
        """any read (int8 codes); it must start and end inside `tile`"""
        bases = np.asarray(bases, np.int8)
        off = self.fill.get(tile, 0)
        assert off + len(bases) + 1 <= TILE
        self.chunks.append((tile, off, np.append(bases, np.int8(-1))))
        self.fill[tile] = off + len(bases) + 1
        for key in kmers_of(bases, self.k, self.canonical)[1]:
            self.counts[int(key)] = self.counts.get(int(key), 0) + 1

    def seg_now(self, leaf, sh):
        """elements of `leaf` per sub-region so far (from the intended counts' positions: by recount)"""
        b = self.finish(sh=sh, check_n=False)
        return [b.seg.get((leaf, s), 0) for s in range(NREG)]

    def top_up(self, leaf, n_target, filler, sh):
        """copies of `filler` (a key of `leaf`) so that the leaf's n becomes exactly n_target: every sub-region's
        segment is first made a multiple of eight, the rest goes on in eights"""
        assert int(place([self._canon(filler)], self.k, sh)["leaf"][0]) == leaf
        seg = self.seg_now(leaf, sh)
        for s in range(NREG):
            if seg[s] % GROUP:
                self.put_sub(filler, GROUP - seg[s] % GROUP, s)
                seg[s] += GROUP - seg[s] % GROUP
        rest = n_target - sum(seg)
        assert rest >= 0 and rest % GROUP == 0, (n_target, sum(seg))
        for s in range(NREG):
            n = min(rest, max(0, 2048 - seg[s]))          # (2048 per sub-region: the bin's regions stay far below a tile)
            if n:
                self.put_sub(filler, n, s)
                rest -= n
        assert rest == 0, "more than 32 x 2048 elements asked for"

    def finish(self, sh=None, min_tiles=0, check_n=True):
        """-> Built.  The buffer is recounted FROM ITS BYTES: every k-mer's start gives its tile and sub-region, its key
        the bin, leaf and counter; the recount must equal the intended multiset.  sh: the shape to place by (default: the
        one of the buffer's own size).  check_n: every region must fit one RX2 tile, so that n is exact."""
        k = self.k
        ntiles = max([t + 1 for t in self.fill] + [min_tiles, 1])
        data = np.full(ntiles * TILE, -1, np.int8)
        for tile, off, block in self.chunks:
            data[tile * TILE + off: tile * TILE + off + len(block)] = block
        b = Built()
        b.k, b.canonical, b.data = k, self.canonical, data
        b.counts = dict(self.counts)
        b.sh = sh if sh is not None else shape(k, len(data))
        starts, keys = kmers_of(data, k, self.canonical)
        uk, uc = np.unique(keys, return_counts=True)
        assert {int(a): int(c) for a, c in zip(uk, uc)} == b.counts, "the buffer does not hold the intended multiset"
        b.keys_sorted, b.counts_sorted = uk, uc.astype(np.uint64)
        b.region, b.seg, b.leaf_lo, b.leaf_hi, b.entries = {}, {}, {}, {}, {}
        b.n_exact = True
        if b.sh["direct"] or not len(keys):
            return b
        sub = (starts // TILE) & (NREG - 1)
        p = place(keys, k, b.sh)
        for name, ident in (("region", p["bin"]), ("seg", p["leaf"])):
            u, c = np.unique(ident * NREG + sub, return_counts=True)
            getattr(b, name).update({(int(x) // NREG, int(x) % NREG): int(n) for x, n in zip(u, c)})
        b.n_exact = max(b.region.values()) <= RX2_KEYS
        assert b.n_exact or not check_n, "a region above one RX2 tile: n is not determined"
        for (leaf, s), n in b.seg.items():
            # a region of T tiles cuts a segment into at most T pieces, each rounded up on its own (<= 7 pads a piece)
            tiles = (b.region[(leaf >> b.sh["b2"], s)] + RX2_KEYS - 1) // RX2_KEYS
            up = (n + GROUP - 1) // GROUP * GROUP
            b.leaf_lo[leaf] = b.leaf_lo.get(leaf, 0) + up
            b.leaf_hi[leaf] = b.leaf_hi.get(leaf, 0) + (up if tiles == 1 else n + (GROUP - 1) * min(tiles, n))
        ul, cl = np.unique(place(uk, k, b.sh)["leaf"], return_counts=True)
        b.entries = {int(l): int(c) for l, c in zip(ul, cl)}
        return b


def _windows(code, k, rev):
    """the k-base window starting at every position of a uint32 array of 2-bit codes (first base most significant; rev:
    LAST base most significant, for a reverse complement), built from windows of 1, 2, 4, 8 bases: log k passes"""
    pow2, L = {1: code}, 1
    while 2 * L <= k:
        w = pow2[L]
        pow2[2 * L] = ((w[L:] << np.uint32(2 * L)) | w[:-L]) if rev else ((w[:-L] << np.uint32(2 * L)) | w[L:])
        L *= 2
    acc, a = None, 0
    while L:
        if k & L:
            if acc is None:
                acc, a = pow2[L], L
            else:
                m = len(code) - (a + L) + 1
                piece = pow2[L][a:a + m]
                acc = ((piece << np.uint32(2 * a)) | acc[:m]) if rev else ((acc[:m] << np.uint32(2 * L)) | piece)
                a += L
        L //= 2
    return acc[:len(code) - k + 1]


def survey(data, k, canonical, chunk=1 << 22, threads=1):
    """What Layout.finish() says about a buffer's placement -- region, seg, leaf_lo / leaf_hi, n_exact -- for ANY buffer,
    from its bytes alone and in chunks, so that it also serves one of 10^8 bytes (no multiset: counts / entries stay
    empty) -> Built."""
    data = np.asarray(data, np.int8)
    b = Built()
    b.k, b.canonical, b.data, b.sh = k, canonical, data, shape(k, len(data))
    b.counts, b.entries = {}, {}
    sh = b.sh
    assert not sh["direct"] and chunk % TILE == 0
    nb, nl = 1 << sh["b1"], 1 << (sh["b1"] + sh["b2"])
    region, seg = np.zeros(nb * NREG, np.int64), np.zeros(nl * NREG, np.int64)
    full = np.uint32((1 << (2 * k)) - 1)
    def one(c0):
        d = data[c0:c0 + chunk + k - 1]
        m = len(d) - k + 1                                    # window starts of this chunk
        if m <= 0:
            return None
        bad = np.concatenate([[0], np.cumsum((d < 0) | (d > 3), dtype=np.int32)])
        ok = bad[k:] == bad[:-k]
        if not ok.any():
            return None
        code = (d & 3).astype(np.uint32)
        key = _windows(code, k, False)
        if canonical:
            key = np.minimum(key, _windows(np.uint32(3) - code, k, True))
        x = ((key * np.uint32(MUL)) & full)[ok].astype(np.int64)       # (uint32 products wrap mod 2^32, as the device's do)
        sub = (((c0 + np.nonzero(ok)[0]) // TILE) & (NREG - 1)).astype(np.int64)
        return (np.bincount((x >> (2 * k - sh["b1"])) * NREG + sub, minlength=len(region)),
                np.bincount((x >> sh["idx"]) * NREG + sub, minlength=len(seg)))
    starts = range(0, len(data), chunk)
    if threads > 1:                                           # (numpy releases the interpreter lock in these passes)
        with concurrent.futures.ThreadPoolExecutor(threads) as pool:
            parts = list(pool.map(one, starts))
    else:
        parts = [one(c0) for c0 in starts]
    for part in parts:
        if part is not None:
            region += part[0]
            seg += part[1]
    b.region = {(int(i) // NREG, int(i) % NREG): int(region[i]) for i in np.nonzero(region)[0]}
    b.seg = {(int(i) // NREG, int(i) % NREG): int(seg[i]) for i in np.nonzero(seg)[0]}
    tiles = np.repeat(((region + RX2_KEYS - 1) // RX2_KEYS).reshape(nb, NREG), 1 << sh["b2"], axis=0).reshape(-1)
    up = (seg + GROUP - 1) // GROUP * GROUP
    hi = np.where(tiles <= 1, up, seg + (GROUP - 1) * np.minimum(tiles, seg))
    lo_l, hi_l = up.reshape(nl, NREG).sum(1), hi.reshape(nl, NREG).sum(1)
    b.leaf_lo = {int(l): int(lo_l[l]) for l in np.nonzero(lo_l)[0]}
    b.leaf_hi = {int(l): int(hi_l[l]) for l in np.nonzero(lo_l)[0]}
    b.n_exact = int(region.max()) <= RX2_KEYS
    return b


def leaf_mode(k, sh, n_lo, n_hi):
    """the leaf kernel's mode for a leaf of n elements (n_lo <= n <= n_hi); the bounds must agree on it"""
    if sh["idx"] <= nclog(k):
        return 1 if sh["idx"] < nclog(k) else 0
    assert (n_lo < 65536) == (n_hi < 65536), "the mode depends on an n that is not determined"
    return 2 if n_hi < 65536 else 3


def predict(b, grid=None):
    """what an add of the buffer must do -> dict: mode {leaf: 0..3}, entries {leaf: distinct keys}, relaid1 / relaid2
    (level 1 / the leaves overflow their fixed strides cap1 / cap2 and are laid out again), attempts of the layout loop;
    with the leaf kernel's grid also walks(w): the leaves workgroup w counts, in order."""
    sh = b.sh
    out = dict(mode={l: leaf_mode(b.k, sh, b.leaf_lo[l], b.leaf_hi[l]) for l in b.leaf_lo}, entries=dict(b.entries))
    out["relaid1"] = max(b.region.values()) > sh["cap1"]
    lo, hi = max(b.leaf_lo.values()), max(b.leaf_hi.values())
    assert (lo > sh["cap2"]) == (hi > sh["cap2"]), "whether the leaves overflow depends on an n that is not determined"
    out["relaid2"] = lo > sh["cap2"]
    out["attempts"] = 1 + int(out["relaid1"]) + int(out["relaid2"])
    if grid:
        nleaf = 1 << (sh["b1"] + sh["b2"])
        out["walks"] = lambda w: list(range(w, nleaf, grid))
    return out
