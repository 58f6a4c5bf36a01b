"""The crafted buffers of tests/test_gpu_radix_shapes.py, built with tests/radix_ref.py -- shared with
tests/test_radix_ref_cpu.py, which recounts every one of them with the oracle.  Every function returns a radix_ref.Built
(or a list of them) whose construction has been asserted from its bytes; `note` on it names what the case relies on.
GRID: the leaf kernel's grid a case is built for when no device says otherwise (256 CUs: 4 workgroups per CU, 2 at
k = 16); the GPU tests pass the grid the product reports."""
import functools

import numpy as np

from . import radix_ref as rr

NOMINAL = 1 << 20           # placement (b1, b2, idx) does not depend on the size below ~1e8 bytes: asserted per case


def GRID(k):
    return 512 if k == 16 else 1024


def _rng(*a):
    return np.random.default_rng([int(x) for x in a] + [58])


def _sh(k):
    return rr.shape(k, NOMINAL)


def _done(lay, sh, note, **kw):
    b = lay.finish(**kw)
    assert (b.sh["b1"], b.sh["b2"], b.sh["idx"]) == (sh["b1"], sh["b2"], sh["idx"]), "the buffer's size changed the shape"
    b.note = note
    b.data.setflags(write=False)
    return b


def find_leaf(k, sh, counters, canonical, leaves):
    """the first of `leaves` in which every one of `counters` has a key (canonical: that is its own canonical form)"""
    for leaf in leaves:
        keys = [rr.craft(k, sh, leaf, c, canonical) for c in counters]
        if all(x is not None for x in keys):
            return leaf, keys
    raise ValueError("no such leaf")


# --------------------------------------------------------------------------------------------------------- a
@functools.lru_cache(maxsize=None)
def case_a(k, canonical=False):
    """one leaf of packed 16-bit counters at n = 65528: pairs (2c, 2c + 1) with counts (1, N), (N, 1), (N, N), and
    counter 0, counter 2^idx - 1, one in each half"""
    sh = _sh(k)
    assert sh["idx"] > rr.nclog(k)
    top, N = (1 << sh["idx"]) - 1, 15000
    counts = [1, N, N, 1, N, N, 3, 5, 7, 11]
    leaf, _ = find_leaf(k, sh, [0, top], canonical, range(300, 1 << (sh["b1"] + sh["b2"])))

    def first(cands):               # the first candidate tuple of counters whose keys all exist (canonical filter)
        return next(c for c in cands if all(rr.craft(k, sh, leaf, x, canonical) is not None for x in c))
    half = (top + 1) // 2
    counters = list(first((2 * c, 2 * c + 1) for c in range(1000, half // 2))) + \
        list(first((2 * c, 2 * c + 1) for c in range(half // 2 + 1000, half))) + \
        list(first((2 * c, 2 * c + 1) for c in range(half - 2, half // 2, -1))) + [0, top] + \
        list(first((c,) for c in range(half // 2, half))) + list(first((c,) for c in range(half + half // 2 + 1, top))) + \
        list(first((c,) for c in range(777, half)))
    assert len(set(counters)) == 11
    keys = [rr.craft(k, sh, leaf, c, canonical) for c in counters]
    lay = rr.Layout(k, canonical)
    for key, c in zip(keys, counts):
        lay.put_spread(key, c, 8)
    lay.top_up(leaf, 65528, keys[-1], sh)
    b = _done(lay, sh, "n = 65528: mode 2")
    assert b.leaf_lo == {leaf: 65528} and b.n_exact and rr.predict(b)["mode"][leaf] == 2
    b.leaf = leaf
    return b


# --------------------------------------------------------------------------------------------------------- b
@functools.lru_cache(maxsize=None)
def case_b(k, n, canonical=False):
    """a single even counter holds all n elements of its leaf, n = 65528 (packed counters) or 65536 (two passes)"""
    sh = _sh(k)
    leaf, (key, odd) = find_leaf(k, sh, [4242, 4243], canonical, range(555, 1 << (sh["b1"] + sh["b2"])))
    lay = rr.Layout(k, canonical)
    lay.top_up(leaf, n, key, sh)
    b = _done(lay, sh, "one key, n elements")
    assert b.counts == {key: n} and b.leaf_lo == {leaf: n} and b.n_exact
    assert all(v % 8 == 0 for v in b.seg.values())
    assert rr.predict(b)["mode"][leaf] == (2 if n < 65536 else 3)
    b.leaf, b.odd = leaf, odd
    return b


# --------------------------------------------------------------------------------------------------------- c
@functools.lru_cache(maxsize=None)
def case_c(k, grid, canonical=False):
    """a two-pass leaf with keys at the first and last counter of each half, and a packed leaf the same workgroup walked
    before it and one it walks next"""
    sh = _sh(k)
    H = 1 << (sh["idx"] - 1)
    assert sh["idx"] == rr.nclog(k) + 1
    leaf = grid + 5
    ok = lambda c: rr.craft(k, sh, leaf, c, canonical) is not None
    # (canonical run: the nearest counters whose keys are their own canonical form)
    counters = [next(c for c in range(0, H) if ok(c)), next(c for c in range(H - 1, 0, -1) if ok(c)),
                next(c for c in range(H, 2 * H) if ok(c)), next(c for c in range(2 * H - 1, H, -1) if ok(c))]
    counters += [next(c for c in range(counters[0] + 17, H) if ok(c)), next(c for c in range(counters[2] + 17, 2 * H) if ok(c))]
    assert canonical or counters[:4] == [0, H - 1, H, 2 * H - 1]
    counts = [1, 70000, 40000, 1, 300, 9]
    keys = [rr.craft(k, sh, leaf, c, canonical) for c in counters]
    lay = rr.Layout(k, canonical)
    for key, c in zip(keys, counts):
        lay.put_spread(key, c)
    rng = _rng(k, grid, canonical)
    big = {}
    for other, pairs in ((leaf - grid, [(40, 3), (41, 9)]), (leaf + grid, [(2 * H - 2, 2), (2 * H - 1, 60000)])):
        for key in rr.craft_some(k, sh, other, 5, rng, canonical):
            lay.put_sub(key, 4, int(rng.integers(0, 32)))
        for c, n in pairs:
            # (canonical run: the nearest counter below whose key is its own canonical form and still unused)
            key = next(x for x in (rr.craft(k, sh, other, cc, canonical) for cc in range(c, -1, -1))
                       if x is not None and x not in lay.counts)
            lay.put_spread(key, n)
            big[other] = big.get(other, 0) + n
    b = _done(lay, sh, "modes 2, 3, 2 in one workgroup")
    p = rr.predict(b, grid)
    assert b.n_exact and not p["relaid1"] and p["mode"][leaf] == 3 and p["mode"][leaf - grid] == 2 and p["mode"][leaf + grid] == 2
    assert all(b.leaf_lo[l] >= n for l, n in big.items()) and b.leaf_lo[leaf + grid] >= 60000     # (nothing vanished)
    w = p["walks"](leaf % grid)
    assert w[w.index(leaf) - 1] == leaf - grid and w[w.index(leaf) + 1] == leaf + grid
    pl = rr.place(list(b.counts), k, sh)
    inleaf = pl["counter"][pl["leaf"] == leaf]
    assert set(counters) <= set(inleaf.tolist())
    b.leaf = leaf
    return b


# --------------------------------------------------------------------------------------------------------- d
@functools.lru_cache(maxsize=None)
def case_d(k, canonical=False):
    """keys that look like pads: level-1 value all ones, counter all ones, raw and scrambled 0 and 4^k - 1; poly-A and
    poly-T reads of 200 bases"""
    sh = _sh(k)
    full = (1 << (2 * k)) - 1
    keys = [0, full, int(rr.unmix(full, k)[0]), int(rr.unmix(0, k)[0])]
    if not sh["direct"]:
        low = 2 * k - sh["b1"]
        for bin_ in (0, 1, 77, 128, 255):
            for l1 in ((1 << low) - 1, (1 << low) - 2, (1 << 16) - 1 if low > 16 else 1, ((1 << low) - 1) ^ 0xFFFF if low > 16 else 2):
                keys.append(int(rr.unmix((bin_ << low) | l1, k)[0]))
        for leaf in (3, 1000, (1 << (sh["b1"] + sh["b2"])) - 1):
            keys.append(rr.craft(k, sh, leaf, (1 << sh["idx"]) - 1))
    lay = rr.Layout(k, canonical)
    seen = set()
    for i, key in enumerate(keys):
        if key in seen or (canonical and not rr.canonical_ok(key, k)):
            continue
        seen.add(key)
        lay.put(key, 1 + i % 9, i % 5)
    for t, base in ((1, 0), (2, 3), (33, 0), (34, 3)):
        lay.put_read(np.full(200, base, np.int8), t)
    b = _done(lay, sh, "look-alikes")
    if not sh["direct"]:
        p = rr.place(list(b.counts), k, sh)
        low = 2 * k - sh["b1"]
        assert canonical or ((p["l1"] == (1 << low) - 1).sum() >= 5 and (p["x"] == full).any() and (p["x"] == 0).any())
    assert b.counts[0] >= (4 if canonical else 2) * (200 - k + 1)
    return b


# --------------------------------------------------------------------------------------------------------- e
def _small_shapes(lay, k, sh, rng, canonical):
    """regions of 1, 7, 8, 9, 15, 16, 17 elements and (leaf, sub) segments of 1, 7, 8, 9 -> what to assert"""
    nsub = 1 << sh["b2"]
    want_reg, want_seg = {}, {}
    for i, r in enumerate((1, 7, 8, 9, 15, 16, 17)):
        bin_ = 100 + i
        for j in range(r):
            key = rr.craft_some(k, sh, (bin_ << sh["b2"]) | (j % nsub), 1, rng, canonical, avoid=lay.counts)[0]
            lay.put(key, 1, 9 + 32 * (i % 2))
        want_reg[(bin_, 9)] = r
    for j, c in enumerate((1, 7, 8, 9)):
        leaf = (120 << sh["b2"]) | j
        lay.put(rr.craft_some(k, sh, leaf, 1, rng, canonical, avoid=lay.counts)[0], c, 11)
        want_seg[(leaf, 11)] = c
    return want_reg, want_seg


@functools.lru_cache(maxsize=None)
def case_e_small(k, canonical=False):
    sh = _sh(k)
    lay = rr.Layout(k, canonical)
    reg, seg = _small_shapes(lay, k, sh, _rng(k, 5), canonical)
    b = _done(lay, sh, "short regions and segments under the fixed stride")
    assert all(b.region[x] == n for x, n in reg.items()) and all(b.seg[x] == n for x, n in seg.items())
    assert not rr.predict(b)["relaid1"]
    return b


@functools.lru_cache(maxsize=None)
def case_e_tile(k, big, canonical=False):
    """one region of exactly 8192 elements, every sub-bin present with a count = 1 mod 8: RX2's padded tile at its
    largest.  big: the buffer is long enough (mostly -1) for cap1 >= 8192, so the tile goes through the vector kernel
    under the fixed stride; otherwise level 1 is laid out again and the scalar kernel takes it"""
    sh = _sh(k)
    nsub = 1 << sh["b2"]
    per = {512: [9] * 64 + [17] * 448, 8: [1025] * 7 + [1017]}[nsub]
    assert sum(per) == 8192 and all(c % 8 == 1 for c in per)
    B, S = 37, 5
    rng = _rng(k, big, 7)
    lay = rr.Layout(k, canonical)
    for j, c in enumerate(per):
        k1, k2 = rr.craft_some(k, sh, (B << sh["b2"]) | j, 2, rng, canonical)
        lay.put_sub(k1, 1, S)
        lay.put_sub(k2, c - 1, S)
    reg, seg = _small_shapes(lay, k, sh, rng, canonical)
    b = _done(lay, sh, "a full padded tile", min_tiles=3200 if big else 0)
    assert b.region[(B, S)] == 8192 and all(b.seg[((B << sh["b2"]) | j, S)] == c for j, c in enumerate(per))
    assert sum((c + 7) // 8 * 8 for c in per) == 8192 + 7 * nsub
    assert all(b.region[x] == n for x, n in reg.items()) and all(b.seg[x] == n for x, n in seg.items())
    assert rr.predict(b)["relaid1"] == (not big)
    return b


# --------------------------------------------------------------------------------------------------------- f
@functools.lru_cache(maxsize=None)
def case_f(k, size, one_leaf, canonical=False):
    """all keys in one bin, `size` elements in its largest region: above cap1, level 1 is laid out again (the scalar
    RX2 with 1, 2 or 3 tiles per region); one_leaf: they are all of one leaf, which then overflows cap2 as well"""
    sh = _sh(k)
    B, S = 200, 3
    rng = _rng(k, size, one_leaf)
    nsub = 1 << sh["b2"]
    m = 4 if one_leaf else 64
    keys = [rr.craft_some(k, sh, (B << sh["b2"]) | (0 if one_leaf else j % nsub), 1, rng, canonical, avoid=())[0] for j in range(m)]
    keys = list(dict.fromkeys(keys))
    lay = rr.Layout(k, canonical)
    left = size
    for i, key in enumerate(keys):
        n = left if i == len(keys) - 1 else size // len(keys)
        lay.put_sub(key, n, S)
        left -= n
    for s in (0, 4, 31):
        lay.put_sub(keys[s % len(keys)], 100 + s, s)
    b = _done(lay, sh, "one bin", check_n=False)
    p = rr.predict(b)
    assert max(b.region.values()) == b.region[(B, S)] == size and {x[0] for x in b.region} == {B}
    assert p["relaid1"] and p["relaid2"] == one_leaf and p["attempts"] == (3 if one_leaf else 2)
    return b


# --------------------------------------------------------------------------------------------------------- g
PATTERNS = [(300, 404), (300, 405), (704, 1), (705,), (10, 705, 10), (0, 704, 0, 1)]


@functools.lru_cache(maxsize=None)
def case_g(k, grid, canonical=False):
    """the leaf kernel's result buffer (704 entries): every pattern of distinct-key counts on the successive leaves of a
    workgroup of its own -- as many patterns as the leaves per workgroup allow --, everything else empty but for a
    sprinkling of random reads"""
    sh = _sh(k)
    nleaf = 1 << (sh["b1"] + sh["b2"])
    rng = _rng(k, grid, 9)
    lay = rr.Layout(k, canonical)
    used, wgs, i = {}, {}, 0
    for pi, pat in enumerate(PATTERNS):
        if len(pat) > nleaf // grid:
            continue
        w = 10 + 7 * pi
        wgs[w] = pat
        for j, m in enumerate(pat):
            if m:
                for key in rr.craft_some(k, sh, w + j * grid, m, rng, canonical):
                    lay.put_sub(key, 1 + j % 3, i % 32)
                    i += 1
                used[w + j * grid] = m
    extra = 0
    while extra < 200:
        key = int(rng.integers(0, 1 << (2 * k)))
        leaf = int(rr.place([key], k, sh)["leaf"][0])
        if leaf % grid in wgs or key in lay.counts or (canonical and not rr.canonical_ok(key, k)):
            continue
        lay.put_sub(key, 1, extra % 32)
        extra += 1
    b = _done(lay, sh, "result buffer patterns")
    p = rr.predict(b, grid)
    for w, pat in wgs.items():
        assert tuple(p["entries"].get(l, 0) for l in p["walks"](w))[:len(pat)] == pat
        assert all(p["entries"].get(l, 0) == 0 for l in p["walks"](w)[len(pat):])
    assert len(wgs) >= 4
    b.patterns = wgs
    return b


# --------------------------------------------------------------------------------------------------------- h
@functools.lru_cache(maxsize=None)
def case_h(k, canonical=False):
    """three adds of crafted sets that overlap in some keys -> three Built"""
    sh = _sh(k)
    rng = _rng(k, 11)
    if sh["direct"]:
        keys = [int(x) for x in rng.permutation(1 << (2 * k))[:200] if not canonical or rr.canonical_ok(int(x), k)][:60]
    else:
        keys = []
        for leaf in (1, 2, 700, 701, 2047, 1500):
            keys += rr.craft_some(k, sh, leaf, 10, rng, canonical)
    out = []
    for a, sel in enumerate((keys[0:40], keys[20:60], keys[0:60:2])):
        lay = rr.Layout(k, canonical)
        for i, key in enumerate(sel):
            lay.put(key, 1 + (i * 7 + a) % 13, (i + a) % 4)
        out.append(_done(lay, sh, f"add {a}"))
    return out


# ------------------------------------------------------------------------------------------ the list of sections a-h
def all_cases(grid=GRID):
    """[(id, thunk -> Built or list of Built)]: every crafted buffer, forward-strand, and each letter once as a
    canonical job with canonical-filtered keys.  grid(k): the leaf kernel's grid to build cases c and g for."""
    out = []
    add = lambda name, f, *a: out.append((name, functools.partial(f, *a)))
    for k in (13, 15, 16):
        add(f"a-k{k}", case_a, k)
    add("a-k13-canonical", case_a, 13, True)
    for k in (13, 16):
        for n in (65528, 65536):
            add(f"b-k{k}-n{n}", case_b, k, n)
    add("b-k16-n65528-canonical", case_b, 16, 65528, True)
    add("b-k16-n65536-canonical", case_b, 16, 65536, True)
    for k in (13, 15, 16):
        add(f"c-k{k}", lambda k: case_c(k, grid(k)), k)
    add("c-k15-canonical", lambda: case_c(15, grid(15), True))
    for k in (4, 7, 8, 10, 12, 13, 15, 16):
        add(f"d-k{k}", case_d, k)
        add(f"d-k{k}-canonical", case_d, k, True)
    for k in (8, 12, 13):
        add(f"e-small-k{k}", case_e_small, k)
    add("e-small-k12-canonical", case_e_small, 12, True)
    for k in (10, 16):
        add(f"e-tile-k{k}-relaid", case_e_tile, k, False)
        add(f"e-tile-k{k}-fixed-stride", case_e_tile, k, True)
    add("e-tile-k16-relaid-canonical", case_e_tile, 16, False, True)
    for k in (12, 15, 16):
        for size in (8192, 8193, 16385):
            add(f"f-k{k}-{size}", case_f, k, size, False)
    add("f-k12-16385-one-leaf", case_f, 12, 16385, True)
    add("f-k16-8193-one-leaf-canonical", case_f, 16, 8193, True, True)
    for k in (12, 13):
        add(f"g-k{k}", lambda k: case_g(k, grid(k)), k)
    add("g-k13-canonical", lambda: case_g(13, grid(13), True))
    for k in (7, 12, 15, 16):
        add(f"h-k{k}", case_h, k)
    add("h-k12-canonical", case_h, 12, True)
    return out
