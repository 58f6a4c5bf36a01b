"""CPU: tests/radix_ref.py -- the numpy restatement of radix.hip's placement, its key crafter and its buffer builder --
held against the product's host shape function (cfrk_debug_radix_info without a context: pure host arithmetic, no device
needed), against a slow key-by-key walk of the three kernels' bookkeeping, and against the oracle on every crafted buffer
of tests/radix_cases.py.  The GPU tests (tests/test_gpu_radix_shapes.py) rest on what is asserted here."""
import numpy as np
import pytest

from . import oracle_lib as orc
from . import radix_cases as rc
from . import radix_ref as rr
from .hash_craft import revcomp_int

SHAPE_KEYS = ("b1", "b2", "idx", "mul", "inv", "cap1", "cap2", "takes", "direct", "hi8")


@pytest.fixture(scope="module")
def product():
    import cfrk_amd
    return cfrk_amd


def _same_shape(product, k, nN):
    got, want = product.radix_info(k, nN), rr.shape(k, nN)
    assert {x: got[x] for x in SHAPE_KEYS} == {x: want[x] for x in SHAPE_KEYS}, (k, nN)
    assert (got["attempts"], got["relaid1"], got["relaid2"], got["grid"]) == (0, False, False, 0)     # no context


# ------------------------------------------------------------------------------------------------- the scramble
@pytest.mark.parametrize("k", range(8, 17))
def test_unmix_inverts_mix(k):
    full = (1 << (2 * k)) - 1
    x = np.concatenate([np.random.default_rng(k).integers(0, full + 1, 20000, dtype=np.uint64),
                        np.array([0, 1, full], np.uint64)])
    y = rr.mix(x, k)
    assert (y <= np.uint64(full)).all() and (rr.unmix(y, k) == x).all() and (rr.mix(rr.unmix(x, k), k) == x).all()
    assert (rr.MUL * rr.INV) % (1 << 32) == 1 and rr.MUL % 2 == 1


def test_mix_is_a_bijection_at_k8():
    y = rr.mix(np.arange(1 << 16, dtype=np.uint64), 8)
    assert len(np.unique(y)) == 1 << 16 and int(y.max()) == (1 << 16) - 1


# ------------------------------------------------------------------------------------------------- the shape
@pytest.mark.parametrize("k", range(1, 17))
def test_shape_equals_the_products_host_function(product, k):
    for nN in (1, 10 ** 6, 10 ** 8):
        _same_shape(product, k, nN)
    s = rr.shape(k, 10 ** 6)
    if k <= 7:
        assert s["direct"] and s["takes"] and s["idx"] == 0
    else:
        assert s["b1"] + s["b2"] + s["idx"] == 2 * k and s["b1"] + s["b2"] >= 11 and s["hi8"] == (k >= 12)


def _last_true(pred, lo, hi):
    """largest n in [lo, hi) with pred(n), pred monotone (true, then false)"""
    assert pred(lo) and not pred(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if pred(mid) else (lo, mid)
    return lo


@pytest.mark.parametrize("k", [13, 14, 15])
def test_the_idx_14_to_13_threshold_is_the_products(product, k):
    n = _last_true(lambda n: rr.shape(k, n)["idx"] == 14, 1, 1 << 40)
    assert rr.shape(k, n)["idx"] == 14 and rr.shape(k, n + 1)["idx"] == 13
    # the rule in closed form: a mean leaf of 2^14 keys, pads included, times 1.5 reaches 49152 elements
    b2w = 2 * k - 8 - 14
    assert abs(n - 32768.0 * (1 << (8 + b2w)) / (1.0 + 3.5 * (1 << b2w) / 8192.0)) < 2.0
    assert k != 13 or 1.3e8 < n < 1.35e8
    _same_shape(product, k, n)
    _same_shape(product, k, n + 1)
    assert product.radix_info(k, n)["idx"] == 14 and product.radix_info(k, n + 1)["idx"] == 13
    assert product.radix_info(k, n + 1)["b2"] == 2 * k - 8 - 13


def test_the_k16_limit_is_the_products(product):
    n = _last_true(lambda n: rr.shape(16, n)["takes"], 1, 1 << 40)
    assert 3e9 < n < 4e9
    _same_shape(product, 16, n)
    _same_shape(product, 16, n + 1)
    assert product.radix_info(16, n)["takes"] and not product.radix_info(16, n + 1)["takes"]
    assert not product.radix_info(17, 1000)["takes"] and not product.radix_info(0, 1000)["takes"]


# ------------------------------------------------------------------------------------------------- the crafter
@pytest.mark.parametrize("k", [8, 10, 12, 13, 15, 16])
def test_craft_lands_where_it_says(k):
    sh = rr.shape(k, 1 << 20)
    rng = np.random.default_rng(k)
    nleaf, nctr = 1 << (sh["b1"] + sh["b2"]), 1 << sh["idx"]
    for leaf, counter in [(0, 0), (nleaf - 1, nctr - 1), (0, nctr - 1), (nleaf - 1, 0)] + \
                         [(int(rng.integers(nleaf)), int(rng.integers(nctr))) for _ in range(200)]:
        key = rr.craft(k, sh, leaf, counter)
        p = rr.place([key], k, sh)
        assert (int(p["leaf"][0]), int(p["counter"][0])) == (leaf, counter) and int(p["bin"][0]) == leaf >> sh["b2"]
        assert int(p["l1"][0]) == ((leaf << sh["idx"]) | counter) & ((1 << (2 * k - 8)) - 1)
        c = rr.craft(k, sh, leaf, counter, canonical=True)
        assert c == (key if key <= revcomp_int(key, k) else None)
    m = min(20, nctr // 4)
    some = rr.craft_some(k, sh, 77, m, rng, canonical=True, avoid=[rr.craft(k, sh, 77, 0)])
    assert len(set(some)) == m and all(x <= revcomp_int(x, k) for x in some) and rr.craft(k, sh, 77, 0) not in some
    assert (rr.place(some, k, sh)["leaf"] == 77).all()


# ------------------------------------------------------------------------------------------------- the builder
def _walk(b):
    """radix.hip's bookkeeping key by key, in plain Python: RX1 sends the k-mer starting at byte p to region (bin,
    (p // 8192) & 31); RX2 cuts every region into tiles of 8192 elements and appends each tile's segment of a leaf,
    rounded up to eight, to the leaf -> (n per leaf, {key: count}).  Only for buffers whose regions fit one tile (the
    order of a region's elements is the device's own)."""
    k, sh = b.k, b.sh
    data = np.asarray(b.data)
    full = (1 << (2 * k)) - 1
    regions, counts = {}, {}
    run, key, prev = 0, 0, -2
    valid = np.nonzero((data >= 0) & (data <= 3))[0]
    for p, c in zip(valid.tolist(), data[valid].tolist()):
        if p != prev + 1:                                    # an invalid byte lies between: the window starts over
            run = 0
        prev = p
        key = ((key << 2) | c) & full
        run += 1
        if run >= k:
            kk = min(key, revcomp_int(key, k)) if b.canonical else key
            counts[kk] = counts.get(kk, 0) + 1
            x = (kk * rr.MUL) & full
            start = p - k + 1
            regions.setdefault((x >> (2 * k - 8), (start // 8192) & 31), []).append(x)
    n = {}
    for (bin_, sub), xs in regions.items():
        assert len(xs) <= 8192
        seg = {}
        for x in xs:
            seg[x >> sh["idx"]] = seg.get(x >> sh["idx"], 0) + 1
        for leaf, c in seg.items():
            n[leaf] = n.get(leaf, 0) + (c + 7) // 8 * 8
    return n, counts


@pytest.mark.parametrize("name", ["a-k13", "b-k13-n65528", "b-k16-n65536-canonical", "d-k12", "d-k16-canonical",
                                  "e-small-k12", "e-small-k8", "g-k12", "h-k15"])
def test_builder_promises_hold_against_a_key_by_key_walk(name):
    built = dict(rc.all_cases())[name]()
    for b in built if isinstance(built, list) else [built]:
        n, counts = _walk(b)
        assert counts == b.counts and b.n_exact
        assert n == b.leaf_lo == b.leaf_hi
        assert sum(b.region.values()) == sum(b.seg.values()) == sum(counts.values())
        p = rr.place(list(counts), b.k, b.sh)
        ent = {}
        for leaf in p["leaf"].tolist():
            ent[leaf] = ent.get(leaf, 0) + 1
        assert ent == b.entries
        if b.canonical:
            assert all(x <= revcomp_int(x, b.k) for x in counts)


@pytest.mark.parametrize("name", ["a-k13-canonical", "c-k15-canonical", "d-k8-canonical", "d-k16-canonical", "e-small-k12",
                                  "e-tile-k10-fixed-stride", "f-k15-16385", "f-k16-8193-one-leaf-canonical", "g-k13"])
def test_survey_reads_the_builders_placement_from_the_bytes_alone(name):
    """radix_ref.survey (chunked, threaded, windows in log k passes: what case j of the GPU tests predicts its add from)
    against the builder's own recount, with chunks far smaller than the buffer and regions of one, two and three tiles"""
    b = dict(rc.all_cases())[name]()
    for chunk, threads in ((1 << 16, 3), (1 << 22, 1)):
        s = rr.survey(b.data, b.k, b.canonical, chunk=chunk, threads=threads)
        assert s.sh == b.sh and s.region == b.region and s.seg == b.seg and s.n_exact == b.n_exact
        assert s.leaf_lo == b.leaf_lo and s.leaf_hi == b.leaf_hi
        ps, pb = rr.predict(s), rr.predict(b)
        assert (ps["mode"], ps["attempts"], ps["relaid1"], ps["relaid2"]) == (pb["mode"], pb["attempts"], pb["relaid1"], pb["relaid2"])


def test_the_upper_bound_of_n_covers_every_split_of_a_segment():
    """a region of T tiles cuts a segment into at most T pieces, each rounded up to eight on its own: the worst split of n
    elements (brute force over two pieces) stays within the bound leaf_hi is built from, n + 7 min(T, n)"""
    for n in range(1, 40):
        worst = max((a + 7) // 8 * 8 + (n - a + 7) // 8 * 8 for a in range(0, n + 1))
        assert (n + 7) // 8 * 8 <= worst <= n + 7 * min(2, n)


def test_builder_refuses_what_it_cannot_promise():
    k = 12
    sh = rr.shape(k, 1 << 20)
    lay = rr.Layout(k)
    with pytest.raises(AssertionError):
        lay.put(5, 8192 // 13 + 1, 0)                        # more reads than a tile holds
    key = rr.craft(k, sh, 9, 1)
    for _ in range(14):
        lay.put_sub(key, 630, 2)                             # 8820 elements in one region
    with pytest.raises(AssertionError):
        lay.finish()                                         # n would depend on how the device orders the region
    b = lay.finish(check_n=False)
    assert not b.n_exact and b.leaf_lo[9] == 8824 and b.leaf_hi[9] == 8820 + 2 * 7
    assert rr.predict(b)["relaid1"] and rr.predict(b)["mode"] == {9: 0}
    assert rr.leaf_mode(13, rr.shape(13, 1), 65528, 65528) == 2 and rr.leaf_mode(13, rr.shape(13, 1), 65536, 65536) == 3
    with pytest.raises(AssertionError):
        rr.leaf_mode(16, rr.shape(16, 1), 65528, 65536)


def test_predict_walks_and_reads_land_in_their_tiles():
    b = rc.case_g(13, 1024)
    p = rr.predict(b, 1024)
    assert p["walks"](10) == [10, 1034, 2058, 3082] and p["relaid2"] and not p["relaid1"] and p["attempts"] == 2
    starts, _ = rr.kmers_of(b.data, 13, False)
    assert len(starts) == sum(b.counts.values()) and (starts % 8192 + 13 <= 8192).all()
    d = rc.case_d(12)
    assert (d.data[d.data >= 0] <= 3).all() and len(d.data) % 8192 == 0


# ------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("name", [n for n, _ in rc.all_cases()])
def test_every_crafted_buffer_counts_to_its_multiset_in_the_oracle(name):
    built = dict(rc.all_cases())[name]()
    for b in built if isinstance(built, list) else [built]:
        lo, hi, cnt = orc.global_count(b.data, b.k, orc.ORC_CANONICAL if b.canonical else 0,
                                       threads=4 if len(b.data) > (1 << 22) else 0)
        assert len(lo) == len(b.keys_sorted) and (lo == b.keys_sorted).all() and (cnt == b.counts_sorted).all()
        assert not hi.any() and {int(a): int(c) for a, c in zip(lo, cnt)} == b.counts
