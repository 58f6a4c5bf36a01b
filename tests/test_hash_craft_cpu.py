"""CPU: the key-crafting helpers of tests/hash_craft.py -- the numpy slot hash against the product's own (the host
evaluation of cfrk_debug_hash_info: the function the kernels call, no device needed), its inverse, every helper's
promise (home slot, range, canonical form), the probing simulation against a brute-force one, and key_to_read against
the oracle.  tests/test_gpu_hash_edges.py builds its adversarial key sets from these."""
import numpy as np
import pytest

from . import hash_craft as hc
from . import oracle_lib as orc


def _rng(seed):
    return np.random.default_rng(seed)


def test_inverse_round_trip():
    x = _rng(1).integers(0, 1 << 63, 100000, dtype=np.uint64) * np.uint64(2) + _rng(2).integers(0, 2, 100000, dtype=np.uint64)
    x[:4] = [0, 1, hc.ALL_ONES, 1 << 63]
    assert (hc.inv_mix(hc.mix(x)) == x).all()
    assert (hc.mix(hc.inv_mix(x)) == x).all()
    assert len(np.unique(hc.mix(x))) == len(np.unique(x))


def test_python_hash_equals_the_products_host_hash():
    import cfrk_amd
    rng = _rng(3)
    lo = rng.integers(0, 1 << 63, 10000, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 10000, dtype=np.uint64)
    hi = rng.integers(0, 1 << 63, 10000, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 10000, dtype=np.uint64)
    lo[:3], hi[:3] = [0, hc.ALL_ONES, 1], [0, hc.ALL_ONES, 0]
    h1, h2 = hc.hash1(lo), hc.hash2(lo, hi)
    for i in range(len(lo)):
        t, q, p1, p2 = cfrk_amd.hash_info(int(lo[i]), int(hi[i]))
        assert (t, q) == (0, 0)                                   # no context: no geometry
        assert (p1, p2) == (int(h1[i]), int(h2[i])), (i, int(lo[i]), int(hi[i]))


@pytest.mark.parametrize("k,canonical", [(13, False), (13, True), (21, False), (31, False), (31, True), (32, False),
                                         (33, False), (47, False), (47, True), (64, False), (64, True)])
@pytest.mark.parametrize("log2_slots,slot", [(10, 1023), (10, 0), (11, 1300)])
def test_keys_homing_on(k, canonical, log2_slots, slot):
    two = k > 32
    lo, hi = hc.keys_homing_on(slot, log2_slots, k, 70, canonical=canonical, two_word=two, rng=_rng(k))
    assert lo.dtype == np.uint64 and hi.dtype == np.uint64 and len(lo) == len(hi) == 70
    assert (hc.home(lo, hi, log2_slots, two) == slot).all()
    keys = [int(h) << 64 | int(l) for l, h in zip(lo, hi)]
    assert len(set(keys)) == 70
    assert all(x < 4 ** k for x in keys)
    if not two:
        assert (hi == 0).all() and hc.ALL_ONES not in keys
    if canonical:
        assert all(x <= hc.revcomp_int(x, k) for x in keys)
    elif k >= 28:                                                # (small k: the enumerated keys begin with A's)
        assert any(x > hc.revcomp_int(x, k) for x in keys)       # the unfiltered keys are not canonical by accident


@pytest.mark.parametrize("k", [40, 47, 64])
def test_one_word_shared(k):
    lo, hi = hc.same_lo_different_hi(77, 10, k, 64, _rng(k))
    assert len(set(lo.tolist())) == 1 and len(set(hi.tolist())) == 64
    assert (hc.home(lo, hi, 10, True) == 77).all()
    assert all(int(h) < 4 ** (k - 32) for h in hi)
    lo, hi = hc.same_hi_different_lo(77, 10, k, 64, _rng(k + 1))
    assert len(set(hi.tolist())) == 1 and len(set(lo.tolist())) == 64
    assert (hc.home(lo, hi, 10, True) == 77).all()
    assert int(hi[0]) < 4 ** (k - 32)


def test_too_few_keys_is_an_error():
    with pytest.raises(ValueError):
        hc.same_lo_different_hi(1, 10, 33, 64, _rng(0))           # hi < 4: no 64 values
    with pytest.raises(ValueError):
        hc.keys_homing_on(3, 10, 12, 100000, rng=_rng(0))


def _brute(homes, log2_slots):
    """linear probing with a plain list, one step at a time"""
    n = 1 << log2_slots
    table = [None] * n
    disp = []
    for i, h in enumerate(homes):
        d = 0
        while table[(h + d) % n] is not None:
            d += 1
        table[(h + d) % n] = i
        disp.append(d)
    return table, disp


@pytest.mark.parametrize("seed", range(6))
def test_occupied_after_vs_brute_force(seed):
    rng = _rng(seed)
    log2_slots = 10
    n = 1 << log2_slots
    # a few hot homes near the end (the chain wraps) plus scattered ones
    homes = np.concatenate([rng.integers(n - 6, n, 40 * seed), rng.integers(0, n, 100), [n - 1, n - 1, 0]])
    homes = rng.permutation(homes)
    occ, disp = hc.occupied_after(homes, log2_slots)
    table, bdisp = _brute([int(h) for h in homes], log2_slots)
    assert [(-1 if t is None else t) for t in table] == occ.tolist()
    assert bdisp == disp.tolist()
    # the occupied SET is the same in every insertion order; the forced displacement holds in each of them
    forced = hc.forced_displacement(homes, log2_slots)
    for _ in range(5):
        p = rng.permutation(len(homes))
        occ2, disp2 = hc.occupied_after(homes[p], log2_slots)
        assert ((occ2 >= 0) == (occ >= 0)).all()
        assert disp2.max() >= forced
        assert disp2.sum() == disp.sum()
    if seed:
        assert occ[0] >= 0                                        # (the hot chain went through the wrap)


def test_forced_displacement_of_a_wrapping_cluster():
    homes = np.concatenate([np.full(50, s) for s in range(1016, 1024)])
    occ, disp = hc.occupied_after(homes, 10)
    assert set(np.nonzero(occ >= 0)[0].tolist()) == set(range(1016, 1024)) | set(range(0, 392))
    assert hc.forced_displacement(homes, 10) == 392              # slot 391 holds a key homing on 1023 at the latest
    assert hc.forced_displacement(np.arange(100), 10) == 0


@pytest.mark.parametrize("k", [13, 31, 32, 33, 47, 64])
def test_key_to_read_vs_oracle(k):
    two = k > 32
    lo, hi = hc.keys_homing_on(5, 10, k, 20, two_word=two, rng=_rng(k))
    for l, h in zip(lo, hi):
        r = hc.key_to_read(l, h, k)
        assert r.dtype == np.int8 and len(r) == k and ((r >= 0) & (r <= 3)).all()
        wlo, whi, wcnt = orc.global_count(np.concatenate([r, np.array([-1], np.int8)]), k, 0)
        assert (wlo.tolist(), whi.tolist(), wcnt.tolist()) == ([int(l)], [int(h)], [1])
    if k == 32:
        wlo, _, _ = orc.global_count(np.concatenate([hc.key_to_read(hc.ALL_ONES, 0, 32), np.array([-1], np.int8)]), 32, 0)
        assert wlo.tolist() == [hc.ALL_ONES]
