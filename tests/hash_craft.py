"""Crafting keys that collide: a numpy restatement of the slot hash of the HBM table and the query index (dev_mix64,
cfrk_amd/csrc/common.h), its exact inverse, and helpers that place keys on chosen slots -- TEST INFRASTRUCTURE ONLY.

The hash is two rounds of `x ^= x >> 32; x *= M` with an odd M and a last `x ^= x >> 32`: every step is a bijection of
the 64-bit words (a shift of half the word is its own inverse, an odd multiplier has an inverse mod 2^64), so the key
of any hash value can be computed.  A key's home slot in a structure of 2^n slots is the top n bits of its hash:
  one-word keys (k <= 32):  mix(lo)           two-word keys (k > 32):  mix(lo ^ mix(hi))
The restatement is held against the product's own function (cfrk_debug_hash_info) by tests/test_hash_craft_cpu.py and
again by every test of tests/test_gpu_hash_edges.py on its own keys, so a change of the hash cannot go unnoticed.
"""
import functools

import numpy as np

M = 0xD6E8FEB86659FD93
M_INV = pow(M, -1, 1 << 64)
ALL_ONES = (1 << 64) - 1
ENUM_MAX = 1 << 24                    # small k: at most this many keys are enumerated
_U32 = np.uint64(32)


def _u64(x):
    return np.atleast_1d(np.asarray(x, dtype=np.uint64))


def mix(x):
    """dev_mix64 on an array of words (uint64 arithmetic wraps)"""
    x = _u64(x).copy()
    for mul in (M, M):
        x ^= x >> _U32
        x *= np.uint64(mul)
    x ^= x >> _U32
    return x


def inv_mix(y):
    """the word whose mix() is y"""
    y = _u64(y).copy()
    y ^= y >> _U32
    for mul in (M_INV, M_INV):
        y *= np.uint64(mul)
        y ^= y >> _U32
    return y


def hash1(lo):
    return mix(lo)


def hash2(lo, hi):
    return mix(_u64(lo) ^ mix(hi))


def key_hash(lo, hi, two_word):
    return hash2(lo, hi) if two_word else hash1(lo)


def home(lo, hi, log2_slots, two_word):
    """home slot of every key in a structure of 2^log2_slots slots"""
    return (key_hash(lo, hi, two_word) >> np.uint64(64 - log2_slots)).astype(np.int64)


def revcomp_int(x, k):
    """reverse complement of a k-mer held in a Python int (first base most significant)"""
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (x & 3))
        x >>= 2
    return r


def is_canonical(lo, hi, k):
    lo, hi = _u64(lo), _u64(hi)
    out = np.zeros(len(lo), bool)
    for i, (l, h) in enumerate(zip(lo, hi)):
        x = int(h) << 64 | int(l)
        out[i] = x <= revcomp_int(x, k)
    return out


@functools.lru_cache(maxsize=1)
def _enum_top24():
    """top 24 bits of the hash of every key 0 .. ENUM_MAX - 1"""
    return (mix(np.arange(ENUM_MAX, dtype=np.uint64)) >> np.uint64(40)).astype(np.uint32)


def _targets(slot, log2_slots, n, rng):
    """n hash values whose top bits are `slot`, the free low bits random"""
    shift = 64 - log2_slots
    low = rng.integers(0, 1 << shift, n, dtype=np.uint64)
    return (np.uint64(slot) << np.uint64(shift)) | low


def keys_homing_on(slot, log2_slots, k, n, canonical=False, two_word=False, rng=None):
    """n distinct keys of k bases (< 4^k, never the k = 32 all-ones word) whose home is `slot` of 2^log2_slots
    -> (lo, hi) uint64 arrays.  canonical: only keys that are their own canonical form."""
    rng = rng if rng is not None else np.random.default_rng(0)
    assert 0 <= slot < (1 << log2_slots) and 10 <= log2_slots <= 24
    assert two_word == (k > 32) and 12 <= k <= 64
    zeros = lambda a: np.zeros(len(a), np.uint64)
    if not two_word and k < 28:
        # 4^k / 2^64 of the inverted targets would be keys: enumerate the first keys instead
        m = min(1 << (2 * k), ENUM_MAX)
        lo = np.nonzero((_enum_top24()[:m] >> np.uint32(24 - log2_slots)) == slot)[0].astype(np.uint64)
        if canonical:
            lo = lo[is_canonical(lo, zeros(lo), k)]
        if len(lo) < n:
            raise ValueError(f"only {len(lo)} of the first {m} keys of k={k} home on slot {slot}")
        lo = np.sort(rng.choice(lo, n, replace=False))
        return lo, zeros(lo)
    got_lo, got_hi, seen = [], [], set()
    for _ in range(64):
        want = 8 * n + 64
        t = _targets(slot, log2_slots, want, rng)
        if two_word:
            hbits = 2 * k - 64
            hi = rng.integers(0, 1 << hbits, want, dtype=np.uint64) if hbits < 64 else \
                rng.integers(0, 1 << 63, want, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, want, dtype=np.uint64)
            lo = inv_mix(t) ^ mix(hi)
            keep = np.ones(want, bool)
        else:
            lo, hi = inv_mix(t), np.zeros(want, np.uint64)
            keep = (lo >> np.uint64(2 * k)) == 0 if k < 32 else lo != np.uint64(ALL_ONES)
        lo, hi = lo[keep], hi[keep]
        if canonical:
            c = is_canonical(lo, hi, k)
            lo, hi = lo[c], hi[c]
        for l, h in zip(lo, hi):
            if (int(l), int(h)) not in seen and len(got_lo) < n:
                seen.add((int(l), int(h)))
                got_lo.append(l)
                got_hi.append(h)
        if len(got_lo) == n:
            return np.array(got_lo, np.uint64), np.array(got_hi, np.uint64)
    raise ValueError(f"could not craft {n} keys of k={k} for slot {slot}")


def same_lo_different_hi(slot, log2_slots, k, n, rng=None):
    """n two-word keys with ONE lo and distinct hi, all homing on `slot`: a scan over up to 2^22 values of hi"""
    rng = rng if rng is not None else np.random.default_rng(0)
    assert k > 32
    hbits = 2 * k - 64
    span = min(1 << hbits, 1 << 22)
    base = int(rng.integers(0, (1 << min(hbits, 63)) - span + 1))
    hi = np.arange(base, base + span, dtype=np.uint64)
    lo = rng.integers(0, 1 << 63, 1, dtype=np.uint64)
    hit = hi[home(np.full(span, lo[0], np.uint64), hi, log2_slots, True) == slot]
    if len(hit) < n:
        raise ValueError(f"only {len(hit)} of {span} values of hi land on slot {slot} (k={k})")
    hit = np.sort(rng.choice(hit, n, replace=False))
    return np.full(n, lo[0], np.uint64), hit


def same_hi_different_lo(slot, log2_slots, k, n, rng=None):
    """n two-word keys with ONE hi and distinct lo, all homing on `slot`: lo = inv(target) ^ mix(hi)"""
    rng = rng if rng is not None else np.random.default_rng(0)
    assert k > 32
    hbits = 2 * k - 64
    hi = rng.integers(0, 1 << min(hbits, 63), 1, dtype=np.uint64)
    lo = np.unique(inv_mix(_targets(slot, log2_slots, 2 * n, rng)) ^ mix(hi))
    assert len(lo) >= n
    lo = lo[:n]
    return lo, np.full(n, hi[0], np.uint64)


def occupied_after(homes, log2_slots):
    """Linear probing of keys with the given home slots, inserted in the given order, into 2^log2_slots empty slots
    -> (occupant, displacement): occupant[s] = index of the key in slot s or -1, displacement[i] = slots key i sits
    behind its home.  The SET of occupied slots of linear probing does not depend on the insertion order (a key's
    displacement does), so `occupant >= 0` predicts the device's layout exactly."""
    n = 1 << log2_slots
    homes = np.asarray(homes, np.int64)
    assert len(homes) <= n
    occupant = np.full(n, -1, np.int64)
    disp = np.zeros(len(homes), np.int64)
    for i, h in enumerate(homes):
        s = int(h)
        while occupant[s] >= 0:
            s = (s + 1) & (n - 1)
        occupant[s] = i
        disp[i] = (s - int(h)) & (n - 1)
    return occupant, disp


def forced_displacement(homes, log2_slots):
    """a displacement some key has in EVERY insertion order: the key in the last slot of a cluster (a maximal run of
    occupied slots, possibly through the wrap) homes inside the cluster, so it sits at least (last slot - the
    cluster's largest home) behind its home -> the largest such bound over the clusters"""
    n = 1 << log2_slots
    homes = np.asarray(homes, np.int64)
    occ = occupied_after(homes, log2_slots)[0] >= 0
    if occ.all() or not occ.any():
        return 0
    first_empty = int(np.nonzero(~occ)[0][0])
    best, run_start = 0, None
    rel_homes = (homes - first_empty) & (n - 1)            # positions counted from an empty slot: no run wraps
    rel_occ = np.roll(occ, -first_empty)
    for p in range(1, n + 1):
        if p < n and rel_occ[p]:
            if run_start is None:
                run_start = p
        elif run_start is not None:
            inside = rel_homes[(rel_homes >= run_start) & (rel_homes < p)]
            best = max(best, p - 1 - int(inside.max()))
            run_start = None
    return best


def key_to_read(lo, hi, k):
    """the k bases of the key (int8 codes 0..3), first base most significant"""
    x = int(hi) << 64 | int(lo)
    assert x >> (2 * k) == 0
    return np.array([(x >> (2 * (k - 1 - j))) & 3 for j in range(k)], np.int8)
