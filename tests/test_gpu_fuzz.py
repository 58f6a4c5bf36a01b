"""Randomised parity of the global paths against the oracle: random k, read lengths (including
reads shorter than k and empty reads), invalid-base densities, homopolymer / tandem-repeat
stretches, one or two adds; and (test_random_seam_ladders_match_oracle) random features of tests/seam_cases.py on random
wave and tile seams, with buffer sizes around the 32-byte chunk and wave-tile edges."""
import numpy as np
import pytest

from . import oracle_lib as orc
from . import msp_ref
from . import refsem
from . import seam_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


def _case(rng):
    k = int(rng.choice([1, 3, 6, 7, 8, 9, 12, 15, 16, 17, 20, 23, 26, 29, 30, 31, 32, 33, 40, 64]))
    nreads = int(rng.integers(1, 400))
    style = rng.integers(0, 4)
    reads = []
    for _ in range(nreads):
        L = int(rng.integers(0, 3 * k + 40)) if style != 3 else int(rng.integers(0, k + 3))
        if style == 1 and rng.random() < 0.3:        # low complexity
            unit = rng.integers(0, 4, int(rng.integers(1, 5))).astype(np.int8)
            r = np.tile(unit, L // len(unit) + 1)[:L]
        else:
            r = rng.integers(0, 4, L).astype(np.int8)
        p_bad = [0.0, 0.01, 0.2][int(rng.integers(0, 3))]
        if p_bad and L:
            r = r.copy()
            r[rng.random(L) < p_bad] = -1
        reads.append(r)
    return k, reads


@pytest.mark.parametrize("seed", range(60))
def test_random_inputs_match_oracle(ctx, seed):
    import cfrk_amd
    rng = np.random.default_rng(1000 + seed)
    k, reads = _case(rng)
    canonical = bool(rng.integers(0, 2))
    data, start, length = refsem.flatten(reads)
    flags = cfrk_amd.CFRK_CANONICAL if canonical else 0
    g = cfrk_amd.GlobalCounter(ctx, k, flags, 0)
    if rng.random() < 0.3 and len(reads) > 1:          # two adds: the second forces the fold path
        h = len(reads) // 2
        d1, s1, l1 = refsem.flatten(reads[:h])
        d2, s2, l2 = refsem.flatten(reads[h:])
        g.add(d1, s1, l1)
        g.add(d2, s2, l2)
    else:
        g.add(data, start, length)
    lo, hi, cnt = g.export()
    wlo, whi, wcnt = orc.global_count(data, k, orc.ORC_CANONICAL if canonical else 0)
    assert len(lo) == len(wlo)
    assert (lo == wlo).all() and (hi == whi).all() and (cnt.astype(np.uint64) == wcnt).all()


@pytest.mark.parametrize("seed", range(24))
def test_random_seam_ladders_match_oracle(ctx, seed):
    """a random k, ~20 features of the seam ladder drawn at random on random seams (a third of them tile seams) of the
    path's own period, the buffer cut at a random size around a chunk, wave or tile edge; one add or two (the second
    buffer: the first one shifted by a random pad, which moves every feature off its seam and the tie tags with it)"""
    import cfrk_amd
    rng = np.random.default_rng(3000 + seed)
    k = int(rng.choice([8, 12, 15, 16, 17, 20, 23, 26, 29, 30, 31, 32, 33, 40, 47, 64]))
    canonical = bool(rng.integers(0, 2))
    period = sc.PERIOD64 if k < 16 else sc.PERIOD1 if k <= 32 else sc.PERIOD2
    W = msp_ref.params(k).W if k >= 16 else 1
    items = sc.items_for(rng, k, W)
    items = [items[i] for i in rng.choice(len(items), 20, replace=False)]
    seams = sorted({int(8 * rng.integers(1, 13)) if rng.random() < 0.33 else int(rng.integers(1, 100)) for _ in items})
    lad = sc.ladder(period, items[:len(seams)], seams=seams)
    unit = int(rng.choice([32, period, 8 * period]))                       # a chunk, wave or tile edge somewhere behind the first feature
    first = (seams[0] * period + 700) // unit + 1
    edge = unit * int(rng.integers(first, max(first, len(lad.data) // unit) + 1))
    data = lad.data[:min(len(lad.data), edge + int(rng.integers(-33, 34)))]
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL if canonical else 0, 0)
    g.add(data)
    whole = data
    if rng.random() < 0.4:
        second = np.concatenate([sc.padding(int(rng.integers(1, 32))), data, sc.padding(1)])
        g.add(second)
        whole = np.concatenate([data, sc.padding(1), second])
    lo, hi, cnt = g.export()
    wlo, whi, wcnt = orc.global_count(whole, k, orc.ORC_CANONICAL if canonical else 0)
    assert len(lo) == len(wlo) and len(lo) > 0
    assert (lo == wlo).all() and (hi == whi).all() and (cnt.astype(np.uint64) == wcnt).all()


@pytest.mark.parametrize("seed", range(40))
def test_random_dense_matches_oracle(ctx, seed):
    """per-read dense path (kmer_main drop-in): random k <= 9, compat and native semantics"""
    import cfrk_amd
    rng = np.random.default_rng(5000 + seed)
    k = int(rng.integers(1, 10))
    nreads = int(rng.integers(1, 120))
    reads = []
    for _ in range(nreads):
        L = int(rng.choice([0, 1, 2, k - 1, k, k + 1, 150, 300, 1024, 1025, 1026, 1500]))
        L = max(L, 0)
        r = rng.integers(0, 4, L).astype(np.int8)
        if L and rng.random() < 0.5:
            r[rng.random(L) < 0.05] = -1
        reads.append(r)
    data, start, length = refsem.flatten(reads)
    for compat in (True, False):
        got = ctx.per_read_dense(data, start, length, k, cfrk_amd.CFRK_COMPAT if compat else 0)
        want = orc.per_read_dense(data, start, length, k, orc.ORC_COMPAT if compat else 0)
        assert (got == want).all()


@pytest.mark.parametrize("k", [16, 21, 27, 31, 32, 40, 63])
@pytest.mark.parametrize("glen", [20_000, 2_000_000])
def test_coverage_sweep_with_invalid_bases(ctx, k, glen):
    """Sequencing-like input at two depths (≈1100x: every leaf's record table sees each run
    hundreds of times; ≈11x: mostly first sightings), 1 % of the bases invalid, both strands:
    full (key, count) equality with the oracle."""
    import cfrk_amd
    R, L = 150_000, 150
    data, _, _ = orc.synth_reads(0, R, L, glen)
    data = data.copy()
    rng = np.random.default_rng(k * 7 + glen)
    bad = rng.random(len(data)) < 0.01
    bad &= data >= 0                              # keep the read terminators where they are
    data[bad] = -1
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, 4 * min(glen, R * L))
    g.add(data)
    if glen == 20_000 and 16 <= k <= 32:
        # ~4000 leaves hold everything, each several times its fixed stride: the second level is
        # laid out again with exact sizes; nothing is counted through the HBM-table spill path
        assert g.msp_info()["spilled_records"] == 0
    lo, hi, cnt = g.export()
    wlo, whi, wcnt = orc.global_count(data, k, orc.ORC_CANONICAL, threads=8 if k <= 32 else 0)
    assert len(lo) == len(wlo)
    assert (lo == wlo).all() and (hi == whi).all() and (cnt.astype(np.uint64) == wcnt).all()
