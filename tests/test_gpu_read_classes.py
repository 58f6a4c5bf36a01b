"""GPU: one batch through the three calls that give every read to a lane group by its size class -- per-read sparse
rows, read statistics, solid spans -- with the window count chosen PER POSITION of the batch, so that the shared class
dispatch (a 16-lane group per read, a 64-lane wave that ballots 64 lengths at a time) and the shared long-read listing
(blocks of 256 reads, of 1024 in the sparse sort) meet every seam of their index arithmetic together: long reads next
to each other, at a block's first and last index and at index 256, ballot groups with none, one and many reads of the
wave's class, and reads of 0, 1, 16, 255 and 256 windows between them.  The batch has more than 1024 reads (the
sparse listing block must be passed once) but stays at about 0.3 MB: most positions hold short reads.  What the calls
share is the window count per position, which is what the index arithmetic sees: a read's length follows from k, and
the genome and the reads' places in it are drawn anew for every k.
References: _oracle_rows of test_gpu_sparse.py, _ref_stats of test_gpu_read_stats.py, filter_ref.ref_spans; each is
computed once per k and compared exactly."""
import functools

import numpy as np
import pytest

from . import filter_ref as fr
from . import refsem
from .test_gpu_filter import COUNT_MAX, _assert_spans, _device_spans
from .test_gpu_query import _oracle
from .test_gpu_read_stats import _assert_rows, _device_stats, _ref_stats
from .test_gpu_sparse import _check_contract, _device_form, _flags, _oracle_rows, _same

pytestmark = pytest.mark.gpu

NS = 1100
CAP16, CAP64 = 256, 2048                                         # == CFRK_*_FAST_WINDOWS, asserted below
LONG_AT = (0, 1, 255, 256, 257, 511, 512, 1023, 1024, NS - 1)    # blocks of 256: first / last index, neighbours; of 1024 too
ONE_AT = 150                                                     # the only 64-lane read of the ballot group [128, 192)
MANY = tuple(range(192, 255, 3)) + (193, 254)                    # 23 of them in [192, 256), 192 / 193 / 254 included
FILL = (0, -1, 1, 16, 255, 256, None)                            # windows by position modulo 7: -1 = length 0, None = random


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


def _window_counts():
    """window count per position (-1: a read of length 0)"""
    rng = np.random.default_rng(1700)
    nwin = np.array([FILL[i % 7] if FILL[i % 7] is not None else int(rng.integers(17, 255)) for i in range(NS)])
    for j, i in enumerate(MANY):
        nwin[i] = (CAP16 + 1, CAP64, CAP64 - 1)[j] if j < 3 else int(rng.integers(CAP16 + 1, 700))
    nwin[ONE_AT] = 1000
    nwin[[20, 40, 1030, 1090]] = (300, CAP64, CAP16 + 1, 600)    # the class also beside long reads and in the last groups
    for j, i in enumerate(LONG_AT):
        nwin[i] = (CAP64 + 1, 2300)[j] if j < 2 else int(rng.integers(CAP64 + 1, 2301))
    return nwin


def test_the_batch_holds_what_it_was_built_for():
    import cfrk_amd
    assert CAP64 == cfrk_amd.CFRK_SPARSE_FAST_WINDOWS == cfrk_amd.CFRK_STATS_FAST_WINDOWS == cfrk_amd.CFRK_SPANS_FAST_WINDOWS
    w = _window_counts()
    long_, mid = w > CAP64, (w > CAP16) & (w <= CAP64)
    assert NS > 1024 and NS > 2 * 256 and (w[long_] <= 2300).all()
    assert sorted(np.nonzero(long_)[0]) == sorted(LONG_AT)
    assert long_[:256].sum() >= 3 and long_[256:512].sum() >= 3 and long_[:1024].sum() >= 8 and long_[1024:].sum() == 2
    per_group = [int(mid[b:b + 64].sum()) for b in range(0, NS, 64)]
    assert per_group[1] == 0 and per_group[2] == 1 and per_group[3] == len(MANY) >= 20 and per_group[0] >= 1
    assert {CAP16 + 1, CAP64 - 1, CAP64} <= set(w[mid]) and {CAP64 + 1, 2300} <= set(w[long_])
    for v in (-1, 0, 1, 16, 255, 256):
        assert (w == v).sum() > 100, v
    assert not long_[64:255].any() and not mid[64:128].any()     # (the groups with none and one are not helped by a long read)


@functools.lru_cache(maxsize=None)
def _batch(k):
    """-> (counted data, reads of the batch): a 6000-base genome counted once and every other block of 100 bases twice
    (counts 1 and 2 alternate along every longer read); read i is a random stretch of it with the windows its position
    asks for, a few with one base replaced by N"""
    rng = np.random.default_rng(1750 + k)
    genome = rng.integers(0, 4, 6000).astype(np.int8)
    counted = refsem.flatten([genome] + [genome[b:b + 100].copy() for b in range(0, 6000, 200)])[0]
    reads = []
    for i, w in enumerate(_window_counts()):
        L = 0 if w < 0 else int(w) + k - 1
        a = int(rng.integers(0, len(genome) - L + 1))
        r = genome[a:a + L].copy()
        if L and (i % 9 == 4 or i in (1, 256, 192)):
            r[int(rng.integers(0, L))] = -1
        reads.append(r)
    assert sum(len(r) for r in reads) < 400000
    return counted, reads


@functools.lru_cache(maxsize=None)
def _counts(k):
    """the oracle's result of the counted set, and per start position of the batch its count and validity (canonical)"""
    counted, reads = _batch(k)
    want = _oracle(counted, k, True)
    return want, fr.window_counts(refsem.flatten(reads)[0], k, True, want)


def _job(ctx, k):
    import cfrk_amd
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, 0)
    g.add(_batch(k)[0])
    return g


@pytest.mark.parametrize("canonical", [False, True])
def test_sparse_rows(ctx, canonical):
    reads = _batch(21)[1]
    data, start, length = refsem.flatten(reads)
    got = _device_form(ctx, data, start, length, 21, _flags(canonical))
    _check_contract(*got, NS)
    _same(got, _oracle_rows(reads, 21, canonical))


@pytest.mark.parametrize("k", [12, 21, 40])
def test_read_stats(ctx, k):
    data, start, length = refsem.flatten(_batch(k)[1])
    exp = _ref_stats(data, start, length, k, True, _counts(k)[0], 2)
    w = _window_counts()
    assert (exp["windows"] <= np.maximum(w, 0)).all() and (exp["windows"] < np.maximum(w, 0)).any()     # the Ns
    assert (exp["min"] != exp["max"]).sum() > 100
    _assert_rows(_device_stats(ctx, _job(ctx, k), data, start, length, 2), exp, k)


@pytest.mark.parametrize("k", [12, 21, 40])
def test_read_spans(ctx, k):
    import cfrk_amd
    data, start, length = refsem.flatten(_batch(k)[1])
    counts, valid = _counts(k)[1]
    g = _job(ctx, k)
    for mode in (cfrk_amd.CFRK_SPAN_LONGEST, cfrk_amd.CFRK_SPAN_PREFIX):
        exp = fr.ref_spans(data, start, length, k, 2, COUNT_MAX, mode, counts, valid)
        assert ((exp["length"] > 0) & (exp["length"] < length)).sum() > 50 and (exp["length"] == 0).sum() > 50
        _assert_spans(_device_spans(ctx, g, data, start, length, 2, COUNT_MAX, mode), exp, (k, mode))
