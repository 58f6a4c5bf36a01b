"""The partition front ends (msp.hip: msp_p1b_kernel, msp2.hip: msp2_p1_kernel) and the 64-lane loaders against a plain
reference at every seam.

Both partition kernels cut the flat buffer into 32-byte lane chunks with halo lanes -- 61 owner lanes per wave for one-word
keys (a wave seam every 1952 bytes), 60 for two-word keys (1920) -- and everything a record is made of crosses those seams
by shuffle: the next lanes' bases, the invalid-base smear, the next lane's first hashes and change bits, the previous
lane's last validity bit.  tests/seam_cases.py puts every feature that can go wrong there -- a read's first base, its
terminator, one invalid code (every invalid byte value takes its turn) inside a long read, tandem repeats, reads of k - 1, k
and k + W - 1 bases, the buffer's end and its start -- at every offset of its range from a wave seam; consecutive seams,
so every eighth feature sits on a tile seam, and a reduced set on tile seams only, which under CFRK_DEBUG_SMALL_PIPELINE
are the pipeline's chunk seams.

Expected values never come from the partitioned path: counts are tests/oracle_lib.global_count entry for entry and the
digest of a CFRK_FORCE_HASH job; record counts and the records themselves are tests/msp_ref.py, the partition rule in
plain numpy (checked on the CPU in tests/test_msp_ref_cpu.py), ties included.
"""
import functools

import numpy as np
import pytest

from . import msp_ref
from . import oracle_lib as orc
from . import seam_cases as sc

pytestmark = pytest.mark.gpu

ONE_WORD = list(range(16, 33))
TWO_WORD = [33, 34, 36, 38, 40, 42, 44]                  # one k per instantiated W2 = 18, 20 .. 30
SMALLER = [17, 21, 27, 31, 32, 33, 44, 63]


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


def period_of(k):
    return sc.PERIOD2 if k > 32 else sc.PERIOD1


MIN_STRIDE = 96            # msp_count_tiles of msp.hip and msp2.hip: cap2c, cap2t = (a share of the expected records) + 96
MIN_REGION = 2048          # ... and cap1, cap1c = (a share) + 2048 records per level-1 sub-region


def stream_loads(data, k):
    """from the reference: (records in the fullest leaf stream, records beyond 128 per stream summed over the streams,
    records in the fullest level-1 sub-region: bin = leaf >> 8, and a tile appends to sub-region tile % 8 of its bins or,
    with more cursors, to a finer split of the same).  A stream is (leaf, class): complete / truncated runs for one-word keys (msp.hip:
    sub_of), complete / truncated of n <= 4, <= 10, > 10 k-mers for two-word keys (msp2.hip: cls_of)."""
    rr = msp_ref.runs(data, k)
    complete = rr.left & rr.right
    cls = np.where(complete, 3, 0) if k <= 32 else np.where(complete, 3, np.where(rr.n <= 4, 0, np.where(rr.n <= 10, 1, 2)))
    load = np.bincount(rr.leaf * 4 + cls, minlength=4 << 16)
    tile = (rr.first + msp_ref.params(k).c) // (sc.WAVES_PER_TILE * period_of(k))      # (the lane that owns the run's first window)
    bins = np.bincount((rr.leaf >> 8) * 8 + tile % 8, minlength=2048)
    return int(load.max()), int(np.maximum(load - 128, 0).sum()), int(bins.max())


CHUNKED_MIN_STRIDE = 256   # msp2_count_tiles, chunked: streams sized from the first chunk, cap2c = .. + 512, cap2t = .. + 256


def fits_two_word_chunks(data, k):
    """The two-word chunked pipeline lays nothing out again: a leaf stream that overflows by more than the parking buffer
    sends the add back to the one-chunk path (CFRK_ERR_SMALL_BUF inside the library, invisible outside), one that overflows
    by less is parked.  Only a buffer whose every stream stays within the smallest chunked stride is certain to END on the
    chunked path with nothing parked."""
    fullest, _, fullest_region = stream_loads(data, k)
    return fullest_region < MIN_REGION and fullest <= CHUNKED_MIN_STRIDE


def never_parks(data, k):
    """Can this buffer be counted with spilled_records == 0 whatever the order of the device's atomics?  Decided from the
    reference and the sizing rule of msp_count_tiles alone, never from a run:
      * no level-1 sub-region holds MIN_REGION records, so none overflows or parks (this also rules out the
        chunked pipeline's quiet restart on the one-chunk path, which needs a level-1 overflow or a parked level-1 record);
      * and either no leaf stream holds more than MIN_STRIDE records -- nothing overflows --, or the streams overflow by far
        more than the parking buffer takes (expected records / 256, with at most len * (2 / (W + 1) + 1 / 64) expected
        records): then the level is laid out again with exact sizes and nothing is parked either.
    A buffer in between -- a stream a little over its stride -- would have its surplus parked and counted through the HBM
    table; ladders_of() admits none."""
    W = msp_ref.params(k).W
    fullest, surplus, fullest_region = stream_loads(data, k)
    parked_max = (len(data) + 32) * (2.0 / (W + 1) + 1.0 / 64.0) / 256.0
    return fullest_region < MIN_REGION and (fullest <= MIN_STRIDE or surplus > 2 * parked_max)


@functools.lru_cache(maxsize=None)
def ladders_of(k, period=None):
    """the ladders of k: every feature at every delta on consecutive wave seams (the first seam moves with k, so over the
    k every feature meets a tile seam), each buffer at least six tiles long, and the reduced set on the tile seams"""
    period = period or period_of(k)
    W = msp_ref.params(k).W if k >= 16 else 1
    rng = np.random.default_rng(9000 + k)
    items = sc.items_for(rng, k, W)
    if period != sc.PERIOD64:
        # the tandem repeats first: all 128 in ONE ladder, whose homopolymers then flood a leaf stream for certain, and none in
        # the others (never_parks: no ladder with a stream only a little over its stride)
        items = [it for it in items if it[0].kind.startswith("tandem")] + [it for it in items if not it[0].kind.startswith("tandem")]
    lads = sc.ladders(period, items, first_seam=1 + k % 8, min_len=6 * sc.WAVES_PER_TILE * period + 1)
    if period == sc.PERIOD64:                              # (the plain loaders: wave seams only)
        return [lad.data for lad in lads]
    tile = sc.tile_ladder(period, sc.tile_items_for(rng, k, W))
    ntiles = sc.tiles_of(len(tile.data), period, k > 32)
    chunk_tiles = sc.pipeline_chunk_tiles(ntiles)
    assert len(chunk_tiles) >= 2 and {8 * t for t in chunk_tiles} <= {p.seam for p in tile.placed}   # features on every chunk seam
    for lad in lads:
        assert any(p.seam % 8 == 0 for p in lad.placed) and sc.tiles_of(len(lad.data), period, k > 32) >= 6
    for lad in lads + [tile]:
        assert never_parks(lad.data, k)                # (so that every add below can be held to spilled_records == 0)
    return [lad.data for lad in lads] + [tile.data]


@functools.lru_cache(maxsize=64)
def oracle(k, i, canonical, period=None):
    want = orc.global_count(ladders_of(k, period)[i], k, orc.ORC_CANONICAL if canonical else 0)
    return want, orc.digest(*want, two_word=k > 32)


_hash_digest = {}


def hash_digest(ctx, data, key, k, canonical):
    """digest of the CFRK_FORCE_HASH job on the same bytes (one job per input, kept)"""
    import cfrk_amd
    if key not in _hash_digest:
        g = cfrk_amd.GlobalCounter(ctx, k, (cfrk_amd.CFRK_CANONICAL if canonical else 0) | cfrk_amd.CFRK_FORCE_HASH, 0)
        g.add(data)
        _hash_digest[key] = g.digest()
    return _hash_digest[key]


def add_with(ctx, data, k, flags, dbg=0, hint=0):
    import cfrk_amd
    if k == 16:
        dbg |= cfrk_amd.lib.CFRK_DEBUG_NO_RADIX16          # (k = 16 and a small batch would go to the radix path)
    g = cfrk_amd.GlobalCounter(ctx, k, flags, hint)
    g.set_debug_flags(dbg)
    try:
        g.add(data)
    finally:
        g.set_debug_flags(0)
    return g


def same_counts(g, want, digest):
    assert g.digest() == digest
    lo, hi, cnt = g.export()
    wlo, whi, wcnt = want
    assert len(lo) == len(wlo)
    assert (lo == wlo).all() and (hi == whi).all() and (cnt.astype(np.uint64) == wcnt).all()


def check_ladders(ctx, k, canonical, dbg=0, hint=0, records=False, only=None):
    import cfrk_amd
    flags = cfrk_amd.CFRK_CANONICAL if canonical else 0
    for i, data in enumerate(ladders_of(k)):
        if only is not None and i not in only:
            continue
        want, digest = oracle(k, i, canonical)
        assert hash_digest(ctx, data, (k, i, canonical), k, canonical) == digest
        g = add_with(ctx, data, k, flags, dbg, hint)
        info = g.msp_info()
        same_counts(g, want, digest)
        assert info["spilled_records"] == 0                # (every ladder: never_parks)
        if records and k <= 32:
            n = len(msp_ref.runs(data, k))
            assert info["l1_records"] == n and info["l2_records"] == n
        elif records:
            # cfrk_debug_msp_info (msp.hip) reads the one-word path's MspView; "the two-word path keeps no view of its
            # record levels", so both fields stay 0 there.  The two-word record count is held to the reference through
            # the packed header triples in test_records_of_the_ladders_and_of_reads_at_two_pads.
            assert info["l1_records"] == 0 and info["l2_records"] == 0


# ---------------------------------------------------------------------------- counts and record counts

@pytest.mark.parametrize("canonical", [True, False], ids=["canonical", "forward"])
@pytest.mark.parametrize("k", ONE_WORD + TWO_WORD)
def test_ladders_match_the_oracle_and_the_reference_run_count(ctx, k, canonical):
    """every ladder, plain add: export() entry for entry, digest() of the hash path, and as many level-1 and level-2
    records as the reference has runs (ties modelled: exact)"""
    check_ladders(ctx, k, canonical, records=True)


@pytest.mark.parametrize("mode", ["small_wave_cap", "no_pipeline", "small_pipeline", "shared_leaves"])
@pytest.mark.parametrize("k", SMALLER)
def test_ladders_on_the_other_paths(ctx, k, mode):
    """CFRK_DEBUG_SMALL_WAVE_CAP (direct append beyond 64 runs per wave), CFRK_DEBUG_NO_PIPELINE, CFRK_DEBUG_SMALL_PIPELINE
    (every ladder is >= 6 tiles: cut into chunks of tiles, the tile ladder with a feature on every chunk seam), and a
    capacity hint above 2.7e8 (the SUB instantiations, which also stage the sub-value bits).
    No status says whether an add finished on the chunked path: msp_count_tiles keeps that in a local and restarts on the
    one-chunk path only after a level-1 region overflowed or parked a record.  never_parks() rules that out for every
    ladder from the reference (no level-1 sub-region reaches the 2048 records it holds at least), and
    CFRK_DEBUG_SMALL_PIPELINE cuts any batch of >= 6 tiles -- asserted in ladders_of() -- so the chunked path is the one that
    ends these adds; with one-word keys a leaf stream that overflows (the tandem ladder) is laid out again and the CHUNKS run
    again; with two-word keys that ladder is taken off the list (below)."""
    import cfrk_amd
    dbg = {"small_wave_cap": cfrk_amd.lib.CFRK_DEBUG_SMALL_WAVE_CAP, "no_pipeline": cfrk_amd.lib.CFRK_DEBUG_NO_PIPELINE,
           "small_pipeline": cfrk_amd.lib.CFRK_DEBUG_SMALL_PIPELINE}.get(mode, 0)
    only = None
    if mode == "small_pipeline" and k > 32:
        # Removed from this mode's list: ladder 0 of the two-word k, the one with the 128 tandem repeats.  Its homopolymers
        # put 450 - 1300 records into one leaf stream, and the two-word chunked pipeline, unlike the one-word one, does not
        # lay an overflowing stream out again (fits_two_word_chunks): the add would restart on the one-chunk path unseen, or
        # park ~60 records at k = 63, and either way not test what this mode is for.  The tandem repeats stay under the
        # chunks in the tile ladder, on the chunk seams themselves.
        only = [i for i, data in enumerate(ladders_of(k)) if fits_two_word_chunks(data, k)]
        assert only == list(range(1, len(ladders_of(k))))
    for canonical in (True, False):
        check_ladders(ctx, k, canonical, dbg=dbg, hint=300_000_000 if mode == "shared_leaves" else 0, only=only)


def check_small(ctx, data, k, canonical=True):
    import cfrk_amd
    want = orc.global_count(data, k, orc.ORC_CANONICAL if canonical else 0)
    g = add_with(ctx, data, k, cfrk_amd.CFRK_CANONICAL if canonical else 0)
    same_counts(g, want, orc.digest(*want, two_word=k > 32))
    info = g.msp_info()
    assert info["spilled_records"] == 0                    # (a few hundred bytes to a few tiles of one read: nothing near a stride)
    if k <= 32:                                            # (the two-word path fills neither field: check_ladders)
        n = len(msp_ref.runs(data, k))
        assert info["l1_records"] == n and info["l2_records"] == n


@pytest.mark.parametrize("k", ONE_WORD + TWO_WORD + [63])
def test_the_buffers_end_around_a_seam(ctx, k):
    """nN = seam - 33 .. seam + 33 (every residue mod 32: the byte-wise tail chunk, `off < nN`, msp2.hip's `off < nN + 32`),
    a read running into the end with and without a terminator, at a wave seam; the smaller set of k also at a tile seam"""
    p = msp_ref.params(k)
    rng = np.random.default_rng(9100 + k)
    period = period_of(k)
    cases = sc.end_buffers(rng, period, k, p.W, seam=1 + k % 3)
    if k in SMALLER:
        cases += sc.end_buffers(rng, period, k, p.W, seam=8, deltas=(-33, -32, -1, 0, 1, 31, 32, 33))
    for e, terminated, data in cases:
        check_small(ctx, data, k, canonical=(e + terminated) % 2 == 0)


@pytest.mark.parametrize("k", ONE_WORD + TWO_WORD + [63])
def test_the_very_first_wave(ctx, k):
    """lane 0 of the first wave loads chunk -1: a read's first base, its terminator and an invalid code at offsets 0..40"""
    p = msp_ref.params(k)
    for kind, o, data in sc.head_buffers(np.random.default_rng(9200 + k), k, p.W):
        check_small(ctx, data, k, canonical=o % 2 == 0)


# ---------------------------------------------------------------------------- the records themselves

def export_decoded(ctx, data, k, canonical=True):
    """CFRK_RUNS_ONLY add under CFRK_DEBUG_NO_ANCHORS (no notes: every truncated run travels as a record), the one-shot
    export with one part, decoded -> ({leaf: (complete, truncated)}, header triples)"""
    import cfrk_amd
    g = cfrk_amd.GlobalCounter(ctx, k, (cfrk_amd.CFRK_CANONICAL if canonical else 0) | cfrk_amd.CFRK_RUNS_ONLY, 0)
    cap = 1 << 18
    d = ctx.alloc(cap * 16)
    g.set_debug_flags(cfrk_amd.lib.CFRK_DEBUG_NO_ANCHORS)
    try:
        g.add(data)
        rows = g.export_runs_device(d, cap, 1)
        host = np.empty((rows[0], 4), np.uint32)
        ctx.d2h(host, d)
    finally:
        g.set_debug_flags(0)
        ctx.free(d)
    return msp_ref.decode_packed(host, k)


def same_records(got, hdr, rr):
    want = msp_ref.by_leaf(rr)
    assert int(hdr[:, 0].max()) < 1024                              # every leaf below the 1024-slot record table
    assert int(hdr[:, 2].sum()) == 0                                # CFRK_DEBUG_NO_ANCHORS: no notes
    assert int(hdr[:, 0].sum()) == sum(len(c) for c, _ in want.values())
    assert int(hdr[:, 1].sum()) == sum(sum(t.values()) for _, t in want.values())
    assert sorted(got) == sorted(want)
    for leaf in want:
        assert got[leaf][0] == want[leaf][0], "complete runs of leaf %d" % leaf
        assert got[leaf][1] == want[leaf][1], "truncated runs of leaf %d" % leaf


@pytest.mark.parametrize("k", [17, 21, 31, 32, 33, 63])
def test_records_of_the_ladders_and_of_reads_at_two_pads(ctx, k):
    """per leaf, the multiset of (bases, n, multiplicity) of the complete runs and of (bases, n, flags) of the truncated
    runs is the reference's: on every ladder (ties in the tandem repeats: modelled), and on
    tie-free reads of a small genome at two pads, where the two decoded multisets must also be the same"""
    from .test_msp_ref_cpu import tie_free_draw, with_pad
    for data in ladders_of(k):                     # (in every ladder the reference's fullest leaf holds < 500 distinct runs)
        got, hdr = export_decoded(ctx, data, k)
        same_records(got, hdr, msp_ref.runs(data, k))

    def draw(rng):
        genome = sc.bases(rng, 3000)
        parts = []
        for _ in range(150):
            a = int(rng.integers(0, len(genome) - 150))
            parts += [genome[a:a + 150], [-1]]
        return np.concatenate(parts).astype(np.int8)
    reads = tie_free_draw(9300 + k, k, draw)
    decoded = []
    for pad in (0, 13):
        data = with_pad(pad, reads)
        got, hdr = export_decoded(ctx, data, k)
        same_records(got, hdr, msp_ref.runs(data, k))
        assert max(max(c.values(), default=0) for c, _ in got.values()) > 1      # (multiplicities are in play)
        decoded.append(got)
    assert decoded[0] == decoded[1]


# ---------------------------------------------------------------------------- the 64-lane loaders

def ladders64(k):
    return ladders_of(k, sc.PERIOD64)


@pytest.mark.parametrize("k", [8, 15, 31, 32, 33, 64])
def test_hash_path_on_the_2048_byte_ladders(ctx, k):
    """CFRK_FORCE_HASH adds (global_hash.hip: dev_load_chunk32 and its own lane-63 reload), both strands"""
    import cfrk_amd
    for canonical in (True, False):
        for i, data in enumerate(ladders64(k)):
            want, digest = oracle(k, i, canonical, sc.PERIOD64)
            g = cfrk_amd.GlobalCounter(ctx, k, (cfrk_amd.CFRK_CANONICAL if canonical else 0) | cfrk_amd.CFRK_FORCE_HASH, 0)
            g.add(data)
            same_counts(g, want, digest)


@pytest.mark.parametrize("k", [9, 13, 15, 16])
def test_radix_path_on_the_2048_byte_ladders(ctx, k):
    """the radix path (radix.hip: rx_load_chunk16): k <= 15, and k = 16 with a small batch"""
    import cfrk_amd
    for canonical in (True, False):
        for i, data in enumerate(ladders64(k)):
            want, digest = oracle(k, i, canonical, sc.PERIOD64)
            g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL if canonical else 0, 0)
            g.add(data)
            same_counts(g, want, digest)


@pytest.mark.parametrize("k", [15, 31, 33, 64])
def test_query_reads_on_the_2048_byte_ladders(ctx, k):
    import cfrk_amd
    from .test_gpu_query import _want_reads
    for i, data in enumerate(ladders64(k)):
        want, _ = oracle(k, i, True, sc.PERIOD64)
        g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, 0)
        g.add(data)
        got = g.query_reads(data)
        exp = _want_reads(data, k, True, want)
        bad = np.flatnonzero(got != exp)
        assert len(bad) == 0, (k, i, bad[:10], got[bad[:10]], exp[bad[:10]])


@pytest.mark.parametrize("k", [8, 31, 32, 33, 64])
def test_sketch_registers_on_the_2048_byte_ladders(ctx, k):
    import cfrk_amd
    from . import sketch_ref as sr
    from .test_gpu_sketch import _same
    for flags in (0, cfrk_amd.CFRK_CANONICAL):
        for data in ladders64(k):
            _same(ctx.distinct_sketch(data, k, flags), sr.sketch_of_reads(data, k, flags))
