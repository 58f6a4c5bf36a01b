"""The plain reference of the partition rule (tests/msp_ref.py) and the seam ladder (tests/seam_cases.py) against what
does not depend on either: the oracle's counts, the partition property, the record sizes, the host model of
tests/test_gpu_leaf_twins.py, and a round trip through the packed runs form.  Every property runs with 0..31 invalid
bytes in front of the buffer: the tie rule looks at an m-mer's offset mod 32.

k: every one-word k (each has its own window, m-mer or both) and, for two-word keys, one k per instantiated window
(18 .. 30), both parities of m, and the larger margins c of k = 45, 63, 64.
"""
import collections

import numpy as np
import pytest

from . import msp_ref
from . import oracle_lib as orc
from . import seam_cases as sc

KS = list(range(16, 33)) + [33, 34, 35, 36, 38, 40, 42, 44, 45, 63, 64]


def with_pad(pad, data):
    return np.concatenate([sc.padding(pad, phase=pad), np.asarray(data, np.int8)])


def random_reads(rng, k, n=12, p_bad=0.01):
    parts = []
    for _ in range(n):
        r = sc.bases(rng, int(rng.integers(0, 3 * k + 60)))
        r[rng.random(len(r)) < p_bad] = sc.INVALID[int(rng.integers(0, len(sc.INVALID)))]
        parts += [r, sc.INVALID[rng.integers(0, len(sc.INVALID), int(rng.integers(1, 3)))]]
    return np.concatenate(parts)


def same_as_oracle(rr, canonical):
    lo, hi, cnt = msp_ref.expand(rr, canonical)
    wlo, whi, wcnt = orc.global_count(rr.data, rr.k, orc.ORC_CANONICAL if canonical else 0)
    assert len(lo) == len(wlo)
    assert (lo == wlo).all() and (hi == whi).all() and (cnt == wcnt).all()


def test_parameters_restate_the_host_code():
    from .test_gpu_leaf_scan import mmer_len, mmer_len2
    for k in range(16, 65):
        p = msp_ref.params(k)
        assert p.m == (mmer_len(k) if k <= 32 else mmer_len2(k))
        assert p.W + 2 * p.c == k - p.m + 1 and p.W < 32 and p.W + k - 1 <= p.max_bases
    assert [msp_ref.params(k).W for k in (16, 17, 26, 27, 30, 31, 32)] == [5, 6, 15, 15, 18, 18, 17]
    assert sorted({msp_ref.params(k).W for k in range(33, 65)}) == [18, 20, 22, 24, 26, 28, 30]
    assert [msp_ref.params(k).c for k in (33, 43, 44, 45, 63, 64)] == [1, 1, 1, 1, 10, 11]


@pytest.mark.parametrize("k", KS)
def test_runs_partition_the_valid_kmers_and_expand_to_the_oracles_counts(k):
    """at every pad, on a ladder of a 32nd of the seam features and on random reads with invalid codes (a reduction: every
    ladder feature is seen at ONE pad, the random reads at every pad -- the reference has no seams, only the offset mod 32): every valid k-mer lies in exactly one run, a run holds at most W k-mers and fits its record, and the
    runs' k-mers, counted, are the oracle's result on both strands"""
    p = msp_ref.params(k)
    rng = np.random.default_rng(100 + k)
    period = sc.PERIOD2 if p.two else sc.PERIOD1
    items = sc.items_for(rng, k, p.W)
    for pad in range(32):
        lad = sc.ladder(period, items[pad::32])
        data = with_pad(pad, np.concatenate([lad.data, random_reads(rng, k)]))
        rr = msp_ref.runs(data, k)
        assert len(rr) > 100
        assert (msp_ref.covered_positions(rr) == msp_ref.valid_kmers(data, k)).all()
        assert rr.n.min() >= 1 and rr.n.max() <= p.W
        assert (rr.n + k - 1).max() <= p.max_bases
        assert ((rr.occ >= rr.first + p.c) & (rr.occ <= rr.first + p.c + p.W - 1)).all()
        for canonical in (True, False):
            same_as_oracle(rr, canonical)


def hashes25(data, m):
    """(hash without its low seven bits, m-mer is all bases) per offset"""
    h = msp_ref.ordering_values(data, m) >> np.uint64(7)
    return h, msp_ref.valid_kmers(data, m)


def tie_free(data, k):
    """no two m-mers that one window (or two neighbouring windows) can hold agree in their 25 hash bits"""
    p = msp_ref.params(k)
    h, ok = hashes25(data, p.m)
    for d in range(1, p.W + 1):
        if ((h[d:] == h[:-d]) & ok[d:] & ok[:-d]).any():
            return False
    return True


def tie_free_draw(seed, k, draw):
    """the first of the seeds seed, seed + 1000, ... whose draw is tie-free (an m-mer next to its own reverse complement
    -- the two share one canonical hash -- turns up once in a few thousand bases at m = 12)"""
    for s in range(seed, seed + 50_000, 1000):
        data = draw(np.random.default_rng(s))
        if tie_free(data, k):
            return data
    raise AssertionError("no tie-free draw")


@pytest.mark.parametrize("k", [17, 21, 26, 31, 32, 33, 44, 63])
def test_without_ties_the_records_do_not_depend_on_the_pad(k):
    """random reads in which no window holds two equal 25-bit hashes: the multiset of (bases, n, flags, leaf) is the
    same wherever the reads sit in the buffer"""
    data = tie_free_draw(200 + k, k, lambda rng: random_reads(rng, k, n=30, p_bad=0.005))
    want = collections.Counter(msp_ref.runs(with_pad(0, data), k).records())
    assert sum(want.values()) > 50
    for pad in range(1, 32):
        assert collections.Counter(msp_ref.runs(with_pad(pad, data), k).records()) == want


@pytest.mark.parametrize("period", [1, 2, 3, 5])
@pytest.mark.parametrize("k", [17, 31, 32, 33, 63])
def test_in_a_tandem_repeat_the_boundaries_move_with_the_pad_and_the_counts_do_not(k, period):
    """every m-mer of a repeat comes back after `period` positions with the same hash: the minimum of a window is then
    the occurrence with the smallest offset mod 32, so the runs are cut by the BUFFER's 32-byte grid"""
    rng = np.random.default_rng(300 + 10 * k + period)
    read = sc.tandem(rng, period, length=200).data
    assert not tie_free(read, k)
    cuts, counts = set(), []
    for pad in range(32):
        rr = msp_ref.runs(with_pad(pad, read), k)
        assert (msp_ref.covered_positions(rr) == msp_ref.valid_kmers(rr.data, k)).all()
        cuts.add(tuple(int(x) - pad for x in rr.first))
        counts.append(msp_ref.expand(rr, True))
        same_as_oracle(rr, True)
    assert len(cuts) > 1
    for lo, hi, cnt in counts[1:]:
        assert (lo == counts[0][0]).all() and (hi == counts[0][1]).all() and (cnt == counts[0][2]).all()


@pytest.mark.parametrize("k", [17, 27, 31, 32])
def test_complete_run_lengths_agree_with_the_leaf_tests_host_model(k):
    """tests/test_gpu_leaf_twins.py: complete_run_lengths (earliest of equal hashes wins there: tie-free reads only)"""
    from .test_gpu_leaf_twins import complete_run_lengths
    flat = tie_free_draw(400 + k, k, lambda rng: np.concatenate([np.concatenate([sc.bases(rng, 120), [-1]]).astype(np.int8) for _ in range(40)]))
    reads = list(flat.reshape(40, 121)[:, :120])
    for pad in range(32):
        data = with_pad(pad, flat)
        rr = msp_ref.runs(data, k)
        complete = rr.left & rr.right
        assert {int(n) for n in rr.n[complete]} == complete_run_lengths(reads, k)


@pytest.mark.parametrize("k", [17, 31, 32, 33, 64])
def test_packed_runs_round_trip(k):
    """encoder -> decoder of the one-shot packed form, at every pad; reads sampled many times over, so that complete runs
    have multiplicities"""
    rng = np.random.default_rng(500 + k)
    genome = sc.bases(rng, 700)
    for pad in range(32):
        reads = []
        for _ in range(25):
            a = int(rng.integers(0, len(genome) - 200))
            reads += [genome[a:a + 200], [-1]]
        rr = msp_ref.runs(with_pad(pad, np.concatenate(reads).astype(np.int8)), k)
        leaves = msp_ref.by_leaf(rr)
        assert max(max(c.values(), default=0) for c, _ in leaves.values()) > 1
        rows = msp_ref.encode_packed(leaves, k)
        got, hdr = msp_ref.decode_packed(rows, k)
        assert got == leaves
        assert int(hdr[:, 0].sum()) == sum(len(c) for c, _ in leaves.values())
        assert int(hdr[:, 1].sum()) == sum(sum(t.values()) for _, t in leaves.values())


@pytest.mark.parametrize("k", [31, 47])
def test_a_note_decodes_to_a_prefix_of_its_twin(k):
    """msp_runs.h: a note (list position << 5 | n - 1) stands for the first n k-mers of the distinct complete run at that
    position of the leaf's list, closed on the left only; eight notes per row, the last row padded"""
    rng = np.random.default_rng(600 + k)
    runs = sorted((sc.bases(rng, 5 + i + k - 1).tobytes(), 5 + i) for i in range(3))
    comp = collections.Counter({r: 2 + i for i, r in enumerate(runs)})
    trunc = collections.Counter({(sc.bases(rng, k + 1).tobytes(), 2, msp_ref.RIGHT): 1})
    notes = [(i % 3, 1 + i % 5) for i in range(11)]
    rows = msp_ref.encode_packed({77: (comp, trunc)}, k, notes={77: notes})
    got, hdr = msp_ref.decode_packed(rows, k)
    assert tuple(hdr[77]) == (3, 1, 11)
    want = collections.Counter(trunc)
    for pos, n in notes:
        want[(runs[pos][0][:n + k - 1], n, msp_ref.LEFT)] += 1
    assert got == {77: (comp, want)}


def test_the_ladder_builder_places_and_checks_its_features():
    """each family at the ends of its range, on chosen seams, tile seams included; a feature that does not sit where it
    was asked fails the builder's own check"""
    rng = np.random.default_rng(700)
    k, W = 31, msp_ref.params(31).W
    items = sc.items_for(rng, k, W)
    kinds = collections.Counter(f.kind for f, _ in items)
    R = sc.reach(k, W)
    assert kinds["start"] == kinds["end"] == R + 35 and kinds["invalid"] == 2 * R + 33
    assert all(kinds["tandem%d_160" % q] == 32 for q in (1, 2, 3, 5)) and kinds["read30"] == kinds["read31"] == kinds["read48"] == 3
    assert {d for f, d in items if f.kind == "invalid"} == set(range(-(k + W + 2), k + W + 35))
    assert {d for f, d in items if f.kind == "start"} == set(range(-(k + W + 2), 35))
    assert {(d + 64) % 32 for f, d in items if f.kind == "tandem3_160"} == set(range(32))
    for period in (sc.PERIOD1, sc.PERIOD2, sc.PERIOD64):
        lads = sc.ladders(period, items, first_seam=3, min_len=6 * 8 * period)
        assert sum(len(l.placed) for l in lads) == len(items)
        for l in lads:
            assert 6 * 8 * period <= len(l.data) <= sc.MAX_LEN
            assert [p.seam for p in l.placed] == list(range(3, 3 + len(l.placed)))
            assert any(p.seam % 8 == 0 for p in l.placed)
    t = sc.tile_ladder(sc.PERIOD1, sc.tile_items_for(rng, k, W))
    assert all(p.seam % 8 == 0 for p in t.placed) and len(t.data) <= sc.MAX_LEN
    ntiles = sc.tiles_of(len(t.data), sc.PERIOD1)
    chunk_tiles = sc.pipeline_chunk_tiles(ntiles)
    assert ntiles >= 6 and chunk_tiles and set(8 * c for c in chunk_tiles) <= {p.seam for p in t.placed}
    # a moved feature is noticed
    moved = sc.Ladder(np.roll(t.data, 1), t.period, t.placed)
    with pytest.raises(AssertionError):
        sc.check_ladder(moved)
    # the buffer's end and start
    ends = sc.end_buffers(rng, sc.PERIOD1, k, W)
    assert {len(d) - sc.PERIOD1 for _, _, d in ends} == set(range(-33, 34)) and {len(d) % 32 for _, _, d in ends} == set(range(32))
    assert collections.Counter(term for _, term, _ in ends) == {True: 67, False: 67}
    heads = sc.head_buffers(rng, k, W)
    assert {(kind, o) for kind, o, _ in heads} >= {(kind, o) for kind in ("start", "invalid") for o in range(41)}
