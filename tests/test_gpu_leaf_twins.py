"""The leaf kernel's expansion of the distinct complete runs (msp.hip: p3_body phase 2) where a locus is read on both strands.

The record table is keyed by a run's bases as read, so a locus read on both strands sits in it twice, as a run and as its
reverse complement (its strand twin); both are expanded, and their k-mers meet in the k-mer table.  Every canonical
leaf gives a run three lanes, over as many trips of the item loop as it takes (the shared-leaf and the forward-strand
instantiations: three, two or one by the number of runs).  What the cases check: leaves read on one strand, the other
and both with unequal multiplicities; run lengths up to the window; read ends of every length noted with the
forward-strand entry, the reverse-strand entry and both; note lists beyond the one-walk path; a run that is its own
reverse complement; a repeat; tables below and above the sizes at which the lanes per run used to change and the item
loop takes a second trip, and one that overflows; the debug paths and the other instantiations.  (Merging the twins
before the expansion was measured slower and is not in the kernel, msp.hip: STRAND TWINS; these cases passed with it
too.)

All of it can only go wrong inside a leaf, so the inputs put their records into ONE leaf with the planted m-mer of
tests/test_gpu_leaf_scan.py and are built read by read with the builder of tests/test_gpu_leaf_latency.py; a read is
put on the other strand by reverse-complementing it.  Every case that is about one side runs on either side.

Which of a read's ends lands in which list follows from the side the run is cut on, not from the read's strand: a run
cut on its genomic RIGHT is a prefix of the forward-strand entry (read on the reverse strand it is a suffix there and
is reverse-complemented first), a run cut on its genomic LEFT a prefix of the reverse-strand entry.

Run lengths: two planted occurrences d apart give runs of min(d, 18) k-mers at k = 31 (a window holds 18 m-mers), and d
cannot be smaller than the m-mer's 14 bases; a weaker m-mer between two planted ones keeps >= 10 windows to itself.
Complete runs of fewer k-mers only come from unplanted sequence, where every length from 1 on occurs: the random-genome
case.

Expected values never come from the partitioned path: the digest of the CFRK_FORCE_HASH path on the same reads and, entry
for entry, tests/oracle_lib.global_count (test_gpu_leaf_scan: expect / check).
"""
import numpy as np
import pytest

from . import refsem
from .test_gpu_leaf_latency import Leaf, fenced_genome
from .test_gpu_leaf_scan import (HASH_MUL, HASH_MUL_INV, _export_runs, _merge_runs, _same_counts, _shards, check,  # noqa: F401
                                 count_partitioned, ctx, expect, mmer_len, planted_genome, sample_reads, winning_mmer)

pytestmark = pytest.mark.gpu


def rc(read):
    return (3 - read[::-1]).astype(np.int8)


def flat(reads):
    return refsem.flatten(reads)[0]


def cover_reads(genome, pos, m, c=5):
    """span reads of c complete records over every inner occurrence (Leaf.cover), forward strand"""
    leaf = Leaf(genome, pos, m)
    leaf.cover(c)
    return leaf.reads, leaf.complete


def same_as_oracle(ctx, reads, k=31, canonical=True, dbg=0, hint=0, min_leaf=0):
    import cfrk_amd
    data = flat(reads)
    want_digest, want = expect(ctx, data, k, canonical)
    info = check(count_partitioned(ctx, data, k, cfrk_amd.CFRK_CANONICAL if canonical else 0, hint=hint, dbg=dbg), want_digest, want)
    print("reads", len(reads), info)
    assert info["l2_max_leaf"] >= min_leaf
    return info


# ---------------------------------------------------------------------------- strand mixes

@pytest.mark.parametrize("fwd,rev", [(1, 0), (0, 1), (1, 1), (1, 3), (70, 2)])
def test_one_locus_set_on_either_strand_and_on_both(ctx, fwd, rev):
    """ten loci read `fwd` times on the forward and `rev` times on the reverse strand: no twin at all, and twins whose
    multiplicities (1, 1), (1, 3), (70, 2) add"""
    rng = np.random.default_rng(3200 + 100 * fwd + rev)
    m = mmer_len(31)
    genome, pos = fenced_genome(rng, m, 12)
    reads, complete = cover_reads(genome, pos, m)
    same_as_oracle(ctx, reads * fwd + [rc(r) for r in reads] * rev, min_leaf=complete * max(fwd, rev))


# ---------------------------------------------------------------------------- run lengths, other k

def spaced_genome(rng, m, plants, d):
    """the winning m-mer every d bases (d >= m)"""
    mm, _ = winning_mmer(m)
    pos = np.array([20 + d * i for i in range(plants)])
    genome = rng.integers(0, 4, int(pos[-1]) + m + 40).astype(np.int8)
    for q in pos:
        genome[q:q + m] = mm
    return genome, pos


@pytest.mark.parametrize("k,d", [(31, 14), (31, 17), (31, 18), (31, 22), (27, 13), (27, 16), (32, 16), (32, 19)])
def test_runs_of_min_d_and_the_window_k_mers(ctx, k, d):
    """occurrences d apart: runs of min(d, window) k-mers -- at k = 31: 14, 17 and 18 (twice: the window's 18 m-mers bound
    it) --, every locus on both strands (2 + 3 reads), read ends on both sides of every locus"""
    rng = np.random.default_rng(3300 + 40 * k + d)
    m = mmer_len(k)
    assert d >= m
    genome, pos = spaced_genome(rng, m, 16, d)
    reads = sample_reads(rng, genome, 60, both_strands=True, L=110)
    same_as_oracle(ctx, reads, k=k, min_leaf=60)


def complete_run_lengths(reads, k):
    """the lengths, in k-mers, of the complete runs of the reads (host model of msp_dev.h: msp_minimizers): a k-mer's
    minimizer is the canonical m-mer of its window with the smallest ordering hash, compared without the low seven
    bits; a run is a stretch of k-mers with the same minimizer OCCURRENCE, complete when a change of the minimizer, not
    the read's end, closes it on both sides.  (Equal hashes in one window are told apart by position on the device; in
    random bases two of a window's 18 hashes agree in their top 25 bits once in ~10^5 windows, and the earliest wins here.)"""
    m = mmer_len(k)
    w, mask = k - m + 1, (1 << (2 * m)) - 1
    lengths = set()
    for r in reads:
        f = rcv = 0
        h = []
        for i, b in enumerate(int(x) for x in r):
            f = ((f << 2) | b) & mask
            rcv = (rcv >> 2) | ((3 - b) << (2 * (m - 1)))
            if i >= m - 1:
                h.append(((min(f, rcv) * HASH_MUL) & 0xFFFFFFFF) >> 7)
        h = np.array(h)
        occ = np.array([s + int(np.argmin(h[s:s + w])) for s in range(len(r) - k + 1)])
        cuts = [0] + [s for s in range(1, len(occ)) if occ[s] != occ[s - 1]] + [len(occ)]
        lengths.update(b - a for a, b in zip(cuts[1:-2], cuts[2:-1]))        # (the first and the last run end with the read)
    return lengths


def test_unplanted_sequence_has_runs_of_every_length(ctx):
    """3 kb of random bases, 700 reads from both strands: complete runs of 1, 2, 9, 17 and 18 k-mers among all lengths
    (the planted constructions cannot make one shorter than 10), on both strands with read ends of every length on
    either side -- a few entries in each of many leaves"""
    rng = np.random.default_rng(3350)
    genome = rng.integers(0, 4, 3000).astype(np.int8)
    reads = sample_reads(rng, genome, 700, both_strands=True, L=100)
    lengths = complete_run_lengths(reads, 31)
    print(sorted(lengths))
    assert {1, 2, 9, 17, 18} <= lengths and max(lengths) <= 18
    same_as_oracle(ctx, reads)


# ---------------------------------------------------------------------------- read ends

def end_sweeps(genome, pos, m, J, side):
    """reads whose end moves base by base through the run of occurrence J, the run's other side closed by two more
    occurrences and their margin: the run is cut to every length 1 .. n.  side "right": cut on the genomic right (a
    prefix of the forward-strand entry), "left": on the genomic left (a prefix of the reverse-strand entry).  Every
    second read is given on the reverse strand."""
    margin, out = max(12, m) - 1, []
    if side == "right":
        for E in range(int(pos[J]) + m, int(pos[J + 1]) + m + margin + 1):
            out.append(genome[pos[J - 2] - margin:E].copy())
    else:
        for S in range(int(pos[J - 1]) - margin, int(pos[J]) + 1):
            out.append(genome[S:pos[J + 2] + m + margin].copy())
    return [r if i % 2 == 0 else rc(r) for i, r in enumerate(out)]


@pytest.mark.parametrize("sides", [("right",), ("left",), ("right", "left")], ids=["right", "left", "both"])
@pytest.mark.parametrize("fwd,rev", [(1, 1), (2, 0)], ids=["twins", "forward_only"])
def test_read_ends_of_every_length_on_one_twin_the_other_and_both(ctx, sides, fwd, rev):
    """the noted lengths 1 .. n in the forward-strand entry's list only, in the reverse-strand entry's only, and in both:
    one canonical k-mer then takes counts from both entries' lists.  forward_only: the reverse-strand entry does not exist, and the
    runs cut on the left find no complete twin (they are counted k-mer by k-mer)"""
    rng = np.random.default_rng(3400 + 10 * len(sides) + (sides[0] == "left") + 100 * rev)
    m = mmer_len(31)
    genome, pos = fenced_genome(rng, m, 14)
    base, _ = cover_reads(genome, pos, m)
    reads = base * fwd + [rc(r) for r in base] * rev
    for side in sides:
        for J in (4, 7):
            reads += end_sweeps(genome, pos, m, J, side)
    same_as_oracle(ctx, reads, min_leaf=40)


@pytest.mark.parametrize("side", ["right", "left"])
def test_more_than_127_noted_ends_on_one_twin_take_the_slow_walk(ctx, side):
    """140 + the sweep's ~30 read ends in ONE entry's list: beyond the seven bits of the one-walk counts, so the wave
    walks its lists per k-mer pair.  The forward-strand entry's list, and the reverse-strand entry's."""
    rng = np.random.default_rng(3500 + (side == "left"))
    m = mmer_len(31)
    genome, pos = fenced_genome(rng, m, 14)
    base, _ = cover_reads(genome, pos, m)
    sweep = end_sweeps(genome, pos, m, 6, side)
    reads = base + [rc(r) for r in base] + sweep + [sweep[len(sweep) // 2], sweep[3]] * 70
    same_as_oracle(ctx, reads, min_leaf=140)


# ---------------------------------------------------------------------------- palindrome, repeat

def palindromic_mmer(m):
    """the m-mer (m even) that is its own reverse complement with the smallest ordering hash above 2^10 -> (bases, hash)"""
    assert m % 2 == 0
    h = np.arange(1 << 10, 1 << 21, dtype=np.uint64)
    c = (h * np.uint64(HASH_MUL_INV)) & np.uint64(0xFFFFFFFF)
    ok = (c >> np.uint64(2 * m)) == 0
    h, c = h[ok], c[ok]
    r, x = np.zeros_like(c), c.copy()
    for _ in range(m):
        r = (r << np.uint64(2)) | (np.uint64(3) - (x & np.uint64(3)))
        x >>= np.uint64(2)
    i = int(np.argmax(r == c))
    assert r[i] == c[i] and (int(c[i]) * HASH_MUL) & 0xFFFFFFFF == int(h[i])
    return np.array([(int(c[i]) >> (2 * (m - 1 - j))) & 3 for j in range(m)], np.int8), int(h[i])


def test_a_run_that_is_its_own_reverse_complement(ctx):
    """a palindromic m-mer in the middle of a flank and the flank's reverse complement, alone in its windows: the run of
    all 18 windows that hold it is 48 bases that read the same on both strands -- ONE entry whatever the strand of the
    read, which must be counted once per read and not per strand; its k-mers J and n - 1 - J are the same key"""
    k, m = 31, mmer_len(31)
    mm, h = palindromic_mmer(m)
    assert h < 1 << 20                                           # (a window of 18 random hashes beats it once in ~200)
    rng = np.random.default_rng(3600)
    flank = rng.integers(0, 4, 60).astype(np.int8)
    locus = np.concatenate([flank, mm, rc(flank)])
    assert (locus == rc(locus)).all()
    genome = np.concatenate([rng.integers(0, 4, 100).astype(np.int8), locus, rng.integers(0, 4, 100).astype(np.int8)])
    reads = []
    for i in range(40):                                          # 100-base reads over the locus, ends everywhere
        p = 60 + 3 * i
        r = genome[p:p + 100].copy()
        reads.append(r if i % 3 else rc(r))
    same_as_oracle(ctx, reads)


def test_a_genomic_repeat_adds_across_runs(ctx):
    """40 bases of one locus copied into another: two loci (four entries, two pairs of twins) share ten k-mers, which the
    k-mer table still has to add up across runs"""
    rng = np.random.default_rng(3700)
    m = mmer_len(31)
    genome, pos = fenced_genome(rng, m, 14)
    a, b = int(pos[4]) - 13, int(pos[9]) - 13
    genome[b:b + 40] = genome[a:a + 40]
    base, _ = cover_reads(genome, pos, m)
    same_as_oracle(ctx, base * 2 + [rc(r) for r in base] * 3, min_leaf=40)


# ---------------------------------------------------------------------------- table chains, lanes per run, trips

@pytest.mark.parametrize("both", [True, False], ids=["both_strands", "forward_only"])
@pytest.mark.parametrize("distinct", [40, 330, 350, 520, 1100])
def test_distinct_runs_in_one_leaf(ctx, distinct, both):
    """`distinct` entries in the 1024-slot table (two per planted occurrence when both strands are read): twins at the end
    of probe chains; below and above 341 and 512 entries (three, two lanes, one lane per run before every canonical leaf
    took three): 350 / 520 runs x 3 lanes take two trips of the item loop; 1100 do not fit the table: the leaf is
    counted from its streams"""
    rng = np.random.default_rng(3800 + distinct + both)
    m = mmer_len(31)
    plants = distinct // 2 if both else distinct
    genome, pos = planted_genome(rng, m, plants)
    nreads = max(30, plants // 2)                                # ~5-fold: nearly every occurrence has a complete run
    reads = sample_reads(rng, genome, nreads, both_strands=both)
    same_as_oracle(ctx, reads, min_leaf=5 * nreads)


# ---------------------------------------------------------------------------- the debug paths, forward-strand counting

def _mixed_leaf(seed):
    rng = np.random.default_rng(seed)
    m = mmer_len(31)
    genome, pos = fenced_genome(rng, m, 14)
    base, _ = cover_reads(genome, pos, m)
    reads = base * 3 + [rc(r) for r in base] * 2
    for side in ("right", "left"):
        reads += end_sweeps(genome, pos, m, 5, side)
    return reads


@pytest.mark.parametrize("which", ["no_anchors", "rt_overflow", "forward_strand"])
def test_debug_paths_and_forward_strand(ctx, which):
    """CFRK_DEBUG_NO_ANCHORS (no noted lengths), CFRK_DEBUG_FORCE_RT_OVERFLOW (the table is not listed) and forward-strand
    counting, where a run and its reverse complement are different keys, on a leaf with both strands and read ends on
    either side"""
    import cfrk_amd
    dbg = {"no_anchors": cfrk_amd.lib.CFRK_DEBUG_NO_ANCHORS, "rt_overflow": cfrk_amd.CFRK_DEBUG_FORCE_RT_OVERFLOW}.get(which, 0)
    same_as_oracle(ctx, _mixed_leaf(3900), canonical=which != "forward_strand", dbg=dbg, min_leaf=100)


# ---------------------------------------------------------------------------- the other instantiations

def test_a_leaf_shared_by_record(ctx):
    """a capacity hint above 2.7e8: msp_p3_kernel<.., true>, which keeps three, two or one lane per run"""
    same_as_oracle(ctx, _mixed_leaf(4000), hint=300_000_000, min_leaf=100)


def test_two_emulated_ranks_through_the_runs_exchange(ctx):
    """2000 reads of a 300-run genome, both strands, split over two ranks: the senders deduplicate (exporting leaves: no
    expansion), the owners count weighted runs -- one shot and pipelined (msp_p3_lists_kernel)"""
    import cfrk_amd
    from .test_gpu_parity import _pipelined_exchange
    k, flags, R, L, world = 31, cfrk_amd.CFRK_CANONICAL, 2000, 150, 2
    rng = np.random.default_rng(4100)
    genome, pos = planted_genome(rng, mmer_len(k), 150)
    data = flat(sample_reads(rng, genome, R))
    want_digest, want = expect(ctx, data, k, True)
    sends = [_export_runs(ctx, shard, k, flags, world, 5 * R // world) for shard in _shards(data, R, L, world)]
    _same_counts(_merge_runs(sends, k, flags, world, want_digest), want, k)
    # (a deferred add keeps the first sizing of its leaf streams: eight reads per rank are what one leaf can take)
    small = np.ascontiguousarray(data[:16 * (L + 1)])
    _, (wlo, _, wcnt) = expect(ctx, small, k, True)
    merged = _pipelined_exchange(ctx, small, 16, L, k, flags, world, 2, 0)
    assert merged is not None
    assert len(merged) == len(wlo) and all(merged[int(a)] == int(b) for a, b in zip(wlo, wcnt))
