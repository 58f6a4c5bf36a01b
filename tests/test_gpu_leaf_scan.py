"""The leaf kernel's scan of the complete stream (msp.hip: p3_body phase 1a) on inputs that put their records into ONE leaf.

The scan -- home-slot step, displaced-run cache, leftover sets, probe loop, the peeled tail -- can only go wrong inside a leaf, and random reads give every leaf a handful of records.  Here an m-mer whose
ordering hash (msp_dev.h: hash_mmer, restated below) is small enough to win almost every window is planted every 12-16
bases of an otherwise random genome: every k-mer of a read then has a planted occurrence as its minimizer, every
occurrence is a distinct run (per strand) of the same leaf, and the number of distinct runs and of records in that leaf
is chosen by the genome's length and the number of reads.  Every case asserts through msp_info() that the largest leaf
stream really holds what the case is about, so a later change of the hash or of the window cannot hollow it out.

Expected values never come from the partitioned path: they are the digest of the CFRK_FORCE_HASH path on the same reads
and, key by key, tests/oracle_lib.global_count.
"""
import numpy as np
import pytest

from . import oracle_lib as orc
from . import refsem

pytestmark = pytest.mark.gpu

STEP = 2048                # records one trip of the scan's main loop takes (two per thread, 16 waves)
SLICE = 512                # a quarter of a trip: below it half the waves of the workgroup have no record at all
RT = 1024                  # slots of the record table
BT_MIN_RUNS = 8192         # complete records from which an overflowing leaf gets the pool-wide table
HASH_MUL = 0x9E3779B1
HASH_MUL_INV = pow(HASH_MUL, -1, 1 << 32)


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


def mmer_len(k):
    """msp.hip: msp_params"""
    w = min(k - 11 if k <= 26 else k - 12, 49 - k)
    return k - w + 1


def _revcomp_int(x, m):
    r = 0
    for _ in range(m):
        r = (r << 2) | (3 - (x & 3))
        x >>= 2
    return r


def winning_mmer(m):
    """the canonical m-mer with the smallest ordering hash above 2^10 (first base most significant) -> (bases, hash).
    Hashes are compared without their low seven bits, and bits 8..23 name the leaf."""
    for h in range(1 << 10, 1 << 24):
        c = (h * HASH_MUL_INV) & 0xFFFFFFFF
        if c >> (2 * m):
            continue
        rc = _revcomp_int(c, m)
        if c < rc:                                             # canonical, not its own reverse complement
            assert (c * HASH_MUL) & 0xFFFFFFFF == h
            return np.array([(c >> (2 * (m - 1 - j))) & 3 for j in range(m)], np.int8), h
    raise AssertionError("no winning m-mer")


def planted_genome(rng, m, plants):
    """random bases with the winning m-mer every 12..16 bases -- every max(12, m)..16 for the longer m-mers of k >= 31,
    whose occurrences would overlap otherwise -> (genome, start of every occurrence)"""
    mm, h = winning_mmer(m)
    assert h < 1 << 20                                         # a window of <= 18 random hashes beats it once in ~200
    pos, p = [], 20
    for _ in range(plants):
        pos.append(p)
        p += int(rng.integers(max(12, m), 17))
    genome = rng.integers(0, 4, p + 40).astype(np.int8)
    for q in pos:
        genome[q:q + m] = mm
    return genome, np.array(pos)


def sample_reads(rng, genome, n, both_strands=True, L=150):
    reads = []
    for _ in range(n):
        p = int(rng.integers(0, len(genome) - L + 1))
        r = genome[p:p + L].copy()
        if both_strands and rng.random() < 0.5:
            r = (3 - r[::-1]).astype(np.int8)
        reads.append(r)
    return reads


def pad_reads(genome, pos, m, n, first=1):
    """n reads that hold exactly three planted occurrences each and max(12, m) - 1 bases around them (one base short of a
    fourth occurrence): the first and the last window of the read hold an outer occurrence alone (the next one starts
    >= 2 * max(12, m) - 1 > 18 positions in), so each outer occurrence has a run, closed by the read's end; occurrences
    two apart are >= 24 bases from each other and a window is <= 18 m-mers, so some window holds the middle one alone:
    its run is closed by a change of the minimizer on both sides -> ONE complete record per read"""
    out, margin = [], max(12, m) - 1
    for i in range(first, first + n):
        j = 1 + (i % (len(pos) - 2))
        out.append(genome[pos[j - 1] - margin:pos[j + 1] + m + margin].copy())
    return out


def count_partitioned(ctx, data, k, flags, hint=0, dbg=0):
    import cfrk_amd
    g = cfrk_amd.GlobalCounter(ctx, k, flags, hint)
    g.set_debug_flags(dbg)
    try:
        g.add(data)
    finally:
        g.set_debug_flags(0)
    return g


def expect(ctx, data, k, canonical):
    """(digest of the CFRK_FORCE_HASH path, the oracle's keys and counts)"""
    import cfrk_amd
    gh = cfrk_amd.GlobalCounter(ctx, k, (cfrk_amd.CFRK_CANONICAL if canonical else 0) | cfrk_amd.CFRK_FORCE_HASH, 0)
    gh.add(data)
    want = orc.global_count(data, k, orc.ORC_CANONICAL if canonical else 0)
    d = gh.digest()
    assert d == orc.digest(*want, two_word=k > 32)
    return d, want


def check(g, want_digest, want):
    info = g.msp_info()
    assert info["l2_records"] > 0 and info["spilled_records"] == 0
    assert g.digest() == want_digest
    lo, hi, cnt = g.export()
    wlo, whi, wcnt = want
    assert len(lo) == len(wlo) and (lo == wlo).all() and (cnt.astype(np.uint64) == wcnt).all()
    return info


# (distinct runs aimed at -- two per planted occurrence, one per strand --, reads, what the leaf's complete stream must hold)
#   records: "below_slice" < SLICE; "below_step": between SLICE and STEP (the first waves take one trip of the main
#   loop, the others only the tail); "odd": several trips of the main loop and a partly filled tail; "mult64": an exact
#   multiple of 64 (no lane of the tail is idle); "step": exactly STEP -- one trip for every wave and nothing for the tail
CASES = [
    (40, 40, "below_slice"),
    (40, 750, "odd"),
    (300, 140, "below_step"),
    (300, 1500, "mult64"),       # the headline workload's load: ~0.3
    (300, 260, "step"),
    (900, 1500, "odd"),          # table nearly full, long probe chains
    (1500, 2000, "odd"),         # more distinct runs than slots, >= BT_MIN_RUNS records: the pool-wide table
    (1500, 600, "odd_small"),    # ... fewer records than that: counted from the streams
]


def _shape_leaf(ctx, rng, k, flags, genome, pos, reads, kind):
    """pad / cut the reads until the largest leaf stream is what `kind` asks for -> (data, records in it)"""
    m = mmer_len(k)

    def records(rs):
        data, _, _ = refsem.flatten(rs)
        return data, count_partitioned(ctx, data, k, flags).msp_info()["l2_max_leaf"]

    data, n = records(reads)
    if kind == "mult64":
        reads = reads + pad_reads(genome, pos, m, (-n) % 64)
        data, n = records(reads)
        assert n % 64 == 0 and n > 2 * STEP
    elif kind == "step":
        while n > STEP:                                        # ~9 complete records per read
            reads = reads[:-max(1, (n - STEP) // 12)]
            data, n = records(reads)
        reads = reads + pad_reads(genome, pos, m, STEP - n)
        data, n = records(reads)
        assert n == STEP
    elif kind in ("odd", "odd_small"):
        if n % 64 == 0:
            reads = reads + pad_reads(genome, pos, m, 1)
            data, n = records(reads)
        assert n % 64 != 0 and n > 2 * STEP
        assert (n >= BT_MIN_RUNS) if kind == "odd" and len(pos) > 700 else True
        assert n < BT_MIN_RUNS if kind == "odd_small" else True
    elif kind == "below_slice":
        assert 64 < n < SLICE
    elif kind == "below_step":
        assert SLICE < n < STEP
    return data, n


@pytest.mark.parametrize("distinct,nreads,kind", CASES, ids=["%d-%s-%d" % (d, s, r) for d, r, s in CASES])
def test_one_leaf_distinct_runs_and_record_counts(ctx, distinct, nreads, kind):
    """k = 31, canonical: 40 / 300 / 900 / 1500 distinct runs in the leaf against every length class of its stream"""
    import cfrk_amd
    k, flags = 31, cfrk_amd.CFRK_CANONICAL
    rng = np.random.default_rng(7000 + distinct + nreads)
    genome, pos = planted_genome(rng, mmer_len(k), distinct // 2)
    reads = sample_reads(rng, genome, nreads)
    data, n = _shape_leaf(ctx, rng, k, flags, genome, pos, reads, kind)
    want_digest, want = expect(ctx, data, k, True)
    info = check(count_partitioned(ctx, data, k, flags), want_digest, want)
    print("distinct aimed at", distinct, "reads", len(data) // 151, "largest leaf stream", n, info)
    assert info["l2_max_leaf"] == n
    # (every planted occurrence away from the genome's ends is a run of the leaf on either strand; that the leaf holds
    #  about `distinct` of them shows in the records per read: ~9 of a read's ~11 occurrences are complete runs)
    assert n >= 5 * nreads


@pytest.mark.parametrize("distinct,nreads", [(300, 1500), (1500, 2000), (40, 40)])
def test_one_leaf_with_the_record_table_forced_to_overflow(ctx, distinct, nreads):
    """CFRK_DEBUG_FORCE_RT_OVERFLOW: the scan runs as ever, its table is then declared full -- second chance in the
    pool-wide table (>= BT_MIN_RUNS records, or forced) and the stream path behind it"""
    import cfrk_amd
    k, flags = 31, cfrk_amd.CFRK_CANONICAL
    rng = np.random.default_rng(7100 + distinct)
    genome, pos = planted_genome(rng, mmer_len(k), distinct // 2)
    data, _, _ = refsem.flatten(sample_reads(rng, genome, nreads))
    want_digest, want = expect(ctx, data, k, True)
    info = check(count_partitioned(ctx, data, k, flags, dbg=cfrk_amd.CFRK_DEBUG_FORCE_RT_OVERFLOW), want_digest, want)
    assert info["l2_max_leaf"] >= 5 * nreads


@pytest.mark.parametrize("k,canonical,nreads", [(28, True, 800), (32, True, 800), (31, False, 800), (27, True, 1400), (27, True, 300)])
def test_one_leaf_other_k_and_strand(ctx, k, canonical, nreads):
    """k = 28 / 32 (other m-mers, other masks of the slot hash), forward-strand counting, and k = 27: a leaf of
    >= BT_MIN_RUNS complete records goes to the pool-wide table at once (big_first: no cache), a smaller one
    through the ordinary scan -- both as before"""
    import cfrk_amd
    flags = cfrk_amd.CFRK_CANONICAL if canonical else 0
    rng = np.random.default_rng(7200 + 10 * k + canonical)
    genome, pos = planted_genome(rng, mmer_len(k), 150)
    data, _, _ = refsem.flatten(sample_reads(rng, genome, nreads))
    want_digest, want = expect(ctx, data, k, canonical)
    info = check(count_partitioned(ctx, data, k, flags), want_digest, want)
    print("k", k, info)
    if k == 27:
        assert (info["l2_max_leaf"] >= BT_MIN_RUNS) == (nreads == 1400)
    assert info["l2_max_leaf"] >= 5 * nreads


def test_one_leaf_shared_by_several_workgroups(ctx):
    """a capacity hint above 2.7e8 makes the job share its leaves by record (msp_p3_kernel<.., true>): the general scan,
    which gathers a workgroup's own records before the table look-up"""
    import cfrk_amd
    k, flags = 31, cfrk_amd.CFRK_CANONICAL
    rng = np.random.default_rng(7300)
    genome, pos = planted_genome(rng, mmer_len(k), 150)
    data, _, _ = refsem.flatten(sample_reads(rng, genome, 1000))
    want_digest, want = expect(ctx, data, k, True)
    info = check(count_partitioned(ctx, data, k, flags, hint=300_000_000), want_digest, want)
    assert info["l2_max_leaf"] >= 5000


def _shards(data, R, L, world):
    return [np.ascontiguousarray(data[(R * r // world) * (L + 1):(R * (r + 1) // world) * (L + 1)]) for r in range(world)]


def _heaviest_leaf(host, rows, world, rows_per_record=1):
    """the (distinct, truncated, noted) header triple of the leaf with the most rows in one rank's packed buffer
    (msp_runs.h: every owner's segment starts with one triple per leaf of that owner)"""
    lpp = -(-65536 // world)
    best, at = (0, 0, 0), 0
    for r in rows:
        hdr = host[at:at + (lpp * 12 + 15) // 16].view(np.uint32).reshape(-1)[:3 * lpp].reshape(lpp, 3)
        nd, nu, na = (int(x) for x in hdr[np.argmax(rows_per_record * (hdr[:, 0] + hdr[:, 1]) + (hdr[:, 2] + 7) // 8)])
        if nd + nu + na > sum(best):
            best = (nd, nu, na)
        at += r
    return best


def _export_runs(ctx, shard, k, flags, world, min_leaf):
    """one rank: a CFRK_RUNS_ONLY add and the one-shot export -> (packed rows as uint64 [rows, 2], rows per owner)"""
    import cfrk_amd
    g = cfrk_amd.GlobalCounter(ctx, k, flags | cfrk_amd.CFRK_RUNS_ONLY, 0)
    g.add(shard)
    if min_leaf:
        assert g.msp_info()["l2_max_leaf"] >= min_leaf
    cap = 1 << 18
    d = ctx.alloc(cap * 16)
    rows = g.export_runs_device(d, cap, world)
    host = np.empty((sum(rows), 2), np.uint64)
    ctx.d2h(host, d)
    ctx.free(d)
    return host, rows


def _merge_runs(sends, k, flags, world, want_digest):
    """every owner merges what the ranks sent it -> {key: count} over all owners (two-word keys: key = (lo, hi))"""
    import cfrk_amd
    merged = {}
    c2 = cfrk_amd.Context(0)
    try:
        for owner in range(world):
            segs = [host[sum(rows[:owner]):sum(rows[:owner]) + rows[owner]] for host, rows in sends]
            buf = np.concatenate(segs)
            d = c2.alloc(max(len(buf), 1) * 16)
            c2.h2d(d, buf)
            og = cfrk_amd.GlobalCounter(c2, k, flags, 0)
            og.merge_runs_device(d, [rows[owner] for _, rows in sends])
            if world == 1:
                assert og.digest() == want_digest
            lo, hi, cnt = og.export()
            c2.free(d)
            for i, (key, c) in enumerate(zip(lo, cnt)):
                key = int(key) if k <= 32 else (int(key), int(hi[i]))
                assert key not in merged                      # owners hold disjoint key sets
                merged[key] = int(c)
    finally:
        c2.close()
    return merged


def _same_counts(merged, want, k):
    wlo, whi, wcnt = want
    keys = [int(a) for a in wlo] if k <= 32 else [(int(a), int(b)) for a, b in zip(wlo, whi)]
    assert len(merged) == len(keys) and all(merged[a] == int(b) for a, b in zip(keys, wcnt))


@pytest.mark.parametrize("world", [1, 2])
def test_one_leaf_through_the_runs_exchange_weighted(ctx, world):
    """export_runs_device on one context into merge_runs_device on another: the owner's leaf kernel counts DISTINCT runs
    with their multiplicities (P3_WEIGHTED: the general scan, increment = the record's weight)"""
    import cfrk_amd
    k, flags, R, L = 31, cfrk_amd.CFRK_CANONICAL, 1200, 150
    rng = np.random.default_rng(7400 + world)
    genome, pos = planted_genome(rng, mmer_len(k), 150)
    data, _, _ = refsem.flatten(sample_reads(rng, genome, R))
    want_digest, want = expect(ctx, data, k, True)
    sends = [_export_runs(ctx, shard, k, flags, world, 5 * R // world) for shard in _shards(data, R, L, world)]
    _same_counts(_merge_runs(sends, k, flags, world, want_digest), want, k)


@pytest.mark.parametrize("world", [1, 2])
def test_one_leaf_with_more_distinct_runs_than_the_senders_table_through_the_runs_exchange(ctx, world):
    """the (1500, 2000) load of CASES: every rank's leaf holds more distinct complete runs than the sender's record table
    has slots -- the table fails for real (not by CFRK_DEBUG_FORCE_RT_OVERFLOW), the runs leave undeduplicated with
    multiplicity 1 and without notes, and the owner's table merges them"""
    import cfrk_amd
    k, flags, R, L = 31, cfrk_amd.CFRK_CANONICAL, 2000, 150
    rng = np.random.default_rng(7600 + world)
    genome, pos = planted_genome(rng, mmer_len(k), 750)
    data, _, _ = refsem.flatten(sample_reads(rng, genome, R))
    want_digest, want = expect(ctx, data, k, True)
    sends = [_export_runs(ctx, shard, k, flags, world, 5 * R // world) for shard in _shards(data, R, L, world)]
    for host, rows in sends:
        nd, nu, na = _heaviest_leaf(host, rows, world)
        print("heaviest leaf: distinct", nd, "truncated", nu, "noted", na)
        # (undeduplicated: as many "distinct" runs as the leaf has complete records -- ~9 per read --, far more than the
        #  ~1500 runs that are distinct, which no 1024-slot table holds)
        assert nd >= 5 * R // world and nd > RT and na == 0 and nu > 0
    _same_counts(_merge_runs(sends, k, flags, world, want_digest), want, k)


def mmer_len2(k):
    """msp2.hip: msp2_count_tiles"""
    return 14 if k & 1 else 13


@pytest.mark.parametrize("k,world", [(31, 1), (31, 2), (47, 1), (47, 2)])
def test_one_leaf_with_thousands_of_truncated_runs_noted_and_not_through_the_runs_exchange(ctx, k, world):
    """>= 3000 reads of the 300-run genome: several thousand read ends in one leaf, nearly all of them a prefix of a
    complete run of their rank (notes); a few reads of a second genome whose outer occurrences only ever meet a read's
    end have no twin (records).  The split of the truncated stream then runs many trips with both cursors moving, and a
    note count that is no multiple of 8 leaves padding behind.  k = 47: the same through the two-word kernels (no
    msp_info() of the record levels there: the packed header alone says what the leaf holds)."""
    import cfrk_amd
    flags, R, L = cfrk_amd.CFRK_CANONICAL, 3000, 150
    m = mmer_len(k) if k <= 32 else mmer_len2(k)
    rng = np.random.default_rng(7700 + 10 * k + world)
    genome, pos = planted_genome(rng, m, 150)
    lonely, lpos = planted_genome(rng, m, 3)
    shards, sends = [], []
    for r in range(world):
        reads = sample_reads(rng, genome, R // world) + pad_reads(lonely, lpos, m, 4)
        for extra in range(9):
            shard, _, _ = refsem.flatten(reads)
            host, rows = _export_runs(ctx, shard, k, flags, world, 5 * R // world if k <= 32 else 0)
            nd, nu, na = _heaviest_leaf(host, rows, world, 1 if k <= 32 else 2)
            if na % 8:
                break
            reads = reads + sample_reads(rng, genome, 1)        # (one more read: two more read ends)
        print("rank", r, "heaviest leaf: distinct", nd, "truncated", nu, "noted", na, "extra reads", extra)
        assert na > 0 and nu > 0 and na % 8 != 0 and nu + na >= 2 * (R // world) - 200 and nd >= 150
        shards.append(shard)
        sends.append((host, rows))
    data = np.concatenate(shards)
    want_digest, want = expect(ctx, data, k, True)
    _same_counts(_merge_runs(sends, k, flags, world, want_digest), want, k)


@pytest.mark.parametrize("world", [1, 2])
def test_one_leaf_through_the_pipelined_runs_exchange_lists(ctx, world):
    """export_runs_async / merge_runs_group_device: the owner's leaf kernel reads the ranks' lists of the leaf in place
    (msp_p3_lists_kernel: the general scan over N lists, weighted)"""
    import cfrk_amd
    from .test_gpu_parity import _pipelined_exchange
    # (a deferred add cannot lay its leaf streams out again, and a small batch gives every leaf a fixed stride of ~100
    #  records: eight reads per rank, ~70 complete records, is what one leaf can take here)
    k, flags, R, L = 31, cfrk_amd.CFRK_CANONICAL, 8 * world, 150
    rng = np.random.default_rng(7500 + world)
    genome, pos = planted_genome(rng, mmer_len(k), 150)
    data, _, _ = refsem.flatten(sample_reads(rng, genome, R))
    want_digest, want = expect(ctx, data, k, True)
    assert count_partitioned(ctx, _shards(data, R, L, world)[0], k, flags).msp_info()["l2_max_leaf"] >= 40
    merged = _pipelined_exchange(ctx, data, R, L, k, flags, world, 2, 0)
    assert merged is not None
    wlo, _, wcnt = want
    assert len(merged) == len(wlo) and all(merged[int(a)] == int(b) for a, b in zip(wlo, wcnt))
