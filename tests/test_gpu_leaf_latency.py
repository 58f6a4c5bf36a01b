"""The leaf kernel's loads that were moved off its critical path (msp.hip: p3_body), at the edges of a leaf's two streams.

What moved: the first TL_CAP truncated records are asked for in front of the cache merge (branch-free: a leaf without
truncated runs loads one record that is surely there; the rare paths ask again), and the copy-out ranks a wave's slots
with one LDS atomic, the last wave to come by asks the list's cursor and writes the per-leaf index.  (The scan's first
records asked for at the kernel's entry, its loop one trip ahead of its loads and the truncated loops of phase 2 one
trip ahead were measured and not kept; the cases written for them -- every length class of the complete stream, the
lists of the truncated runs without a twin, the tail beyond TL_CAP -- stay: the code they run is next to what moved.
The two-word kernels of msp2.hip and the merge kernels keep the shared ranking helper as it was: no case for them here.)
All of it can only go wrong inside a leaf, so the inputs put their records
into ONE leaf with the planted m-mer of tests/test_gpu_leaf_scan.py, and here they are built read by read so that the
leaf's streams hold an exact number of records:

  * a SPAN read covers c + 2 planted occurrences and one base less than the margin to the next on either side: c complete
    records (the inner occurrences) and two truncated ones (the outer occurrences, cut by the read's ends), each of them a
    prefix or suffix of the complete run of its locus, which another span read supplies -- they have a twin;
  * a LONE read covers one occurrence: one record cut on both sides, which never has a twin;
  * the first and the last occurrence of the genome are ANOTHER m-mer, of another leaf (`fenced_genome`): a span read that
    ends on one of them leaves that truncated record elsewhere, so the leaf under test can hold complete records and no
    truncated ones, and no truncated run without a twin but the lone reads'.

Every case asserts through msp_info() that the job's records and its largest stream are what was built.  Expected values
never come from the partitioned path: they are the digest and the full export of the CFRK_FORCE_HASH path on the same reads.
"""
import numpy as np
import pytest

from . import refsem
from .test_gpu_leaf_scan import (HASH_MUL, HASH_MUL_INV, BT_MIN_RUNS, _revcomp_int, _shape_leaf, check, count_partitioned,  # noqa: F401
                                 ctx, mmer_len, pad_reads, planted_genome, sample_reads, winning_mmer)

pytestmark = pytest.mark.gpu

P3_THREADS = 1024
TL_CAP = 4096              # truncated records that go through the length-sorted list / the anchoring pass
FL_CAP = 1024              # truncated runs without a twin an anchored leaf lists


def other_leaf_mmer(m):
    """the canonical m-mer with the smallest ordering hash in a LATER leaf than winning_mmer's (bits 8..23 of the hash
    name the leaf) -- it still wins every window of random bases, and loses to the planted one (compared without the low
    seven bits)"""
    _, h1 = winning_mmer(m)
    for h in range(((h1 >> 8) + 1) << 8, 1 << 24):
        c = (h * HASH_MUL_INV) & 0xFFFFFFFF
        if c >> (2 * m):
            continue
        if c < _revcomp_int(c, m):
            assert (c * HASH_MUL) & 0xFFFFFFFF == h and h < 1 << 20
            return np.array([(c >> (2 * (m - 1 - j))) & 3 for j in range(m)], np.int8)
    raise AssertionError("no second m-mer")


def fenced_genome(rng, m, plants):
    """planted_genome whose first and last occurrence are the other leaf's m-mer"""
    genome, pos = planted_genome(rng, m, plants)
    mm2 = other_leaf_mmer(m)
    genome[pos[0]:pos[0] + m] = mm2
    genome[pos[-1]:pos[-1] + m] = mm2
    return genome, pos


class Leaf:
    """reads for one leaf and what they put there: complete / truncated records of the leaf under test, truncated
    records of the fence's leaf"""

    def __init__(self, genome, pos, m):
        self.genome, self.pos, self.m, self.margin = genome, pos, m, max(12, m) - 1
        self.reads, self.complete, self.truncated, self.fence = [], 0, 0, 0

    def span(self, j, c):
        """occurrences j - 1 .. j + c: c complete records, two truncated ones"""
        pos, last = self.pos, len(self.pos) - 1
        assert 1 <= j and j + c <= last and c >= 1
        self.reads.append(self.genome[pos[j - 1] - self.margin:pos[j + c] + self.m + self.margin].copy())
        self.complete += c
        for outer in (j - 1, j + c):
            if outer in (0, last):
                self.fence += 1
            else:
                self.truncated += 1

    def lone(self, j):
        assert 1 <= j < len(self.pos) - 1
        self.reads.append(self.genome[self.pos[j] - self.margin:self.pos[j] + self.m + self.margin].copy())
        self.truncated += 1

    def cover(self, c, times=1):
        """span reads of c complete records over every inner occurrence, `times` over: every truncated record they leave
        in the leaf has its twin"""
        for _ in range(times):
            for j in range(1, len(self.pos) - 1 - c + 1):
                self.span(j, c)

    def data(self):
        return refsem.flatten(self.reads)[0]


def expect_hash(ctx, data, k, canonical):
    """digest and full export of the CFRK_FORCE_HASH path"""
    import cfrk_amd
    gh = cfrk_amd.GlobalCounter(ctx, k, (cfrk_amd.CFRK_CANONICAL if canonical else 0) | cfrk_amd.CFRK_FORCE_HASH, 0)
    gh.add(data)
    return gh.digest(), gh.export()


def same_result(g, want):
    want_digest, (wlo, whi, wcnt) = want
    info = g.msp_info()
    assert info["l2_records"] > 0 and info["spilled_records"] == 0 and info["spilled_kmers"] == 0
    assert g.digest() == want_digest
    lo, hi, cnt = g.export()
    assert len(lo) == len(wlo) and (lo == wlo).all() and (cnt == wcnt).all()
    return info


def run_leaf(ctx, leaf, k=31, canonical=True, dbg=0):
    """count the leaf's reads on the partitioned path, compare with the hash path -> msp_info(), shape asserted"""
    import cfrk_amd
    flags = cfrk_amd.CFRK_CANONICAL if canonical else 0
    data = leaf.data()
    want = expect_hash(ctx, data, k, canonical)
    info = same_result(count_partitioned(ctx, data, k, flags, dbg=dbg), want)
    print("complete", leaf.complete, "truncated", leaf.truncated, "fence", leaf.fence, info)
    assert info["l2_records"] == leaf.complete + leaf.truncated + leaf.fence
    assert info["l2_max_leaf"] == max(leaf.complete, leaf.truncated, leaf.fence)
    return info


# ---------------------------------------------------------------------------- the complete stream

@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3 * 1024 + 1])
def test_complete_stream_of_n_records(ctx, n):
    """lanes past the end, zero, one and two trips of the scan's main loop, the peeled tail.  (A job this small sizes its
    fixed-stride streams for ~96 records; beyond that the streams are laid out exactly -- the assertion at the end says
    which layout ran.)"""
    rng = np.random.default_rng(9000 + n)
    genome, pos = fenced_genome(rng, mmer_len(31), 42)
    leaf = Leaf(genome, pos, mmer_len(31))
    c, js = 7, len(pos) - 2 - 7 + 1
    for i in range(n // c):
        leaf.span(1 + i % js, c)
    if n % c:
        leaf.span(1 + (n // c) % js, n % c)
    assert leaf.complete == n and (n < 8 or leaf.truncated < n)
    info = run_leaf(ctx, leaf)
    if n >= 8:
        assert info["l2_max_leaf"] == n
    assert (info["l2_max_leaf"] <= info["l2_cap"]) == (n <= 65)


def test_complete_stream_empty_truncated_stream_not(ctx):
    """a few reads that hold one occurrence each: nothing of the EMPTY complete stream may be counted, and the hoisted
    loads find their records with no complete run beside them"""
    rng = np.random.default_rng(9200)
    genome, pos = fenced_genome(rng, mmer_len(31), 12)
    leaf = Leaf(genome, pos, mmer_len(31))
    for j in (1, 2, 3, 5, 8):
        leaf.lone(j)
    assert leaf.complete == 0 and leaf.truncated == 5
    run_leaf(ctx, leaf)


# ---------------------------------------------------------------------------- the truncated stream: the hoisted loads

@pytest.mark.parametrize("t", [0, 1, 1023, 1024, 1025, TL_CAP - 1, TL_CAP, TL_CAP + 1, 6001])
def test_truncated_stream_of_t_records(ctx, t):
    """>= 300 complete records beside them; the truncated records have twins but (t odd) one: the clamp of the hoisted
    loads at the stream's last record, all four slots of a thread, and the tail beyond the list.  t = 0: every read ends
    on the fence"""
    rng = np.random.default_rng(9300 + t)
    m = mmer_len(31)
    if t == 0:
        genome, pos = fenced_genome(rng, m, 9)                   # one read shape: fence, seven occurrences, fence
        leaf = Leaf(genome, pos, m)
        for _ in range(50):
            leaf.span(1, 7)
        assert leaf.complete == 350 and leaf.truncated == 0 and leaf.fence == 100
    else:
        genome, pos = fenced_genome(rng, m, 62)
        leaf = Leaf(genome, pos, m)
        leaf.cover(7)                                            # 54 reads: 378 complete, 106 truncated
        if t < leaf.truncated:                                   # (t = 1: one lone read beside reads that end on the fence)
            leaf = Leaf(genome, pos, m)
            g9, p9 = fenced_genome(rng, m, 9)
            leaf9 = Leaf(g9, p9, m)
            for _ in range(50):
                leaf9.span(1, 7)
            leaf.reads, leaf.complete, leaf.fence = leaf9.reads, leaf9.complete, leaf9.fence
        j = 0
        while leaf.truncated + 2 <= t:                           # span reads of one complete record, inner occurrences only
            leaf.span(2 + j % (len(pos) - 4), 1)
            j += 1
        if leaf.truncated < t:
            leaf.lone(3)
        assert leaf.truncated == t and leaf.complete >= 300
    run_leaf(ctx, leaf)


@pytest.mark.parametrize("lone", [1, 40, 80])
def test_truncated_stream_on_the_fixed_stride_layout(ctx, lone):
    """the layout the benchmark runs (the truncated stream behind the complete one in the leaf's own stride): a job this
    small has room for ~96 records per stream, so 42 complete records and 10 + `lone` truncated ones stay where the
    first sizing put them -- asserted -- and the hoisted loads read them there"""
    rng = np.random.default_rng(9350 + lone)
    m = mmer_len(31)
    genome, pos = fenced_genome(rng, m, 14)
    leaf = Leaf(genome, pos, m)
    leaf.cover(7)
    for i in range(lone):
        leaf.lone(1 + i % (len(pos) - 2))
    assert leaf.complete == 42 and leaf.truncated == 10 + lone
    info = run_leaf(ctx, leaf)
    assert info["l2_max_leaf"] <= info["l2_cap"]                  # nothing was laid out again


# ---------------------------------------------------------------------------- truncated runs without a twin

@pytest.mark.parametrize("f", [0, 1, 64, 65, FL_CAP, FL_CAP + 1])
def test_twinless_truncated_runs(ctx, f):
    """f lone reads beside a leaf whose other truncated records all have twins: the list of the twinless (flist), and
    beyond FL_CAP the length-sorted list of all truncated records (tlist) with anchoring off.  (Which list a leaf took is
    not reported by msp_info(): that FL_CAP + 1 switches anchoring off rests on the construction -- lone reads are cut
    on both sides and are never looked up, the span reads' ends all find their twin -- and the case checks the counts
    either way.)"""
    rng = np.random.default_rng(9400 + f)
    m = mmer_len(31)
    genome, pos = fenced_genome(rng, m, 62)
    leaf = Leaf(genome, pos, m)
    leaf.cover(7)
    for i in range(f):
        leaf.lone(1 + i % (len(pos) - 2))
    assert leaf.complete >= 300 and leaf.truncated == 106 + f
    run_leaf(ctx, leaf)


# ---------------------------------------------------------------------------- the exact layout and the other paths

def test_exact_layout(ctx):
    """3000 reads of a 300-run genome: the leaf's streams overflow the first sizing by far and are laid out again back
    to back -- the scan asks for its first records at its start there, as before"""
    import cfrk_amd
    k, flags = 31, cfrk_amd.CFRK_CANONICAL
    rng = np.random.default_rng(9500)
    genome, pos = planted_genome(rng, mmer_len(k), 150)
    data, _, _ = refsem.flatten(sample_reads(rng, genome, 3000))
    info = same_result(count_partitioned(ctx, data, k, flags), expect_hash(ctx, data, k, True))
    print(info)
    assert info["l2_max_leaf"] >= 5 * 3000 and info["l2_max_leaf"] > info["l2_cap"]      # no fixed stride holds it


@pytest.mark.parametrize("k,canonical,nreads,dbg", [(31, True, 800, 1), (27, True, 1400, 0), (31, False, 800, 0),
                                                     (28, True, 800, 0), (32, True, 800, 0)],
                         ids=["rt_overflow", "k27_pool_table", "forward", "k28", "k32"])
def test_other_paths_share_the_moved_code(ctx, k, canonical, nreads, dbg):
    """CFRK_DEBUG_FORCE_RT_OVERFLOW (the rare path asks for the truncated records again), k = 27 (the pool-wide table),
    forward-strand counting, k = 28 and k = 32: one mid-size leaf each"""
    import cfrk_amd
    assert cfrk_amd.CFRK_DEBUG_FORCE_RT_OVERFLOW == 1
    flags = cfrk_amd.CFRK_CANONICAL if canonical else 0
    rng = np.random.default_rng(9600 + 10 * k + canonical + dbg)
    genome, pos = planted_genome(rng, mmer_len(k), 150)
    data, _, _ = refsem.flatten(sample_reads(rng, genome, nreads))
    info = same_result(count_partitioned(ctx, data, k, flags, dbg=dbg), expect_hash(ctx, data, k, canonical))
    print("k", k, info)
    assert info["l2_max_leaf"] >= 5 * nreads
    if k == 27:
        assert info["l2_max_leaf"] >= BT_MIN_RUNS


# ---------------------------------------------------------------------------- the copy-out

def _leaf_export(ctx, g):
    """export_leaves_device with one owner -> (keys, counts, per-leaf counts) in leaf order"""
    n = g.finish()
    lpp = g.leaves_per_part(1)
    dk, dc, dl = ctx.alloc(n * 8 + 8), ctx.alloc(n * 4 + 4), ctx.alloc(lpp * 4)
    try:
        pc = g.export_leaves_device(dk, dc, n, 1, dl, 0)
        keys, cnt, lc = np.empty(n, np.uint64), np.empty(n, np.uint32), np.empty(lpp, np.uint32)
        ctx.d2h(keys, dk); ctx.d2h(cnt, dc); ctx.d2h(lc, dl)
    finally:
        ctx.free(dk); ctx.free(dc); ctx.free(dl)
    return n, pc, keys, cnt, lc


def test_copy_out_ranks_and_leaf_index(ctx):
    """the 1024-record leaf: the export equals the hash path's key for key (run_leaf), and the per-leaf index -- offset and
    count of every leaf's segment, written by the wave that asks the cursor -- tiles [0, distinct): gathered leaf by leaf
    through it, every key appears once with its count, none is missing"""
    import cfrk_amd
    k, flags = 31, cfrk_amd.CFRK_CANONICAL
    rng = np.random.default_rng(9700)
    genome, pos = fenced_genome(rng, mmer_len(k), 42)
    leaf = Leaf(genome, pos, mmer_len(k))
    js = len(pos) - 2 - 7 + 1
    for i in range(146):
        leaf.span(1 + i % js, 7)
    leaf.span(1, 2)
    assert leaf.complete == 1024
    run_leaf(ctx, leaf)
    data = leaf.data()
    _, (wlo, _, wcnt) = expect_hash(ctx, data, k, True)
    g = count_partitioned(ctx, data, k, flags)
    n, pc, keys, cnt, lc = _leaf_export(ctx, g)
    assert n == len(wlo) and pc == [n] and int(lc.astype(np.uint64).sum()) == n
    assert int((lc > 0).sum()) >= 2                                # the planted leaf, the fence's, and a few strays
    order = np.argsort(keys, kind="stable")
    assert (keys[order] == wlo).all() and (cnt[order] == wcnt).all()
