"""GPU: reads threaded through the unitig graph (cfrk_global_read_paths and its device form) against
tests/read_paths_ref.py, a lists-and-tuples statement of the contract that shares nothing with the product.  Host and
device form are held to the reference for equality of path_ptr, paths, support and stats: on the unitig tests' k grid,
both strand rules and two thresholds with the library's own hits and links; and on crafted hit sets at the smallest shapes
at which the kernels can go wrong -- rows that start on either side of a workgroup, a path across three workgroups, the
scan's tile seams, empty rows, one-hit reads, nothing at all; ends one k-mer short and window gaps; circles, hairpins, a
homopolymer node, palindromes, a job that is not canonical; a sub-CSR; one hot link; one read of 10^5 hits among 10^4 short
ones; the capacity protocol, skewed outputs, the digest and the state rule; every refusal; the CLI."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from . import read_hits_ref as hr
from . import read_paths_ref as pr
from . import tips_ref as tr
from . import unitig_links_ref as ulr
from . import unitig_ref as ur
from .test_gpu_filter import _Guarded, _upload
from .test_gpu_query import _cli
from .test_gpu_read_hits import _graph
from .test_gpu_unitigs import KS, _input, _job, _rand, _table

pytestmark = pytest.mark.gpu

CFRK_ERR_ARG, CFRK_ERR_STATE, CFRK_ERR_LAYOUT, CFRK_ERR_SMALL_BUF = -1, -4, -5, -9
FROM_MINUS, TO_MINUS = 1, 2


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def jobs(ctx):
    """a job per strand rule: the call reads nothing of it but the rule"""
    import cfrk_amd
    out = {}
    for canonical in (False, True):
        g = cfrk_amd.GlobalCounter(ctx, 5, cfrk_amd.CFRK_CANONICAL if canonical else 0, 1000)
        g.add(*hr.read_codes(["ACGTTGCAAC"]))
        out[canonical] = g
    return out


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if not (got == want).all():
        i = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{what}: {int((got != want).sum())} differ, the first at {i}: {got[i]} against {want[i]}")


def _rec(n_kmers):
    import cfrk_amd
    rec = np.zeros(len(n_kmers), cfrk_amd.UNITIG_DTYPE)
    rec["n_kmers"] = n_kmers
    rec["kc"] = rec["n_kmers"]
    return rec


class _Dev:
    """the inputs on the device, hits 4 bytes off a 64-byte boundary; outputs behind guards, skewed"""

    def __init__(self, ctx, hit_ptr, hits, rec, link_ptr, links, support=None):
        self.ctx, self.nR, self.n_hits, self.nS, self.n_links = ctx, len(hit_ptr) - 1, len(hits), len(rec), len(links)
        self.up = [_upload(ctx, hit_ptr), _upload(ctx, hits, 4), _upload(ctx, rec), _upload(ctx, link_ptr), _upload(ctx, links)]
        self.d_ptr = _Guarded(ctx, (self.nR + 1) * 8, 8)
        self.d_sup = _Guarded(ctx, self.n_links * 4, 4)
        if self.n_links:
            ctx.h2d(self.d_sup.ptr, np.zeros(self.n_links, np.uint32) if support is None else np.ascontiguousarray(support, np.uint32))
        self.d_paths = None

    def call(self, g, d_paths, cap, with_support=True):
        u = self.up
        return g.read_paths_device(u[0], self.nR, u[1] + 4, self.n_hits, u[2], self.nS, u[3], u[4], self.n_links, self.d_ptr.ptr, d_paths, cap,
                                   self.d_sup.ptr if with_support else 0)

    def path_ptr(self):
        return self.d_ptr.fetch((self.nR + 1) * 8, np.int64)

    def support(self):
        return self.d_sup.fetch(self.n_links * 4, np.uint32)

    def free(self):
        for p in self.up:
            self.ctx.free(p)
        for b in (self.d_ptr, self.d_sup, self.d_paths):
            if b is not None:
                b.free()


def _device(ctx, g, hit_ptr, hits, rec, link_ptr, links, support=None):
    """the device form: a sizes-only call without support, then exact capacity -> (path_ptr, paths, support, stats)"""
    import cfrk_amd
    d = _Dev(ctx, hit_ptr, hits, rec, link_ptr, links, support)
    try:
        try:
            n, st = d.call(g, 0, 0, with_support=False)
            assert n == 0
        except cfrk_amd.CfrkError as e:
            assert e.code == CFRK_ERR_SMALL_BUF
            n, st = e.n_paths, e.stats
        ptr = d.path_ptr()
        assert ptr[0] == 0 and ptr[-1] == n == st["n_paths"]
        d.d_paths = _Guarded(ctx, n * 16, 4)
        assert d.call(g, d.d_paths.ptr, n) == (n, st)
        ctx.sync()
        _same(d.path_ptr(), ptr, "path_ptr of the second call")
        return ptr, d.d_paths.fetch(n * 16, pr.READ_PATH_DTYPE), d.support(), st
    finally:
        d.free()


def _check(ctx, g, hit_ptr, hits, rec, link_ptr, links, support=None, what=""):
    """host form and device form against the reference -> the reference's (path_ptr, paths, support, stats)"""
    hit_ptr, hits = np.ascontiguousarray(hit_ptr, np.int64), np.ascontiguousarray(hits, hr.READ_HIT_DTYPE)
    link_ptr, links = np.ascontiguousarray(link_ptr, np.int64), np.ascontiguousarray(links, ulr.UNITIG_LINK_DTYPE)
    want = pr.path_rows(hit_ptr, hits, [int(x) for x in rec["n_kmers"]], link_ptr, links, support)
    for form, got in (("host", g.read_paths(hit_ptr, hits, rec, link_ptr, links, None if support is None else support.copy())),
                      ("device", _device(ctx, g, hit_ptr, hits, rec, link_ptr, links, support))):
        for name, a, b in zip(("path_ptr", "paths", "support"), got, want):
            _same(a, b, f"{what} {name}, {form} form")
        assert got[3] == want[3], (what, form, got[3], want[3])
    return want


def _hit_rows(rows):
    """[[hit, ...] per read] -> (hit_ptr, hits)"""
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return ptr, np.array([h for r in rows for h in r], hr.READ_HIT_DTYPE).reshape(-1)


# ------------------------------------------------------------------ the grid: the library's own hits and links

def _walks(G, seqs, k):
    """walks through the graph: the input and its reverse complements, every circle 2.5 times round, an N and a
    substitution planted in the genome, pieces, short reads"""
    strings = [s for s, _ in seqs]
    reads = strings + [ur.rc(s) for s in strings]
    reads += [s + (s[k - 1:] * 2)[:n + n // 2] for s, _, n, circ in G.units if circ]
    g0 = strings[0]
    sub = ur.BASES[(ur.BASES.index(g0[700]) + 1) % 4]
    reads += [g0[:1500] + "N" + g0[1501:], g0[:700] + sub + g0[701:1400], g0[100:100 + 3 * k], g0[:k - 1], ""]
    return reads


def _end_to_end(ctx, seqs, k, canonical, min_count, reads, G=None):
    """count, unitigs, links, index and hits by the product (each held to its reference), then the paths"""
    table = _table(seqs, k, canonical)
    G = G or hr.Graph(table, k, canonical, min_count)
    g = _job(ctx, seqs, k, canonical)
    digest = g.digest()
    udata, ustart, ulength, rec = ur.layout(G.units)
    g.unitig_index(udata, ustart, ulength, min_count)
    link_ptr, links = g.unitig_links(udata, ustart, ulength, min_count)
    w_ptr, w_links = ulr.links(G.units, table, k, canonical, min_count)
    _same(link_ptr, w_ptr, "link_ptr")
    assert links.tolist() == w_links.tolist()
    hit_ptr, hits = g.read_hits(*hr.read_codes(reads))
    ref = pr.graph_paths(G, w_ptr, w_links, reads)                    # (asserts the consequences)
    _same(hit_ptr, ref[0], "hit_ptr")
    _same(hits, ref[1], "hits")
    want = _check(ctx, g, hit_ptr, hits, rec, link_ptr, links, what=f"k={k}")
    assert want[3] == ref[5] and want[3]["n_unlinked"] == 0
    assert g.digest() == digest
    return g, G, rec, hit_ptr, hits, link_ptr, links, want


@pytest.mark.parametrize("min_count", [1, 2])
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", KS)
def test_paths_on_the_grid(ctx, k, canonical, min_count):
    seqs = _input(k)
    G = _graph(k, canonical, min_count)
    g, G, rec, hit_ptr, hits, link_ptr, links, want = _end_to_end(ctx, seqs, k, canonical, min_count, _walks(G, seqs, k), G)
    assert want[3]["n_paths"] >= len(seqs) and want[3]["n_gaps"] >= 1 and (want[3]["n_steps"] > 10 or min_count == 2)
    # the same reads with every third link row removed: they break there and nowhere else
    keep = np.ones(len(links), bool)
    keep[::3] = False
    sub_ptr = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)[link_ptr]
    sub = _check(ctx, g, hit_ptr, hits, rec, sub_ptr, links[keep], what="sub-CSR")
    assert (sub[2] == want[2][keep]).all() and sub[3]["n_unlinked"] == int(want[2][~keep].sum())
    assert sub[3]["n_paths"] == want[3]["n_paths"] + sub[3]["n_unlinked"]


# ------------------------------------------------------------------ special links

FORK = [("GAAGAGTC", 1), ("AGTCATT", 1), ("AGTCCAA", 1)]
WALK_A, WALK_B = "GAAGAGTCATT", "GAAGAGTCCAA"


@pytest.mark.parametrize("canonical", [False, True])
def test_fork_hand_worked(ctx, canonical):
    reads = [WALK_A, ur.rc(WALK_B), WALK_B, ur.rc(WALK_A), "GAAGANTCATT"]
    want = _end_to_end(ctx, FORK, 5, canonical, 1, reads)[-1]
    if canonical:
        assert want[1].tolist() == [(0, 2, 0, 7)] * 4 + [(0, 1, 0, 1), (1, 1, 6, 1)] and want[2].tolist() == [1, 1, 1, 1]
        assert want[3] == {"n_paths": 6, "n_steps": 4, "n_gaps": 1, "n_unlinked": 0}
    else:
        assert want[0].tolist() == [0, 1, 1, 2, 2, 4] and want[2].tolist() == [1, 1]


@pytest.mark.parametrize("canonical", [False, True])
def test_circle_once_and_two_and_a_half_times_round(ctx, canonical):
    rng = np.random.default_rng(31)
    c = _rand(rng, 40)
    k = 9
    G = hr.Graph(_table([(c + c[:k - 1], 1)], k, canonical), k, canonical)
    (s, _, n, circ), = G.units
    assert circ and n == 40
    reads = [s + s[k - 1:2 * k], s + (s[k - 1:] * 2)[:n + n // 2], ur.rc(s + s[k - 1:2 * k]), s[3:] + s[k - 1:k + 5]]
    want = _end_to_end(ctx, [(c + c[:k - 1], 1)], k, canonical, 1, reads, G)[-1]
    assert want[1]["n_hits"].tolist()[:2] == [2, 3] and want[2][0] == 1 + 2 + 1            # the self-link (0,+) -> (0,+)


def test_hairpin_homopolymer_and_palindromes(ctx):
    h = "AACGT"
    want = _end_to_end(ctx, [(h + ur.rc(h), 1)], 5, True, 1, [h + ur.rc(h)])[-1]
    assert want[1].tolist() == [(0, 4, 0, 6)] and want[2].tolist() == [1, 0, 1, 0, 1]
    # a homopolymer node repeated: every window is the same single-node unitig, joined through its self-link
    for canonical in (False, True):
        want = _end_to_end(ctx, [("CC" + "A" * 12 + "GG", 1)], 4, canonical, 1, ["A" * 12, "T" * 9, "CC" + "A" * 12 + "GG"])[-1]
        assert want[1]["n_hits"].tolist()[0] == 9 and want[1]["n_windows"].tolist()[0] == 9 and want[3]["n_gaps"] == 0
    # palindromes at k = 4 and k = 32: entered and left as (v,+) by a read and by its reverse complement
    want = _end_to_end(ctx, [("TTACGTCC", 1)], 4, True, 1, ["TTACGTCC", "GGACGTAA"])[-1]
    assert want[1].tolist() == [(0, 3, 0, 5)] * 2 and want[2].tolist() == [1, 1, 0, 0, 1, 0, 1, 0]
    rng = np.random.default_rng(32)
    half = _rand(rng, 16)
    s = _rand(rng, 20) + half + ur.rc(half) + _rand(rng, 20)
    want = _end_to_end(ctx, [(s, 1)], 32, True, 1, [s, ur.rc(s)])[-1]
    assert want[1]["n_hits"].tolist() == [3, 3] and want[1]["n_windows"].tolist() == [len(s) - 31] * 2


# ------------------------------------------------------------------ ends, crafted by editing the hits

def test_short_of_the_end_is_unlinked_and_a_window_gap_is_a_gap(ctx, jobs):
    # the canonical fork: unitig 2 (4 k-mers) leaves through (2,+) -> (0,-); WALK_A is hits (2,+) 0..3 and (0,-) 2..0
    rec = _rec([3, 3, 4])
    link_ptr, links = np.array([0, 1, 2, 4]), np.array([(2, 2), (2, 3), (0, 2), (1, 0)], ulr.UNITIG_LINK_DTYPE)
    good = [(2, 0, 0, 4), (0, 1, 4, 3)]
    rows = [good,
            [(2, 0, 0, 3), (0, 1, 3, 3)],                       # stops one k-mer short of the end, window-adjacent
            [(2, 0, 0, 4), (0, 1, 5, 3)],                       # a window gap between two hits that would join
            [(2, 0, 0, 4), (0, 2 << 1 | 1, 4, 1)],              # enters (0,-) at its head: joined
            [(2, 0, 0, 4), (0, 1 << 1 | 1, 4, 1)],              # enters one k-mer behind the head
            [(2, 0, 0, 4), (0, 0, 4, 3)],                       # the other strand of the target: no such link
            [(2, 1, 0, 4), (0, 1, 4, 3)]]                       # the other strand of the source
    want = _check(ctx, jobs[True], *_hit_rows(rows), rec, link_ptr, links)
    assert np.diff(want[0]).tolist() == [1, 2, 2, 1, 2, 2, 2]
    assert want[3] == {"n_paths": 12, "n_steps": 2, "n_gaps": 1, "n_unlinked": 4} and want[2].tolist() == [0, 0, 2, 0]
    # in a job that is not canonical a strand bit on a hit finds no link
    plain = np.array([(0, 0), (1, 0)], ulr.UNITIG_LINK_DTYPE)
    want = _check(ctx, jobs[False], *_hit_rows([[(2, 0, 0, 4), (0, 0, 4, 3)], [(2, 0, 0, 4), (1, 1, 4, 3)]]), rec, np.array([0, 0, 0, 2]), plain)
    assert want[3] == {"n_paths": 3, "n_steps": 1, "n_gaps": 0, "n_unlinked": 1}


# ------------------------------------------------------------------ seams and rows, on a chain of single-node unitigs

CHAIN = 600


def _chain(canonical):
    """unitig j -> j + 1 for j < CHAIN - 1, every unitig one k-mer; canonical: with the mirrors, so rows of two"""
    rows = [[(j + 1, 0)] if j + 1 < CHAIN else [] for j in range(CHAIN)]
    if canonical:
        for j in range(1, CHAIN):
            rows[j].append((j - 1, FROM_MINUS | TO_MINUS))
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return _rec([1] * CHAIN), ptr, np.array([x for r in rows for x in r], ulr.UNITIG_LINK_DTYPE)


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("filler", [0, 255, 256, 257, 1023])
def test_a_path_across_workgroups_behind_filler_reads(ctx, jobs, filler, canonical):
    """one read over the whole chain is one path of 600 hits, across two or three workgroups of 256 lanes, its row
    starting at hit 0, 255, 256, 257 or 1023 behind reads of one hit; canonical: also walked backwards"""
    rec, link_ptr, links = _chain(canonical)
    rows = [[(7, 0, 0, 1)] for _ in range(filler)] + [[(j, 0, j, 1) for j in range(CHAIN)]]
    if canonical:
        rows.append([(CHAIN - 1 - j, 1, j, 1) for j in range(CHAIN)])
    rows.append([(3, 0, 0, 1), (4, 0, 1, 1)])
    want = _check(ctx, jobs[canonical], *_hit_rows(rows), rec, link_ptr, links)
    assert want[1][filler].tolist() == (0, CHAIN, 0, CHAIN) and want[3]["n_steps"] == (2 if canonical else 1) * (CHAIN - 1) + 1
    assert want[3]["n_paths"] == len(rows)


def test_rows_empty_first_last_three_in_a_row_and_nothing(ctx, jobs):
    rec, link_ptr, links = _chain(False)
    one, two = [(5, 0, 0, 1)], [(5, 0, 2, 1), (6, 0, 3, 1)]
    for rows in ([[], one, two, []], [[], [], [], two, [], [], [], one], [one], [[]], [[], [], []], []):
        want = _check(ctx, jobs[False], *_hit_rows(rows), rec, link_ptr, links)
        assert np.diff(want[0]).tolist() == [1 if r else 0 for r in rows]
    # no unitigs and no links at all; hits behind hit_ptr[nR] belong to no read
    none = np.zeros(0, ulr.UNITIG_LINK_DTYPE)
    want = _check(ctx, jobs[True], *_hit_rows([[], []]), _rec([]), np.zeros(1, np.int64), none)
    assert want[0].tolist() == [0, 0, 0] and want[3]["n_paths"] == 0
    ptr, hits = _hit_rows([one, two])
    want = _check(ctx, jobs[False], ptr[:2], hits, rec, link_ptr, links)
    assert want[0].tolist() == [0, 1] and want[3] == {"n_paths": 1, "n_steps": 0, "n_gaps": 0, "n_unlinked": 0}


# ------------------------------------------------------------------ random walks: the scan's seams, balance

def _random_graph(rng, nS, canonical):
    """random checked rows (at most 4; strand bits only when canonical, else no unitig entered more than 4 times; no
    mirrors: any sub-CSR is accepted)"""
    rows, entered = [], [0] * nS
    for _ in range(nS):
        row = []
        for _ in range(int(rng.integers(0, 5))):
            to = int(rng.integers(0, nS))
            if canonical or entered[to] < 4:
                entered[to] += 1
                row.append((to, int(rng.integers(0, 4)) if canonical else 0))
        rows.append(row)
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return rows, ptr, np.array([x for r in rows for x in r], ulr.UNITIG_LINK_DTYPE).reshape(-1)


def _walk(rng, rows, n_kmers, n_hits):
    """a read of n_hits hits that follows links, with a gap, a teleport or a short end now and then"""
    nS = len(rows)
    j, m, at, out = int(rng.integers(0, nS)), 0, 0, []
    for i in range(n_hits):
        N = n_kmers[j]
        n = N if 0 < i < n_hits - 1 or rng.random() < 0.5 else int(rng.integers(1, N + 1))
        first = i == 0 or rng.random() < 0.03                   # a first hit ends at the end; else it begins at the head
        off = (0 if m else N - n) if first else (N - n if m else 0)
        out.append((j, off << 1 | m, at, n))
        at += n + (1 if rng.random() < 0.03 else 0)
        nxt = [(to, f) for to, f in rows[j] if (f & FROM_MINUS) == m]
        if nxt and rng.random() < 0.95:
            j, f = nxt[int(rng.integers(0, len(nxt)))]
            m = 1 if f & TO_MINUS else 0
        else:
            j, m = int(rng.integers(0, nS)), 0
    return out


def _random_case(rng, nS, canonical, hit_counts):
    rows, link_ptr, links = _random_graph(rng, nS, canonical)
    n_kmers = [int(x) for x in rng.integers(1, 6, nS)]
    return _hit_rows([_walk(rng, rows, n_kmers, n) for n in hit_counts]) + (_rec(n_kmers), link_ptr, links)


def test_scan_tile_seams(ctx, jobs):
    """n_hits + 1 scanned flags on either side of the scan's tile.  rocPRIM has no tuned scan entry for gfx950, so a scan of
    32-bit values takes its untuned shape, 256 lanes x 16 items = 4096 per block (`default_scan_config_base`): every size
    from 8 below to 8 above one and two tiles; and, should another shape be chosen, either side of 256 lanes x the items
    its tuned tables hold for integers (15, 21, 24) and the powers of two around them.  The paths lie across the seams"""
    rng = np.random.default_rng(77)
    sizes = set(range(4096 - 9, 4096 + 8)) | set(range(8192 - 9, 8192 + 8))
    for t in (256 * i for i in (1, 2, 4, 8, 12, 15, 21, 24, 32)):
        sizes |= {t - 2, t - 1, t, t + 1}
    for n in sorted(sizes):
        canonical = bool(n & 1)
        counts = [int(x) for x in rng.integers(0, 40, n // 20)]
        counts.append(n - sum(counts))
        want = _check(ctx, jobs[canonical], *_random_case(rng, 50, canonical, counts), what=f"n_hits={n}")
        assert want[0][-1] == want[3]["n_paths"] and want[3]["n_steps"] > n // 5, want[3]


def test_one_read_of_a_hundred_thousand_hits_among_ten_thousand_short_ones(ctx, jobs):
    rng = np.random.default_rng(78)
    counts = [int(x) for x in rng.integers(0, 6, 10000)]
    counts[4321] = 100000
    case = _random_case(rng, 3000, True, counts)
    want = _check(ctx, jobs[True], *case)
    long_paths = want[1][want[0][4321]:want[0][4322]]
    assert long_paths["n_hits"].sum() == 100000 and long_paths["n_hits"].max() > 10 and want[3]["n_steps"] > 30000, (long_paths["n_hits"].max(), want[3])


def test_hot_link(ctx, jobs):
    """20 000 identical reads across one link: every step adds to one counter; a second call adds again"""
    rec, link_ptr, links = _rec([3, 3, 4]), np.array([0, 1, 2, 4]), np.array([(2, 2), (2, 3), (0, 2), (1, 0)], ulr.UNITIG_LINK_DTYPE)
    ptr, hits = _hit_rows([[(2, 0, 0, 4), (0, 1, 4, 3)]] * 20000)
    g = jobs[True]
    for form in ("host", "device"):
        first = g.read_paths(ptr, hits, rec, link_ptr, links) if form == "host" else _device(ctx, g, ptr, hits, rec, link_ptr, links)
        assert first[2].tolist() == [0, 0, 20000, 0] and first[3] == {"n_paths": 20000, "n_steps": 20000, "n_gaps": 0, "n_unlinked": 0}
        again = g.read_paths(ptr, hits, rec, link_ptr, links, first[2]) if form == "host" else _device(ctx, g, ptr, hits, rec, link_ptr, links, first[2])
        assert again[2].tolist() == [0, 0, 40000, 0]
        assert (first[1]["n_hits"] == 2).all() and (first[1]["n_windows"] == 7).all() and first[0].tolist() == list(range(20001))


# ------------------------------------------------------------------ capacity, state, arguments

def test_capacity_protocol_digest_and_arguments(ctx, jobs):
    import cfrk_amd
    rng = np.random.default_rng(79)
    g = jobs[True]
    digest = g.digest()
    hit_ptr, hits, rec, link_ptr, links = _random_case(rng, 40, True, [int(x) for x in rng.integers(0, 30, 200)])
    want = pr.path_rows(hit_ptr, hits, [int(x) for x in rec["n_kmers"]], link_ptr, links)
    n = int(want[3]["n_paths"])
    d = _Dev(ctx, hit_ptr, hits, rec, link_ptr, links)
    # one row too few: path_ptr, support and stats complete, nothing written to paths
    d.d_paths = _Guarded(ctx, n * 16, 4)
    with pytest.raises(cfrk_amd.CfrkError) as e:
        d.call(g, d.d_paths.ptr, n - 1)
    assert e.value.code == CFRK_ERR_SMALL_BUF and e.value.n_paths == n and e.value.stats == want[3]
    assert len(d.d_paths.fetch(0)) == 0                              # (every byte still the guard's)
    _same(d.path_ptr(), want[0], "path_ptr of a call that did not fit")
    _same(d.support(), want[2], "support of a call that did not fit")
    # a roomy array: the rows, and nothing behind them
    d.d_paths.free()
    d.d_paths = _Guarded(ctx, (n + 9) * 16, 12)
    assert d.call(g, d.d_paths.ptr, n + 9, with_support=False) == (n, want[3])
    ctx.sync()
    _same(d.d_paths.fetch(n * 16, pr.READ_PATH_DTYPE), want[1], "paths in a roomy array")
    _same(d.support(), want[2], "support of a call without it")
    d.free()
    assert g.digest() == digest
    # the CFRK_ERR_ARG cases
    L, h = ctx._L, ctx._h
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    links = np.ascontiguousarray(links)
    nR, nH, nS, nL = len(hit_ptr) - 1, len(hits), len(rec), len(links)
    ptr, got_n, st = np.zeros(nR + 1, np.int64), C.c_int64(), np.zeros(4, np.uint64)
    ok = [h, vp(hit_ptr), nR, vp(hits), nH, vp(rec), nS, vp(link_ptr), vp(links), nL, vp(ptr), None, 0, C.byref(got_n), None, vp(st)]

    def with_(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return a
    assert L.cfrk_global_read_paths(*ok) == CFRK_ERR_SMALL_BUF and got_n.value == n
    for bad in (with_(_2=-1), with_(_4=-1), with_(_6=-1), with_(_9=-1), with_(_1=None), with_(_3=None), with_(_5=None), with_(_7=None),
                with_(_8=None), with_(_10=None), with_(_12=5), with_(_13=None), with_(_15=None), with_(_6=1 << 32), with_(_4=1 << 32)):
        assert L.cfrk_global_read_paths(*bad) == CFRK_ERR_ARG
        assert L.cfrk_global_read_paths_device(*bad) == CFRK_ERR_ARG


def test_need_a_job():
    import cfrk_amd
    with cfrk_amd.Context(0) as c:
        z, n = np.zeros(4, np.int64), C.c_int64()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        for fn in (c._L.cfrk_global_read_paths, c._L.cfrk_global_read_paths_device):
            assert fn(c._h, vp(z), 0, None, 0, None, 0, None, None, 0, vp(z), None, 0, C.byref(n), None, vp(z)) == CFRK_ERR_STATE


# ------------------------------------------------------------------ refusals

def _refused(ctx, g, hit_ptr, hits, rec, link_ptr, links, who, number, words):
    """both forms refuse with CFRK_ERR_LAYOUT naming `who` `number`; no byte outside the guards is written, path_ptr is
    all 0 and support is what it was"""
    import cfrk_amd
    hit_ptr, hits = np.ascontiguousarray(hit_ptr, np.int64), np.ascontiguousarray(hits, hr.READ_HIT_DTYPE)
    link_ptr, links = np.ascontiguousarray(link_ptr, np.int64), np.ascontiguousarray(links, ulr.UNITIG_LINK_DTYPE)
    before = np.arange(7, 7 + len(links), dtype=np.uint32)
    d = _Dev(ctx, hit_ptr, hits, rec, link_ptr, links, before)
    d.d_paths = _Guarded(ctx, max(len(hits), 1) * 16, 4)
    with pytest.raises(cfrk_amd.CfrkError) as e:
        d.call(g, d.d_paths.ptr, len(hits))
    assert e.value.code == CFRK_ERR_LAYOUT and e.value.n_paths == 0 and not any(e.value.stats.values())
    m = re.search(r"(read|unitig) (\d+) ", str(e.value))
    assert m and (m.group(1), int(m.group(2))) == (who, number) and words in str(e.value), str(e.value)
    assert len(d.d_paths.fetch(0)) == 0 and not d.path_ptr().any()
    _same(d.support(), before, "support after a refusal")
    d.free()
    sup = before.copy()
    with pytest.raises(cfrk_amd.CfrkError) as e2:
        g.read_paths(hit_ptr, hits, rec, link_ptr, links, sup)
    assert e2.value.code == CFRK_ERR_LAYOUT and str(e2.value).split(": ", 1)[1] == str(e.value).split(": ", 1)[1]
    assert (sup == before).all()


@pytest.mark.parametrize("canonical", [False, True])
def test_refusals(ctx, jobs, canonical):
    rng = np.random.default_rng(80 + canonical)
    g = jobs[canonical]
    hit_ptr, hits, rec, link_ptr, links = _random_case(rng, 60, canonical, [int(x) for x in rng.integers(1, 9, 700)])
    nS, nH = len(rec), len(hits)
    a = (rec, link_ptr, links)

    def ptr_with(i, v):
        p = hit_ptr.copy()
        p[i] = v
        return p

    def hits_with(h, **kw):
        x = hits.copy()
        for f, v in kw.items():
            x[f][h] = v
        return x
    read_of = lambda h: int(np.searchsorted(hit_ptr, h, side="right")) - 1
    _refused(ctx, g, ptr_with(300, hit_ptr[299] - 1), hits, *a, "read", 299, "hit_ptr")           # descending
    _refused(ctx, g, ptr_with(len(hit_ptr) - 1, nH + 1), hits, *a, "read", len(hit_ptr) - 2, "hit_ptr")     # past n_hits
    _refused(ctx, g, ptr_with(0, 1), hits, *a, "read", 0, "hit_ptr")
    _refused(ctx, g, ptr_with(511, -3), hits, *a, "read", 510, "hit_ptr")
    h = int(hit_ptr[400]) + 1
    _refused(ctx, g, hit_ptr, hits_with(h, unitig=nS), *a, "read", read_of(h), "not in the list")
    _refused(ctx, g, hit_ptr, hits_with(h, n_windows=0), *a, "read", read_of(h), "no windows")
    j = int(hits["unitig"][h])
    _refused(ctx, g, hit_ptr, hits_with(h, unitig_at=(int(rec["n_kmers"][j]) << 1), n_windows=1), *a, "read", read_of(h), "past the end")
    _refused(ctx, g, hit_ptr, hits_with(h, unitig_at=0, n_windows=0xFFFFFFFF), *a, "read", read_of(h), "past the end")
    # two offenders: the first read is named; the last hit of all, and the first
    _refused(ctx, g, hit_ptr, hits_with([h, nH - 1, 0], n_windows=0), *a, "read", 0, "no windows")
    _refused(ctx, g, hit_ptr, hits_with(nH - 1, unitig=0xFFFFFFFF), *a, "read", len(hit_ptr) - 2, "not in the list")
    # a link row the shared check refuses wins over everything behind it
    bad = np.ascontiguousarray(links).copy()
    row = next(j for j in range(nS) if link_ptr[j + 1] > link_ptr[j] and j > 3)
    bad["to"][link_ptr[row]] = nS
    _refused(ctx, g, hit_ptr, hits_with(h, n_windows=0), rec, link_ptr, bad, "unitig", row, "not in the list")
    bad = np.ascontiguousarray(links).copy()
    bad["flags"][link_ptr[row]] = 4
    _refused(ctx, g, hit_ptr, hits, rec, link_ptr, bad, "unitig", row, "flag")
    lp = link_ptr.copy()
    assert lp[19] > 0
    lp[20] = lp[19] - 1
    _refused(ctx, g, hit_ptr, hits, rec, lp, links, "unitig", 19, "link_ptr")
    # wild tables: nothing outside the buffers is touched, the call returns
    wild = rng.integers(-2 ** 62, 2 ** 62, len(hit_ptr)).astype(np.int64)
    wild[0] = 0
    _refused(ctx, g, wild, hits, *a, "read", 0, "hit_ptr")
    wild_hits = rng.integers(0, 2 ** 32, (nH, 4), dtype=np.uint64).astype(np.uint32).view(hr.READ_HIT_DTYPE).reshape(-1)
    _refused(ctx, g, hit_ptr, wild_hits, *a, "read", 0, "")
    # and the right arrays are accepted afterwards
    _check(ctx, g, hit_ptr, hits, *a)


def test_the_first_offender_is_named_when_blocks_start_late(ctx, jobs):
    """more hits than one turn of the largest grid takes (16 workgroups of 256 lanes per compute unit, 256 units), so
    that workgroups start after others have finished: hit 1 100 000 is looked at by an early workgroup in its second
    turn, hit 600 000 by one that may start only after that.  Reads of one hit: the read is the hit"""
    n = 2_300_000
    assert n > 2 * 256 * 16 * 256
    hits = np.zeros(n, hr.READ_HIT_DTYPE)
    hits["n_windows"] = 1
    hits["n_windows"][[600_000, 1_100_000]] = 0
    hit_ptr = np.arange(n + 1, dtype=np.int64)
    links = np.array([(0, 0)], ulr.UNITIG_LINK_DTYPE)
    _refused(ctx, jobs[False], hit_ptr, hits, _rec([1]), np.array([0, 1]), links, "read", 600_000, "no windows")
    hits["unitig"][2_200_000] = 1
    _refused(ctx, jobs[True], hit_ptr, hits, _rec([1]), np.array([0, 1]), links, "read", 600_000, "no windows")


# ------------------------------------------------------------------ CLI

def _write_inputs(tmp_path, seqs, reads):
    fasta, q = tmp_path / "in.fa", tmp_path / "q.fq"
    with open(fasta, "w") as f:
        i = 0
        for s, t in seqs:
            for _ in range(t):
                f.write(">r%d\n%s\n" % (i, s))
                i += 1
    with open(q, "w") as f:
        for i, s in enumerate(reads):
            f.write("@q%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)))
    return fasta, q


@pytest.mark.parametrize("k,canonical,min_count", [(21, True, 1), (12, False, 1)])
def test_cli_paths_support_and_stats(tmp_path, k, canonical, min_count):
    seqs = _input(k)
    table = _table(seqs, k, canonical)
    G = _graph(k, canonical, min_count)
    reads = [r for r in _walks(G, seqs, k) if r]                  # (a FASTQ record has a sequence)
    fasta, q = _write_inputs(tmp_path, seqs, reads)
    tail = [str(k), "--global"] + (["--canonical"] if canonical else [])
    P = lambda name: str(tmp_path / name)
    read = lambda name: open(tmp_path / name, "rb").read()
    base = lambda t: ["--unitigs-gfa", P(t + ".gfa"), "--unitigs-map", str(q), "--unitigs-map-out", P(t + ".gaf"), "--unitigs-min-count", str(min_count)]
    new = lambda t: base(t) + ["--unitigs-map-paths", "--unitigs-link-support", "--unitigs-map-stats", P(t + ".tsv")]
    units, _, reduced = tr.clip(table, k, canonical, min_count, None, 512, rounds=4)
    for name, graph, clip in (("raw", G, []), ("clip", hr.Graph(reduced, k, canonical, min_count), ["--unitigs-clip-tips"])):
        assert graph.units == (units if clip else G.units)
        t = reduced if clip else table
        link_ptr, links = ulr.links(graph.units, t, k, canonical, min_count)
        hit_ptr, hits, path_ptr, paths, support, st = pr.graph_paths(graph, link_ptr, links, reads)
        subprocess.run([_cli(), str(fasta), P(name + ".out")] + tail + new(name) + clip, check=True, timeout=300)
        lens = [len(s) for s in graph.seqs]
        assert read(name + ".gaf") == pr.gaf_paths_text(lens, k, [len(r) for r in reads], hit_ptr, hits, path_ptr, paths)
        assert read(name + ".gfa") == pr.gfa_support_text(graph.units, k, link_ptr, links, support, canonical)
        assert read(name + ".tsv") == pr.stats_text(len(reads), len(hits), st)
        assert st["n_steps"] > 10 and st["n_unlinked"] == 0
        # without the three options every byte is what the parent commit's options write
        subprocess.run([_cli(), str(fasta), P(name + "0.out")] + tail + base(name + "0") + clip, check=True, timeout=300)
        assert read(name + "0.gaf") == graph.gaf_text(reads) and read(name + "0.gfa") == ulr.gfa_text(graph.units, k, link_ptr, links)
        assert read(name + "0.out") == read(name + ".out")
    # each option alone
    subprocess.run([_cli(), str(fasta), P("s.out")] + tail + base("s") + ["--unitigs-map-stats", P("s.tsv")], check=True, timeout=300)
    assert read("s.gaf") == read("raw0.gaf") and read("s.gfa") == read("raw0.gfa") and read("s.tsv") == read("raw.tsv")
    subprocess.run([_cli(), str(fasta), P("p.out")] + tail + base("p")[2:] + ["--unitigs-map-paths"], check=True, timeout=300)
    assert read("p.gaf") == read("raw.gaf") and not (tmp_path / "p.gfa").exists()
    subprocess.run([_cli(), str(fasta), P("l.out")] + tail + base("l") + ["--unitigs-link-support"], check=True, timeout=300)
    assert read("l.gaf") == read("raw0.gaf") and read("l.gfa") == read("raw.gfa")


@pytest.mark.parametrize("args, msg", [
    (["--unitigs-gfa", "g.gfa", "--unitigs-map-paths"], b"--unitigs-map-paths needs --unitigs-map QFILE"),
    (["--unitigs-map", "q.fa", "--unitigs-map-out", "m.gaf", "--unitigs-link-support"], b"--unitigs-link-support needs --unitigs-map QFILE and --unitigs-gfa GFILE"),
    (["--unitigs-out", "u.fa", "--unitigs-map-stats", "s.txt"], b"--unitigs-map-stats needs --unitigs-map QFILE"),
])
def test_cli_misuse_is_refused(tmp_path, args, msg):
    p = subprocess.run([_cli(), str(tmp_path / "missing.fasta"), str(tmp_path / "o.txt"), "15", "--global"] + args, cwd=tmp_path,
                       capture_output=True, timeout=60)
    assert p.returncode == 1 and msg in p.stderr and not list(tmp_path.iterdir())
