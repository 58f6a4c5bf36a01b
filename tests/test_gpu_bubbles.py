"""GPU: the bubble rule (cfrk_global_unitig_bubbles) in its device form and its host form against tests/bubbles_ref.py on
the k grid of the unitig tests under both strand rules; the simplify loop round for round on the reduced dictionary;
crafted rows it must refuse, hostile rows that pass the check, and a chain of 10^5 bubbles built as records and rows; the CLI."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from . import bubbles_ref as br
from . import tips_ref as tr
from . import unitig_links_ref as lr
from . import unitig_ref as ur
from .test_gpu_filter import _Guarded, _upload
from .test_gpu_query import _cli
from .test_gpu_tips import _other, _tip_input
from .test_gpu_unitig_links import _same_links
from .test_gpu_unitigs import KS, _job, _rand, _same, _table

pytestmark = pytest.mark.gpu

CFRK_ERR_ARG, CFRK_ERR_STATE, CFRK_ERR_LAYOUT = -1, -4, -5
NONE = 0xFFFFFFFF
# (max_kmers, max_diff, ratio_q8)
PARAMS = lambda k: [(k, 0, 0), (k, 1, 0), (k, 1, 512), (k, 1, 513), (0, 0, 0)]


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


# At k = 3 and 4 a random genome of any useful length holds nearly every k-mer and no path runs parallel to another for a
# whole unitig.  These inputs were picked by a seed search on the REFERENCE for graphs with at least three popped arms
# and an arm that stays at (max_kmers, max_diff, ratio_q8) = (k, 1, 0); they are data.  At k = 3 no input serves both
# strand rules, so each has its own; with both strands (32 nodes in all) the search found no graph with more than two
# popped arms (tests/test_bubbles_cpu.py says why), and the input has two.
_K4 = [("ACGGCAACGACAGTGTCATC", 4), ("CGGAAAC", 1), ("CGGGAAC", 2), ("CGGTAAC", 3), ("CAGAGTC", 3), ("CAGCGTC", 1), ("CAGTC", 1)]
_SMALL = {
    (3, False): [("CGTATGGCCCGAGCC", 4), ("GTCTG", 1), ("GTTG", 1), ("CCAAG", 2), ("CCCAG", 1), ("TGGG", 1)],
    (3, True): [("TGTGTGTT", 4), ("GTATG", 3), ("GTCTG", 3), ("GTTG", 1), ("TGTA", 1)],
    (4, False): _K4,
    (4, True): _K4,
}
_INPUTS = {}


def _bubble_input(k, canonical):
    """[(string, times counted)]: the tip input (a random genome of 3000 bases counted 4 times with its tips, its bubble, its
    circle and its hairpin) and, planted on the same genome between the tips: SNP arms counted once, 4 times (equal
    means: the index decides) and twice (popped at ratio_q8 512, kept at 513); a tri-allelic site; a one-base deletion
    and a one-base insertion (parallel at max_diff 1 only); an arm of k + 1 k-mers; two substitutions closer than k; an
    arm that carries a tip; a SNP on a circle of 3k k-mers"""
    if (k, canonical) in _SMALL:
        return _SMALL[(k, canonical)]
    if k in _INPUTS:
        return _INPUTS[k]
    seqs = list(_tip_input(k))
    G = seqs[0][0]
    L = len(G)
    rng = np.random.default_rng(9000 + 100 * k)
    taken = np.linspace(1, L - k - 2, 12)
    spots = iter(((taken[:-1] + taken[1:]) / 2).astype(int).tolist())       # half way between the tip input's spots
    snp = lambda a, x: G[a - k + 1:a] + x + G[a + 1:a + k]                  # the k k-mers that hold x at position a
    for times in (1, 4, 2):
        a = next(spots)
        seqs.append((snp(a, _other(rng, G[a])), times))
    a = next(spots)                                                         # three alleles
    x = _other(rng, G[a])
    y = next(c for c in ur.BASES if c not in (G[a], x))
    seqs += [(snp(a, x), 1), (snp(a, y), 2)]
    a = next(spots)                                                         # a deletion: k - 1 k-mers beside k
    seqs.append((G[a - k + 1:a] + G[a + 1:a + k], 1))
    a = next(spots)                                                         # an insertion: k k-mers beside k - 1
    seqs.append((G[a - k + 1:a] + _other(rng, G[a]) + G[a:a + k - 1], 1))
    a = next(spots)                                                         # one base replaced by two: k + 1 k-mers
    x, y = _other(rng, G[a]), _other(rng, G[a])                             # (neither is G[a]: no mere insertion)
    seqs.append((G[a - k + 1:a] + x + y + G[a + 1:a + k], 1))
    a = next(spots)                                                         # two substitutions k // 2 apart, and the first alone
    d = max(1, k // 2)
    x, y = _other(rng, G[a]), _other(rng, G[a + d])
    seqs.append((G[a - k + 1:a] + x + G[a + 1:a + d] + y + G[a + d + 1:a + d + k], 1))
    seqs.append((snp(a, x), 1))
    a = next(spots)                                                         # an arm that carries a tip
    arm = snp(a, _other(rng, G[a]))
    seqs.append((arm, 1))
    m = k + k // 2
    seqs.append((arm[m - k:m] + _other(rng, arm[m]) + _rand(rng, 2), 1))
    c = _rand(rng, 3 * k)                                                   # a SNP on a circle
    seqs.append((c + c[:k - 1], 2))
    b = k + k // 2
    seqs.append((c[b - k + 1:b] + _other(rng, c[b]) + c[b + 1:b + k], 1))
    _INPUTS[k] = seqs
    return seqs


_REF = {}


def _ref(k, canonical):
    """(table, units, link_ptr, links) of the planted input, computed once"""
    key = (k, canonical)
    if key not in _REF:
        table = _table(_bubble_input(k, canonical), k, canonical)
        _REF[key] = (table,) + tr.graph(table, k, canonical, 1)
    return _REF[key]


_WANT = {}


def _want(k, canonical, params):
    key = (k, canonical, params)
    if key not in _WANT:
        _, units, link_ptr, links = _ref(k, canonical)
        _WANT[key] = br.bubbles(units, link_ptr, links, canonical, *params)
    return _WANT[key]


def _bubbles_device(ctx, g, rec, link_ptr, links, params, skew=3, partner=True):
    """the device form into guarded arrays -> (pop, partner, n_pop)"""
    nS = len(rec)
    ins = [_upload(ctx, rec), _upload(ctx, link_ptr), _upload(ctx, links)]
    d_pop, d_partner = _Guarded(ctx, nS, skew), _Guarded(ctx, nS * 4)
    try:
        n = g.unitig_bubbles_device(ins[0], nS, ins[1], ins[2], len(links), *params, d_pop.ptr, d_partner.ptr if partner else 0)
        ctx.sync()
        return d_pop.fetch(nS, np.uint8), d_partner.fetch(nS * 4 if partner else 0, np.uint32), n
    finally:
        ctx.sync()
        d_pop.fetch(nS)                                             # whatever happened: nothing outside the arrays
        d_partner.fetch(nS * 4 if partner else 0)
        d_pop.free()
        d_partner.free()
        for p in ins:
            ctx.free(p)


# ------------------------------------------------------------------ the rule on the grid

@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", KS)
def test_unitig_bubbles(ctx, k, canonical):
    table, units, link_ptr, links = _ref(k, canonical)
    g = _job(ctx, _bubble_input(k, canonical), k, canonical)
    digest, histo = g.digest(), g.histogram(16)
    data, start, length, rec = g.unitigs(1)
    _same((data, start, length, rec), ur.layout(units))
    _same_links(g.unitig_links(data, start, length), (link_ptr, links))
    for params in PARAMS(k):
        want_pop, want_partner = _want(k, canonical, params)
        pop, partner = g.unitig_bubbles(rec, link_ptr, links, *params)
        assert pop.dtype == np.uint8 and partner.dtype == np.uint32
        assert pop.tolist() == want_pop.tolist() and partner.tolist() == want_partner.tolist(), params
        pop, partner, n = _bubbles_device(ctx, g, rec, link_ptr, links, params)
        assert pop.tolist() == want_pop.tolist() and partner.tolist() == want_partner.tolist() and n == int(want_pop.sum()), params
    pop, _, n = _bubbles_device(ctx, g, rec, link_ptr, links, PARAMS(k)[1], skew=1, partner=False)    # partner may be NULL
    assert pop.tolist() == _want(k, canonical, PARAMS(k)[1])[0].tolist() and n == int(pop.sum())
    assert g.digest() == digest and (g.histogram(16) == histo).all()


# ------------------------------------------------------------------ the loop

def _rows(rows):
    """the reference's bubble rows in the shape simplify() returns them"""
    out = []
    for rnd, j, partner, (seq, kc, n, circ), (kseq, kkc, kn, kcirc) in rows:
        out.append((rnd, j, partner, (kc, n, 1 if circ else 0), (kkc, kn, 1 if kcirc else 0), seq, ur.rc(kseq) if partner & 1 else kseq))
    return out


@pytest.mark.parametrize("mode", ["tips", "bubbles", "both"])
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [12, 21, 33])
def test_simplify_round_for_round(ctx, k, canonical, mode):
    table = _ref(k, canonical)[0]
    tips, bubbles = mode != "bubbles", mode != "tips"
    want_units, want_report, reduced, want_rows = br.simplify(table, k, canonical, 1, tips, bubbles, rounds=8, bubble_max_diff=1)
    assert want_report[-1][1:3] == (0, 0) and len(want_report) >= 2     # (the fixed point is reached, and not at once)
    g = _job(ctx, _bubble_input(k, canonical), k, canonical)
    digest, histo = g.digest(), g.histogram(16)
    got, report, rows = g.simplify(1, tips, bubbles, rounds=8, bubble_max_diff=1)
    assert report == want_report
    assert rows == _rows(want_rows)
    _same(got, ur.layout(want_units))
    _same_links(g.unitig_links(got[0], got[1], got[2]), lr.links(want_units, reduced, k, canonical, 1))
    assert g.mask_count() == len(table) - len(reduced)
    assert g.digest() == digest and (g.histogram(16) == histo).all()
    if mode == "tips":                                                  # tips only: what clip_tips() does
        g2 = _job(ctx, _bubble_input(k, canonical), k, canonical)
        clipped, clip_report = g2.clip_tips(1, None, 2.0, rounds=8)
        _same(got, clipped)
        assert [(u, t, m) for u, t, b, m in report] == clip_report and all(r[2] == 0 for r in report) and rows == []
        return
    # one round only, and the other ratio
    g2 = _job(ctx, _bubble_input(k, canonical), k, canonical)
    got, report, rows = g2.simplify(1, tips, bubbles, rounds=1, bubble_ratio=2.0)
    want_units, want_report, _, want_rows = br.simplify(table, k, canonical, 1, tips, bubbles, rounds=1, bubble_ratio_q8=512)
    assert report == want_report and rows == _rows(want_rows)
    _same(got, ur.layout(want_units))


# ------------------------------------------------------------------ untrusted rows

@pytest.mark.parametrize("canonical", [False, True])
def test_unitig_bubbles_refuses_bad_rows(ctx, canonical):
    import cfrk_amd
    k = 21
    table, units, link_ptr, links = _ref(k, canonical)
    g = _job(ctx, _bubble_input(k, canonical), k, canonical)
    rec = ur.layout(units)[3]
    nS = len(units)
    j = next(i for i in range(nS) if link_ptr[i + 1] - link_ptr[i] >= 1 and i > 0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def refused(ptr, rows, unitig):
        with pytest.raises(cfrk_amd.CfrkError) as e:
            _bubbles_device(ctx, g, rec, ptr, rows, (k, 1, 0))
        assert e.value.code == CFRK_ERR_LAYOUT and ("unitig %d " % unitig) in str(e.value)
        # every byte is written whatever is refused: the device arrays ...
        ins = [_upload(ctx, rec), _upload(ctx, ptr), _upload(ctx, rows)]
        d_pop, d_partner = _Guarded(ctx, nS), _Guarded(ctx, nS * 4)
        n = C.c_int64(-1)
        assert ctx._L.cfrk_global_unitig_bubbles_device(ctx._h, C.c_void_p(ins[0]), nS, C.c_void_p(ins[1]), C.c_void_p(ins[2]), len(rows),
                                                        k, 1, 0, C.c_void_p(d_pop.ptr), C.c_void_p(d_partner.ptr),
                                                        C.byref(n)) == CFRK_ERR_LAYOUT
        ctx.sync()
        assert not d_pop.fetch(nS).any() and (d_partner.fetch(nS * 4, np.uint32) == NONE).all() and n.value == 0
        d_pop.free()
        d_partner.free()
        for p in ins:
            ctx.free(p)
        # ... and the host arrays
        pop, partner = np.full(nS, 7, np.uint8), np.full(nS, 7, np.uint32)
        assert ctx._L.cfrk_global_unitig_bubbles(ctx._h, vp(rec), nS, vp(ptr), vp(rows), len(rows), k, 1, 0, vp(pop), vp(partner),
                                                 C.byref(n)) == CFRK_ERR_LAYOUT
        assert not pop.any() and (partner == NONE).all()

    bad = link_ptr.copy()                                           # link_ptr descends
    bad[j] = link_ptr[j + 1] + 1
    row_max = 16 if canonical else 4                                # (row j - 1 now ends behind row j: it may be refused first)
    refused(bad, links, j - 1 if bad[j] > len(links) or bad[j] - link_ptr[j - 1] > row_max else j)
    bad = link_ptr.copy()                                           # ... does not begin at 0, does not end at n_links
    bad[0] = 1
    refused(bad, links, 0)
    bad = link_ptr.copy()
    bad[nS] -= 1
    refused(bad, links, nS - 1)
    rows = links.copy()                                             # a target that is no unitig
    rows[link_ptr[j]]["to"] = nS
    refused(link_ptr, rows, j)
    rows = links.copy()                                             # an undefined flag bit
    rows[link_ptr[j]]["flags"] |= 4
    refused(link_ptr, rows, j)
    if not canonical:                                               # a strand flag where there is one strand
        rows = links.copy()
        rows[link_ptr[j]]["flags"] = 1
        refused(link_ptr, rows, j)
    long_row = 17 if canonical else 5                               # a row longer than an oriented end can have
    rows = np.zeros(long_row, lr.UNITIG_LINK_DTYPE)
    ptr = np.full(nS + 1, long_row, np.int64)
    ptr[0] = 0
    refused(ptr, rows, 0)
    if not canonical:                                               # more links into one unitig than 4 bases can give
        rows = np.zeros(5, lr.UNITIG_LINK_DTYPE)
        rows["to"] = nS - 1
        ptr = np.array([0, 1, 2, 3, 4] + [5] * (nS - 4), np.int64)
        refused(ptr, rows, nS - 1)
    # CFRK_ERR_ARG
    L, h = ctx._L, ctx._h
    pop, partner, n = np.zeros(nS, np.uint8), np.zeros(nS, np.uint32), C.c_int64()
    ok = (vp(rec), nS, vp(link_ptr), vp(links), len(links), k, 0, 0, vp(pop), vp(partner), C.byref(n))
    for fn in (L.cfrk_global_unitig_bubbles, L.cfrk_global_unitig_bubbles_device):
        for pos, value in ((0, None), (2, None), (3, None), (8, None), (10, None), (1, -1), (4, -1), (1, 1 << 31), (7, 65537)):
            args = list(ok)
            args[pos] = value
            assert fn(h, *args) == CFRK_ERR_ARG, (pos, value)
        assert fn(h, None, 0, None, None, 0, k, 0, 0, None, None, C.byref(n)) == 0 and n.value == 0     # nS = 0: nothing popped
    assert L.cfrk_global_unitig_bubbles(h, *ok[:7], 65536, *ok[8:]) == 0                               # the bound itself is fine
    args = list(ok)
    args[9] = None                                                                                     # partner may be NULL
    assert L.cfrk_global_unitig_bubbles(h, *args) == 0 and n.value == int(_want(k, canonical, (k, 0, 0))[0].sum())
    with cfrk_amd.Context(0) as c:                                                                     # no job
        assert c._L.cfrk_global_unitig_bubbles(c._h, None, 0, None, None, 0, 1, 0, 0, None, None, C.byref(n)) == CFRK_ERR_STATE
        assert c._L.cfrk_global_unitig_bubbles_device(c._h, None, 0, None, None, 0, 1, 0, 0, None, None, C.byref(n)) == CFRK_ERR_STATE


def _csr(nS, frm, to, flags):
    """links (frm[i] -> to[i], flags[i]) as the CSR rows of nS unitigs"""
    order = np.argsort(frm, kind="stable")
    rows = np.zeros(len(frm), lr.UNITIG_LINK_DTYPE)
    rows["to"], rows["flags"] = np.asarray(to)[order], np.asarray(flags)[order]
    ptr = np.zeros(nS + 1, np.int64)
    np.cumsum(np.bincount(np.asarray(frm, np.int64), minlength=nS), out=ptr[1:])
    return ptr, rows


@pytest.mark.parametrize("canonical", [False, True])
def test_hostile_rows_that_pass_the_check(ctx, canonical):
    """rows that are no real link set but pass the check: CFRK_OK, every byte written, partners in range, nothing outside
    the arrays touched"""
    import cfrk_amd
    g = cfrk_amd.GlobalCounter(ctx, 21, cfrk_amd.CFRK_CANONICAL if canonical else 0, 1000)
    nS = 700
    rng = np.random.default_rng(77 + canonical)
    rec = np.zeros(nS, cfrk_amd.UNITIG_DTYPE)
    rec["kc"], rec["n_kmers"] = rng.integers(1, 1000, nS), rng.integers(1, 4, nS)
    cases = []
    # an arm whose src row points back at it: 0 -> 1 -> 0 -> ..., and a two-cycle of arms 2 <-> 3
    frm, to = [0, 1, 2, 3] + list(range(4, nS - 1)), [1, 0, 3, 2] + list(range(5, nS))
    cases.append(_csr(nS, frm, to, np.zeros(len(frm), np.uint32)))
    # all targets equal: every unitig links to unitig 5 once (in-degree 4 at most where there is one strand)
    many = nS if canonical else 4
    cases.append(_csr(nS, np.arange(many), np.full(many, 5), np.zeros(many, np.uint32)))
    # random rows, in a canonical job with random strand flags and no mirrors
    m = nS if not canonical else 3 * nS
    frm = rng.integers(0, nS, m)
    to = rng.permutation(nS)[:m] if not canonical else rng.integers(0, nS, m)       # (not canonical: in-degree 1 at most)
    frm = frm[np.argsort(frm, kind="stable")]
    keep = np.ones(m, bool)
    keep[4:] = frm[4:] != frm[:-4]                                                  # rows of at most 4 links
    flags = rng.integers(0, 4, m).astype(np.uint32) if canonical else np.zeros(m, np.uint32)
    cases.append(_csr(nS, frm[keep], to[keep], flags[keep]))
    if canonical:                                                                   # a fan of arms without mirrors: 0 -> 1..8 -> 9
        frm, to = [0] * 8 + list(range(1, 9)), list(range(1, 9)) + [9] * 8
        fl = [0] * 16
        frm += list(range(1, 9))                                                    # their in-links, stated on their own rows only
        to += [0] * 8
        fl += [3] * 8
        cases.append(_csr(nS, frm, to, np.array(fl, np.uint32)))
    for ptr, rows in cases:
        for params in ((3, 3, 0), (3, 0, 512)):
            pop, partner, n = _bubbles_device(ctx, g, rec, ptr, rows, params)
            assert set(pop.tolist()) <= {0, 1} and n == int(pop.sum())
            assert ((partner == NONE) == (pop == 0)).all() and (partner[pop == 1] < 2 * nS).all()
            if not canonical:
                assert (partner[pop == 1] & 1 == 0).all()
            hpop, hpartner = g.unitig_bubbles(rec, ptr, rows, *params)
            assert hpop.tolist() == pop.tolist() and hpartner.tolist() == partner.tolist()
    if canonical:                                                                   # the fan: arms 1..8 are parallel as the rows state it
        pop, partner, n = _bubbles_device(ctx, g, rec, *cases[-1], (3, 3, 0))
        assert n == 7 and pop[1:9].sum() == 7 and not pop[9:].any()


# ------------------------------------------------------------------ a chain of 10^5 bubbles, no k-mers

@pytest.mark.parametrize("canonical", [False, True])
def test_a_chain_of_bubbles(ctx, canonical):
    """src_i -> {a_i, b_i} -> src_{i+1} for i < 10^5, as records and rows: 300 001 unitigs, so the grid-stride loops and the
    wave ballot turn more than once.  src_i = 3i, a_i = 3i + 1, b_i = 3i + 2.  In the canonical variant every link has
    its mirror and every other b_i is stored reversed: it is entered and left as (b_i,-)."""
    import cfrk_amd
    N = 100000
    nS = 3 * N + 1
    rng = np.random.default_rng(5 + canonical)
    i = np.arange(N, dtype=np.int64)
    src, a, b, nxt = 3 * i, 3 * i + 1, 3 * i + 2, 3 * i + 3
    rec = np.zeros(nS, cfrk_amd.UNITIG_DTYPE)
    rec["n_kmers"], rec["kc"] = 5, 50
    rec["n_kmers"][a] = 3
    rec["n_kmers"][b] = np.where(i % 7 == 0, 4, 3)                  # every seventh pair: lengths 3 and 4
    rec["kc"][a], rec["kc"][b] = rng.integers(1, 40, N), rng.integers(1, 40, N)
    same = i % 5 == 0                                               # every fifth pair: equal coverage
    rec["kc"][b] = np.where(same, rec["kc"][a] * rec["n_kmers"][b] // 3, rec["kc"][b])
    rec["kc"][a] = np.where(same, rec["kc"][a] * rec["n_kmers"][a] // 3, rec["kc"][a])
    rec["flags"][a[i % 11 == 0]] = cfrk_amd.CFRK_UNITIG_CIRCULAR    # every eleventh a_i claims to be a circle: no arm
    rev = (i % 2 == 1) if canonical else np.zeros(N, bool)
    FM, TM = cfrk_amd.CFRK_LINK_FROM_MINUS, cfrk_amd.CFRK_LINK_TO_MINUS
    rb = rev.astype(np.uint32)
    frm = [src, a, src, b]
    to = [a, nxt, b, nxt]
    flags = [np.zeros(N, np.uint32), np.zeros(N, np.uint32), rb * TM, rb * FM]
    if canonical:                                                   # (u,ou) -> (v,ov) has the mirror (v,!ov) -> (u,!ou)
        frm += [a, nxt, b, nxt]
        to += [src, a, src, b]
        flags += [np.full(N, FM | TM, np.uint32), np.full(N, FM | TM, np.uint32), (1 - rb) * FM + TM, FM + (1 - rb) * TM]
    ptr, rows = _csr(nS, np.concatenate(frm), np.concatenate(to), np.concatenate(flags).astype(np.uint32))
    g = cfrk_amd.GlobalCounter(ctx, 21, cfrk_amd.CFRK_CANONICAL if canonical else 0, 1000)
    na, nb = rec["n_kmers"][a].astype(np.int64), rec["n_kmers"][b].astype(np.int64)
    ka, kb = rec["kc"][a].astype(np.int64), rec["kc"][b].astype(np.int64)
    for max_kmers, max_diff, ratio_q8 in ((3, 0, 0), (4, 1, 0), (4, 1, 384), (4, 0, 512)):
        both = (rec["flags"][a] == 0) & (na <= max_kmers) & (nb <= max_kmers) & (np.abs(na - nb) <= max_diff)
        a_wins = ka * nb >= kb * na                                 # a ranks above b: the better mean, a < b on a tie
        pop_b = both & a_wins & (256 * ka * nb >= ratio_q8 * kb * na)
        pop_a = both & ~a_wins & (256 * kb * na >= ratio_q8 * ka * nb)
        want_pop = np.zeros(nS, np.uint8)
        want_pop[b[pop_b]], want_pop[a[pop_a]] = 1, 1
        want_partner = np.full(nS, NONE, np.uint32)
        want_partner[b[pop_b]] = (a[pop_b] << 1) | rev[pop_b]
        want_partner[a[pop_a]] = (b[pop_a] << 1) | rev[pop_a]
        assert want_pop.sum() > 1000
        pop, partner, n = _bubbles_device(ctx, g, rec, ptr, rows, (max_kmers, max_diff, ratio_q8))
        assert n == int(want_pop.sum()) and (pop == want_pop).all() and (partner == want_partner).all()
    pop, partner = g.unitig_bubbles(rec, ptr, rows, 4, 0, 512)      # the host form, the last set
    assert (pop == want_pop).all() and (partner == want_partner).all()


# ------------------------------------------------------------------ CLI

@pytest.mark.parametrize("k,canonical,min_count,tips", [(12, False, 1, False), (21, True, 1, True), (31, True, 1, False), (33, False, 1, True)])
def test_cli_pop_bubbles(tmp_path, k, canonical, min_count, tips):
    seqs = _bubble_input(k, canonical)
    fasta = tmp_path / "in.fa"
    with open(fasta, "w") as f:
        i = 0
        for s, t in seqs:
            for _ in range(t):
                f.write(">r%d\n%s\n" % (i, s))
                i += 1
    table = _table(seqs, k, canonical)
    units, report, reduced, rows = br.simplify(table, k, canonical, min_count, tips, True, 4, None, 512, None, 1, 0)
    assert report[0][2] >= 3 and (report[0][1] >= 3) == tips
    link_ptr, links = lr.links(units, reduced, k, canonical, min_count)
    tail = [str(k), "--global"] + (["--canonical"] if canonical else [])
    P = lambda name: str(tmp_path / name)
    outs = lambda t: ["--unitigs-out", P(t + ".fa"), "--unitigs-links", "--unitigs-gfa", P(t + ".gfa"), "--unitigs-min-count", str(min_count)]
    pop = ["--unitigs-pop-bubbles", "--bubble-max-diff", "1", "--tip-report", P("r.tsv"), "--bubble-report", P("b.tsv")]
    subprocess.run([_cli(), str(fasta), P("a.out")] + tail + outs("pop") + pop + (["--unitigs-clip-tips"] if tips else []), check=True, timeout=300)
    read = lambda name: open(tmp_path / name, "rb").read()
    assert read("pop.fa") == lr.fasta_text_links(units, link_ptr, links)
    assert read("pop.gfa") == lr.gfa_text(units, k, link_ptr, links)
    assert read("r.tsv") == br.report_text(report)
    assert read("b.tsv") == br.bubble_lines(rows) and read("b.tsv").count(b"\n") == sum(r[2] for r in report)
    # the other options: one round, the other ratio, shorter arms; no report files
    more = ["--unitigs-pop-bubbles", "--bubble-max-kmers", str(k - 1), "--bubble-ratio", "2", "--simplify-rounds", "1"]
    subprocess.run([_cli(), str(fasta), P("c.out")] + tail + ["--unitigs-out", P("c.fa"), "--unitigs-min-count", str(min_count)] + more,
                   check=True, timeout=300)
    units2 = br.simplify(table, k, canonical, min_count, False, True, 1, None, 512, k - 1, 0, 512)[0]
    assert read("c.fa") == ur.fasta_text(units2)
    assert read("a.out") == read("c.out")                           # the counts' own output does not see the options
    if tips:
        # --unitigs-clip-tips alone: the tip loop and its four-field report, as before
        subprocess.run([_cli(), str(fasta), P("d.out")] + tail + outs("clip") + ["--unitigs-clip-tips", "--tip-report", P("r4.tsv")],
                       check=True, timeout=300)
        cunits, creport, creduced = tr.clip(table, k, canonical, min_count, None, 512, rounds=4)
        cptr, clinks = lr.links(cunits, creduced, k, canonical, min_count)
        assert read("clip.fa") == lr.fasta_text_links(cunits, cptr, clinks)
        assert read("clip.gfa") == lr.gfa_text(cunits, k, cptr, clinks)
        assert read("r4.tsv") == tr.report_text(creport)
        assert read("d.out") == read("a.out")
