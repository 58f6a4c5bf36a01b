"""GPU: the graph mask (cfrk_global_mask_keys / _mask_unitigs / _mask_clear / _mask_count) and the tip rule
(cfrk_global_unitig_tips), every call in its device form and its host form, against tests/tips_ref.py: a masked graph
is the graph of the dictionary without the masked keys, so unitigs, links, neighbour masks, positions and hits are
compared byte for byte with the existing references on the reduced dictionary; counts, digest and histogram do not
move.  The mask's lifetime; the tip rule on the k grid of the unitig tests and on crafted rows it must refuse; the clip
loop round for round; a 300 000-node chain masked in one launch; the CLI."""
import ctypes as C
import subprocess
import time

import numpy as np
import pytest

from . import read_hits_ref as hr
from . import tips_ref as tr
from . import unitig_links_ref as lr
from . import unitig_ref as ur
from .test_gpu_filter import _Guarded, _upload
from .test_gpu_query import _cli
from .test_gpu_read_hits import _hits_device, _keys, _locate_device
from .test_gpu_unitig_links import _DeviceUnitigs, _device_links, _same_links, long_genome  # noqa: F401 (a fixture)
from .test_gpu_unitigs import KS, _device_unitigs, _job, _rand, _same, _table

pytestmark = pytest.mark.gpu

CFRK_ERR_ARG, CFRK_ERR_STATE, CFRK_ERR_LAYOUT = -1, -4, -5
NONE = 0xFFFFFFFF
MASK_KS = [3, 12, 13, 21, 32, 33, 64]
PARAMS = lambda k: [(k, 0), (k, 512), (1, 256), (0, 0)]


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


def _other(rng, c):
    return ur.BASES[(ur.BASES.index(c) + int(rng.integers(1, 4))) % 4]


# At k = 3 and 4 a random genome of any useful length holds nearly every k-mer and the graph has no dead end.  These two
# inputs were picked by a seed search on the REFERENCE for graphs with at least three tips and a surviving candidate
# under both strand rules; they are data, like the seeds below.
_SMALL = {
    3: [("TGCATACTT", 4), ("AATA", 2), ("TGTT", 1), ("TGTC", 2), ("TACT", 2), ("GCTC", 2)],
    4: [("CCTTTTGAGGCTCCCGATTGAGGTAGTCTCGGAGTG", 4), ("CCCGC", 1), ("CAGTC", 1), ("AGTGG", 1), ("AGTGT", 2)],
}
_INPUTS = {}


def _tip_input(k):
    """[(string, times counted)]: a random genome of 3000 bases counted 4 times and, planted on it: right and left tips of
    1, k - 1, k and k + 1 k-mers counted once; two sibling tips at the genome's end, counted once and twice; a bubble
    counted once; an isolated k-mer; a circle of 2k k-mers counted twice that carries a tip; a tip counted 6 times; a
    hairpin counted twice"""
    if k in _INPUTS:
        return _INPUTS[k]
    if k in _SMALL:
        _INPUTS[k] = _SMALL[k]
        return _SMALL[k]
    rng = np.random.default_rng(7000 + 100 * k)
    L = min(3000, max(3 * k, 4 ** k // 6))
    G = _rand(rng, L)
    seqs = [(G, 4)]
    spots = iter(np.linspace(1, L - k - 2, 12).astype(int).tolist())
    for m in (1, k - 1, k, k + 1):
        a = next(spots)                                         # a right tip of m k-mers behind G[a:a+k]
        seqs.append((G[a:a + k] + _other(rng, G[a + k]) + _rand(rng, m - 1), 1))
        a = next(spots)                                         # a left tip of m k-mers in front of G[a:a+k]
        seqs.append((_rand(rng, m - 1) + _other(rng, G[a - 1]) + G[a:a + k], 1))
    x = _rand(rng, 1)
    seqs.append((G[-k:] + x + _rand(rng, 2), 1))                # two sibling tips at the genome's end
    seqs.append((G[-k:] + _other(rng, x) + _rand(rng, 2), 2))
    a = next(spots)                                             # a bubble
    seqs.append((G[a:a + k] + _other(rng, G[a + k]) + G[a + k + 1:a + 2 * k + 1], 1))
    seqs.append((_rand(rng, k), 1))                             # an isolated k-mer
    c = _rand(rng, 2 * k)                                       # a circle of 2k k-mers carrying a tip
    seqs.append((c + c[:k - 1], 2))
    seqs.append((c[2:2 + k] + _other(rng, c[2 + k]) + _rand(rng, 2), 1))
    a = next(spots)                                             # a tip counted 6 times
    seqs.append((G[a:a + k] + _other(rng, G[a + k]) + _rand(rng, 2), 6))
    h = _rand(rng, k + 7)                                       # a hairpin
    seqs.append((h + ur.rc(h), 2))
    _INPUTS[k] = seqs
    return seqs


_REF = {}


def _ref(k, canonical, min_count=1):
    """(table, units, link_ptr, links) of the planted input, computed once"""
    key = (k, canonical, min_count)
    if key not in _REF:
        table = _table(_tip_input(k), k, canonical)
        _REF[key] = (table,) + tr.graph(table, k, canonical, min_count)
    return _REF[key]


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", KS)
def test_the_input_has_tips_and_survivors(k, canonical):
    """on the reference alone: every point of the grid has at least three tips and a candidate that stays"""
    table, units, link_ptr, links = _ref(k, canonical)
    for max_kmers, ratio_q8 in ((k, 0), (k, 512)):
        tip = tr.tips(units, link_ptr, links, canonical, max_kmers, ratio_q8)
        cand = tr.candidates(units, link_ptr, links, canonical, max_kmers)
        assert tip.sum() >= 3, (k, canonical, ratio_q8)
        assert sum(cand) - tip.sum() >= 1, (k, canonical, ratio_q8)


# ------------------------------------------------------------------ the mask

def _mask_keys_device(ctx, g, lo, hi):
    d_lo, d_hi = _upload(ctx, lo), (_upload(ctx, hi) if hi is not None else 0)
    g.mask_keys_device(d_lo, d_hi, len(lo))
    ctx.sync()
    for p in (d_lo, d_hi):
        if p:
            ctx.free(p)


@pytest.mark.parametrize("min_count", [1, 2])
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", MASK_KS)
def test_mask_keys(ctx, k, canonical, min_count):
    import cfrk_amd
    seqs = _tip_input(k)
    table = _table(seqs, k, canonical)
    g = _job(ctx, seqs, k, canonical)
    digest, histo = g.digest(), g.histogram(16)
    rng = np.random.default_rng(300 + k)
    stored = sorted(table)
    gone = [stored[i] for i in sorted(rng.choice(len(stored), max(1, len(stored) // 3), replace=False).tolist())]
    every = ["".join(ur.BASES[(i >> (2 * j)) & 3] for j in range(k)) for i in range(64)] if k == 3 else [_rand(rng, k) for _ in range(50)]
    absent = [x for x in every if (min(x, ur.rc(x)) if canonical else x) not in table][:50]
    assert absent
    # a canonical job canonicalises: every other key goes in as the reverse complement of the stored one
    given = [ur.rc(x) if canonical and i % 2 else x for i, x in enumerate(gone)] + absent + [gone[0]]
    lo, hi = _keys(given)
    hi_arg = hi if k > 32 or rng.random() < 0.5 else None
    reduced = tr.masked_table(table, gone, canonical)
    assert len(reduced) == len(table) - len(gone)
    assert g.mask_count() == 0
    _mask_keys_device(ctx, g, lo, hi_arg)
    assert g.mask_count() == len(gone)
    g.mask_clear()
    assert g.mask_count() == 0
    g.mask_keys(lo[:len(lo) // 2], None if hi_arg is None else hi_arg[:len(lo) // 2])
    g.mask_keys(lo[len(lo) // 2:], None if hi_arg is None else hi_arg[len(lo) // 2:])       # the mask grows
    assert g.mask_count() == len(gone)
    if k < 32:                                                      # bits at or above 2k: no such key
        g.mask_keys(_keys(stored)[0] | np.uint64(1 << (2 * k)))
        assert g.mask_count() == len(gone)
    # the graph is that of the reduced dictionary
    units = ur.unitigs(reduced, k, canonical, min_count)
    want = ur.layout(units)
    _same(_device_unitigs(ctx, g, min_count, skew=1), want)
    got = g.unitigs(min_count)
    _same(got, want)
    data, start, length, rec = got
    want_links = lr.links(units, reduced, k, canonical, min_count)
    _same_links(g.unitig_links(data, start, length, min_count), want_links)
    _same_links(_device_links(ctx, g, min_count, data, start, length, skew=3), want_links)
    probe = stored + [ur.rc(x) for x in stored] + absent
    plo, phi = _keys(probe)
    nb = g.neighbors(plo, phi, min_count)
    assert nb.tolist() == [ur.neighbor_mask(reduced, x, k, canonical, min_count) for x in probe]
    # the position map: the unmasked list is refused, the new one accepted
    full = ur.layout(ur.unitigs(table, k, canonical, min_count))
    if full[0].tobytes() != data.tobytes():
        with pytest.raises(cfrk_amd.CfrkError) as e:
            g.unitig_index(full[0], full[1], full[2], min_count)
        assert e.value.code == CFRK_ERR_LAYOUT
    else:
        assert min_count == 2                                       # (only keys counted once were masked)
    g.unitig_index(data, start, length, min_count)
    G = hr.Graph(reduced, k, canonical, min_count)
    got = g.locate(plo, phi)
    assert got.tobytes() == G.locate_rows(probe).tobytes()
    glo, ghi = _keys(gone)
    assert (g.locate(glo, ghi)["unitig"] == NONE).all()
    assert _locate_device(ctx, g, plo, phi).tobytes() == got.tobytes()
    strings = [s for s, _ in seqs]
    reads = strings + [ur.rc(s) for s in strings] + [strings[0][:len(strings[0]) // 2] + "N" + strings[0][len(strings[0]) // 2:], ""]
    w_ptr, w_hits = G.hit_rows(reads)
    rdata, rstart, rlength = hr.read_codes(reads)
    ptr, hits = g.read_hits(rdata, rstart, rlength)
    assert ptr.tobytes() == w_ptr.tobytes() and hits.tobytes() == w_hits.tobytes()
    ptr, hits = _hits_device(ctx, g, rdata, rstart, rlength)
    assert ptr.tobytes() == w_ptr.tobytes() and hits.tobytes() == w_hits.tobytes()
    # the counts never saw the mask
    assert g.query(glo, ghi).tolist() == [table[x] for x in gone]
    assert g.digest() == digest and (g.histogram(16) == histo).all()
    assert g.mask_count() == len(gone)                              # (digest and histogram left index and mask alone)


def test_mask_lifetime(ctx):
    import cfrk_amd
    k, canonical = 21, True
    seqs = _tip_input(k)
    table, units, _, _ = _ref(k, canonical)
    full = ur.layout(units)
    g = _job(ctx, seqs, k, canonical)
    stored = sorted(table)
    lo, hi = _keys(stored[:40])
    g.unitig_index(full[0], full[1], full[2])
    assert (g.locate(lo)["unitig"] != NONE).all()
    g.mask_keys(lo[:5])
    with pytest.raises(cfrk_amd.CfrkError) as e:                    # every change of the mask drops the map
        g.locate(lo)
    assert e.value.code == CFRK_ERR_STATE
    with pytest.raises(cfrk_amd.CfrkError) as e:
        g.read_hits(*hr.read_codes([seqs[0][0][:100]]))
    assert e.value.code == CFRK_ERR_STATE
    now = g.unitigs(1)
    _same(now, ur.layout(ur.unitigs(tr.masked_table(table, stored[:5]), k, canonical)))
    g.unitig_index(now[0], now[1], now[2])
    assert (g.locate(lo)["unitig"] == NONE).tolist() == [True] * 5 + [False] * 35
    g.mask_clear()                                                  # ... and so does the clear
    with pytest.raises(cfrk_amd.CfrkError) as e:
        g.locate(lo)
    assert e.value.code == CFRK_ERR_STATE
    assert g.mask_count() == 0
    _same(g.unitigs(1), full)
    g.mask_clear()                                                  # fine without a mask
    # the result changes: the index is rebuilt, the mask is gone
    g.mask_keys(lo)
    assert g.mask_count() == 40
    extra = "ACGTTGCA" * 6
    g.add(*hr.read_codes([extra]))
    assert g.mask_count() == 0
    table2 = _table(seqs + [(extra, 1)], k, canonical)
    _same(g.unitigs(1), ur.layout(ur.unitigs(table2, k, canonical)))
    # a mask call on a job whose index was never built builds it
    for call in ("keys", "unitigs", "count", "clear"):
        g2 = _job(ctx, seqs, k, canonical)
        if call == "keys":
            g2.mask_keys(lo)
            assert g2.mask_count() == 40
        elif call == "unitigs":
            g2.mask_unitigs(full[0], full[1], full[2], np.ones(len(full[1]), np.uint8))
            assert g2.mask_count() == len(table)
            assert len(g2.unitigs(1)[1]) == 0                       # nothing is left of the graph
        elif call == "count":
            assert g2.mask_count() == 0
        else:
            g2.mask_clear()
            _same(g2.unitigs(1), full)


def test_mask_arguments_and_state(ctx):
    import cfrk_amd
    L, h = ctx._L, ctx._h
    one = np.zeros(4, np.uint64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    n = C.c_uint64()
    with cfrk_amd.Context(0) as c:                                  # no job
        assert c._L.cfrk_global_mask_keys(c._h, vp(one), None, 1) == CFRK_ERR_STATE
        assert c._L.cfrk_global_mask_keys_device(c._h, None, None, 0) == CFRK_ERR_STATE
        assert c._L.cfrk_global_mask_unitigs(c._h, None, None, None, 0, 0, None) == CFRK_ERR_STATE
        assert c._L.cfrk_global_mask_unitigs_device(c._h, None, None, None, 0, 0, None) == CFRK_ERR_STATE
        assert c._L.cfrk_global_mask_clear(c._h) == CFRK_ERR_STATE
        assert c._L.cfrk_global_mask_count(c._h, C.byref(n)) == CFRK_ERR_STATE
        assert c._L.cfrk_global_unitig_tips(c._h, None, 0, None, None, 0, 1, 0, None, C.byref(C.c_int64())) == CFRK_ERR_STATE
    g = _job(ctx, _tip_input(21), 21, True)
    for fn in (L.cfrk_global_mask_keys, L.cfrk_global_mask_keys_device):
        assert fn(h, None, None, 0) == 0                            # n = 0 is fine
        assert fn(h, None, None, 3) == CFRK_ERR_ARG
        assert fn(h, vp(one), None, -1) == CFRK_ERR_ARG
    for fn in (L.cfrk_global_mask_unitigs, L.cfrk_global_mask_unitigs_device):
        assert fn(h, None, None, None, 0, 0, None) == 0             # nS = 0 is fine
        assert fn(h, None, None, None, 10, 1, None) == CFRK_ERR_ARG
        assert fn(h, None, None, None, -1, 0, None) == CFRK_ERR_ARG
        assert fn(h, None, None, None, 0, -1, None) == CFRK_ERR_ARG
    assert L.cfrk_global_mask_count(h, None) == CFRK_ERR_ARG
    assert g.mask_count() == 0


# ------------------------------------------------------------------ the tip rule

def _tips_device(ctx, g, rec, link_ptr, links, max_kmers, ratio_q8, skew=3):
    """the device form into a guarded byte array -> (tip, n_tips)"""
    nS = len(rec)
    ins = [_upload(ctx, rec), _upload(ctx, link_ptr), _upload(ctx, links)]
    d_tip = _Guarded(ctx, nS, skew)
    try:
        n = g.unitig_tips_device(ins[0], nS, ins[1], ins[2], len(links), max_kmers, ratio_q8, d_tip.ptr)
        ctx.sync()
        return d_tip.fetch(nS, np.uint8), n
    finally:
        ctx.sync()
        d_tip.fetch(nS)                                             # whatever happened: nothing outside the array
        d_tip.free()
        for p in ins:
            ctx.free(p)


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", KS)
def test_unitig_tips(ctx, k, canonical):
    table, units, link_ptr, links = _ref(k, canonical)
    g = _job(ctx, _tip_input(k), k, canonical)
    digest = g.digest()
    data, start, length, rec = g.unitigs(1)
    _same((data, start, length, rec), ur.layout(units))
    _same_links(g.unitig_links(data, start, length), (link_ptr, links))
    for max_kmers, ratio_q8 in PARAMS(k):
        want = tr.tips(units, link_ptr, links, canonical, max_kmers, ratio_q8)
        got = g.unitig_tips(rec, link_ptr, links, max_kmers, ratio_q8)
        assert got.dtype == np.uint8 and got.tolist() == want.tolist(), (max_kmers, ratio_q8)
        got, n = _tips_device(ctx, g, rec, link_ptr, links, max_kmers, ratio_q8)
        assert got.tolist() == want.tolist() and n == int(want.sum()), (max_kmers, ratio_q8)
    assert g.digest() == digest


@pytest.mark.parametrize("canonical", [False, True])
def test_unitig_tips_refuses_bad_rows(ctx, canonical):
    import cfrk_amd
    k = 21
    table, units, link_ptr, links = _ref(k, canonical)
    g = _job(ctx, _tip_input(k), k, canonical)
    rec = ur.layout(units)[3]
    nS = len(units)
    j = next(i for i in range(nS) if link_ptr[i + 1] - link_ptr[i] >= 1 and i > 0)

    def refused(ptr, rows, unitig):
        with pytest.raises(cfrk_amd.CfrkError) as e:
            _tips_device(ctx, g, rec, ptr, rows, k, 0)
        assert e.value.code == CFRK_ERR_LAYOUT and ("unitig %d " % unitig) in str(e.value)
        tip, n = np.full(nS, 7, np.uint8), C.c_int64(-1)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        assert ctx._L.cfrk_global_unitig_tips(ctx._h, vp(rec), nS, vp(ptr), vp(rows), len(rows), k, 0, vp(tip), C.byref(n)) == CFRK_ERR_LAYOUT

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
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    tip, n = np.zeros(nS, np.uint8), C.c_int64()
    ok = (vp(rec), nS, vp(link_ptr), vp(links), len(links), k, 0, vp(tip), C.byref(n))
    for fn in (L.cfrk_global_unitig_tips, L.cfrk_global_unitig_tips_device):
        for pos, value in ((0, None), (2, None), (3, None), (7, None), (8, None), (1, -1), (4, -1), (1, 1 << 32), (6, 65537)):
            args = list(ok)
            args[pos] = value
            assert fn(h, *args) == CFRK_ERR_ARG, (pos, value)
        assert fn(h, None, 0, None, None, 0, k, 0, None, C.byref(n)) == 0 and n.value == 0      # nS = 0: no tips
    assert L.cfrk_global_unitig_tips(h, *ok[:6], 65536, *ok[7:]) == 0                           # the bound itself is fine


# ------------------------------------------------------------------ clipping

@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [12, 21, 33])
def test_mask_unitigs_of_the_tips(ctx, k, canonical):
    table, units, link_ptr, links = _ref(k, canonical)
    tip = tr.tips(units, link_ptr, links, canonical, k, 0)
    gone = [x for j in np.flatnonzero(tip) for x in tr.unit_kmers(units[j][0], k, canonical)]
    want = ur.layout(ur.unitigs(tr.masked_table(table, gone), k, canonical))
    data, start, length, rec = ur.layout(units)
    g = _job(ctx, _tip_input(k), k, canonical)
    digest = g.digest()
    g.mask_unitigs(data, start, length, tip)
    assert g.mask_count() == len(set(gone))
    _same(g.unitigs(1), want)
    g.mask_clear()
    d = _DeviceUnitigs(ctx, data, start, length, skew=5)
    d_drop = _upload(ctx, tip)
    g.mask_unitigs_device(*d.args, d_drop)
    assert g.mask_count() == len(set(gone))
    _same(g.unitigs(1), want)
    # untrusted tables: reads outside [0, nN) and invalid codes are skipped, nothing else is masked
    g.mask_clear()
    far, bad = start.copy(), data.copy()
    first = int(np.flatnonzero(tip)[0])
    far[first] = len(data) - 2
    g.mask_unitigs_device(d.args[0], _upload_keep(ctx, far, d), d.args[2], d.nN, d.nS, d_drop)
    assert g.mask_count() <= len(set(gone)) - 1
    ctx.free(d_drop)
    d.free()
    assert g.digest() == digest


def _upload_keep(ctx, arr, owner):
    p = _upload(ctx, arr)
    owner.base.append(p)                                            # freed with the list
    return p


@pytest.mark.parametrize("ratio", [2.0, 0.0])
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [12, 21, 33])
def test_clip_tips_round_for_round(ctx, k, canonical, ratio):
    table = _ref(k, canonical)[0]
    want_units, want_report, reduced = tr.clip(table, k, canonical, 1, None, int(ratio * 256), rounds=8)
    assert want_report[-1][1] == 0 and len(want_report) >= 2        # (the fixed point is reached, and not at once)
    g = _job(ctx, _tip_input(k), k, canonical)
    got, report = g.clip_tips(1, None, ratio, rounds=8)
    assert report == want_report
    _same(got, ur.layout(want_units))
    assert g.mask_count() == len(table) - len(reduced)
    # one round only
    g2 = _job(ctx, _tip_input(k), k, canonical)
    got, report = g2.clip_tips(1, None, ratio, rounds=1)
    assert report == want_report[:1]
    _same(got, ur.layout(tr.clip(table, k, canonical, 1, None, int(ratio * 256), rounds=1)[0]))


def test_clipped_graph_at_k31(ctx):
    """k = 31, both strands, min_count 1: the clipped graph of the planted input is the reference's, unitig for unitig; the
    genome's chain is cut only where something that is no tip still hangs on it (the bubble, the two tips longer than
    k, the surviving arm at its end, the well-covered tip at the default ratio)"""
    k = 31
    table, units, _, _ = _ref(k, True)
    want_units, want_report, reduced = tr.clip(table, k, True, 1, None, 512, rounds=8)
    assert len(want_units) < len(units) - want_report[0][1]         # clipping merges what the tips had cut apart
    g = _job(ctx, _tip_input(k), k, True)
    (data, start, length, rec), report = g.clip_tips(rounds=8)
    assert len(start) == len(want_units) and report == want_report
    _same((data, start, length, rec), ur.layout(want_units))
    genome = _tip_input(k)[0][0]
    pieces = lambda us: [u[2] for u in us if u[0] in genome or ur.rc(u[0]) in genome]
    assert len(pieces(want_units)) < len(pieces(units)) and max(pieces(want_units)) > max(pieces(units))


# ------------------------------------------------------------------ balance: one launch over tiles

def test_mask_unitigs_of_a_long_chain(ctx, long_genome):
    import cfrk_amd
    G = long_genome
    k = 31
    mid = len(G) // 2
    tip = np.concatenate([G[mid:mid + k], [(G[mid + k] + 1) % 4, 0, 1]]).astype(np.int8)
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, 400000)
    g.add(np.concatenate([G, [-1], tip, [-1]]).astype(np.int8))
    assert len(g.unitigs(1)[1]) == 3                                # the chain cut in two at the fork, and the tip
    chain = np.append(G, np.int8(-1))
    start, length, drop = np.array([0], np.int64), np.array([len(G)], np.int32), np.array([1], np.uint8)
    d = _DeviceUnitigs(ctx, chain, start, length, skew=3)
    d_drop = _upload(ctx, drop)
    ctx.sync()
    t0 = time.perf_counter()
    g.mask_unitigs_device(*d.args, d_drop)
    ctx.sync()
    took = time.perf_counter() - t0
    assert g.mask_count() == len(G) - k + 1
    assert took < 2.0, took
    data, ustart, ulength, rec = g.unitigs(1)                       # what is left: the tip's own three k-mers
    assert rec.tolist() == [(3, 3, 0)]
    ctx.free(d_drop)
    d.free()


# ------------------------------------------------------------------ CLI

@pytest.mark.parametrize("k,canonical,min_count", [(5, False, 1), (21, True, 1), (31, True, 2), (40, False, 1)])
def test_cli_clip_tips(tmp_path, k, canonical, min_count):
    seqs = _tip_input(k)
    fasta = tmp_path / "in.fa"
    with open(fasta, "w") as f:
        i = 0
        for s, t in seqs:
            for _ in range(t):
                f.write(">r%d\n%s\n" % (i, s))
                i += 1
    reads = [s for s, _ in seqs] + [ur.rc(s) for s, _ in seqs[:6]]
    q = tmp_path / "q.fa"
    with open(q, "w") as f:
        for i, s in enumerate(reads):
            f.write(">q%d\n%s\n" % (i, s))
    table = _table(seqs, k, canonical)
    units, report, reduced = tr.clip(table, k, canonical, min_count, None, 512, rounds=4)
    link_ptr, links = lr.links(units, reduced, k, canonical, min_count)
    raw = ur.unitigs(table, k, canonical, min_count)
    raw_ptr, raw_links = lr.links(raw, table, k, canonical, min_count)
    tail = [str(k), "--global"] + (["--canonical"] if canonical else [])
    P = lambda name: str(tmp_path / name)
    outs = lambda t: ["--unitigs-out", P(t + ".fa"), "--unitigs-links", "--unitigs-gfa", P(t + ".gfa"), "--unitigs-map", str(q),
                      "--unitigs-map-out", P(t + ".gaf"), "--unitigs-min-count", str(min_count)]
    subprocess.run([_cli(), str(fasta), P("a.out")] + tail + outs("raw"), check=True, timeout=300)
    subprocess.run([_cli(), str(fasta), P("b.out")] + tail + outs("clip") + ["--unitigs-clip-tips", "--tip-report", P("r.tsv")],
                   check=True, timeout=300)
    read = lambda name: open(tmp_path / name, "rb").read()
    assert read("clip.fa") == lr.fasta_text_links(units, link_ptr, links)
    assert read("clip.gfa") == lr.gfa_text(units, k, link_ptr, links)
    assert read("clip.gaf") == hr.Graph(reduced, k, canonical, min_count).gaf_text(reads)
    assert read("r.tsv") == tr.report_text(report)
    assert read("raw.fa") == lr.fasta_text_links(raw, raw_ptr, raw_links)
    assert read("raw.gfa") == lr.gfa_text(raw, k, raw_ptr, raw_links)
    assert read("raw.gaf") == hr.Graph(table, k, canonical, min_count).gaf_text(reads)
    assert read("a.out") == read("b.out")                           # the counts' own output is what it is without the option
    if report[0][1]:
        assert read("clip.fa") != read("raw.fa")
    # the other options
    more = ["--unitigs-clip-tips", "--tip-max-kmers", "3", "--tip-ratio", "0", "--tip-rounds", "1", "--tip-report", P("r2.tsv")]
    subprocess.run([_cli(), str(fasta), P("c.out")] + tail + ["--unitigs-out", P("c.fa"), "--unitigs-min-count", str(min_count)] + more,
                   check=True, timeout=300)
    units2, report2, _ = tr.clip(table, k, canonical, min_count, 3, 0, rounds=1)
    assert read("c.fa") == ur.fasta_text(units2) and read("r2.tsv") == tr.report_text(report2)
