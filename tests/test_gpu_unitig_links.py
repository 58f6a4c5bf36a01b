"""GPU: the links between the unitigs of a finished global result (cfrk_global_unitig_links and its device form) against
tests/unitig_links_ref.py, a dictionary-and-strings statement of the contract that shares nothing with the product: the
k grid of the unitig tests on both strand rules and two thresholds, byte for byte; the k = 32 all-T key; a 300 000-node
chain and ring (the call does not walk); the capacity protocol and the argument checks; the consistency check on three
inputs the definition guarantees it catches; the CLI's L tags and GFA."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from . import oracle_lib as orc
from . import unitig_links_ref as lr
from . import unitig_ref as ur
from .test_gpu_filter import _Guarded, _upload
from .test_gpu_query import _cli
from .test_gpu_unitigs import KS, _device_unitigs, _input, _job, _table

pytestmark = pytest.mark.gpu

CFRK_ERR_ARG, CFRK_ERR_STATE, CFRK_ERR_LAYOUT, CFRK_ERR_SMALL_BUF = -1, -4, -5, -9


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


_REF = {}


def _ref(k, canonical, min_count):
    """(units, layout, link_ptr, links) of the grid input, computed once"""
    key = (k, canonical, min_count)
    if key not in _REF:
        table = _table(_input(k), k, canonical)
        units = ur.unitigs(table, k, canonical, min_count)
        _REF[key] = (units, ur.layout(units)) + lr.links(units, table, k, canonical, min_count)
    return _REF[key]


class _DeviceUnitigs:
    """a unitig list on the device, the data `skew` bytes off a 64-byte boundary"""

    def __init__(self, ctx, data, start, length, skew=0):
        self.ctx, self.nN, self.nS = ctx, len(data), len(length)
        self.base = [_upload(ctx, np.ascontiguousarray(data, np.int8), skew), _upload(ctx, np.ascontiguousarray(start, np.int64)),
                     _upload(ctx, np.ascontiguousarray(length, np.int32))]
        self.args = (self.base[0] + skew, self.base[1], self.base[2], self.nN, self.nS)

    def free(self):
        for p in self.base:
            self.ctx.free(p)


def _device_links(ctx, g, min_count, data, start, length, skew=0):
    """the device form into guarded arrays of exactly the size a sizes-only call reported -> (link_ptr, links)"""
    import cfrk_amd
    d = _DeviceUnitigs(ctx, data, start, length, skew)
    ptr = _Guarded(ctx, (d.nS + 1) * 8)
    try:
        n = g.unitig_links_device(min_count, *d.args, ptr.ptr, 0, 0)
    except cfrk_amd.CfrkError as e:
        assert e.code == CFRK_ERR_SMALL_BUF
        n = e.n_links
    ctx.sync()
    sized = ptr.fetch((d.nS + 1) * 8, np.int64)
    rows = _Guarded(ctx, n * 8)
    ptr2 = _Guarded(ctx, (d.nS + 1) * 8)
    assert g.unitig_links_device(min_count, *d.args, ptr2.ptr, rows.ptr, n) == n
    ctx.sync()
    link_ptr, links = ptr2.fetch((d.nS + 1) * 8, np.int64), rows.fetch(n * 8, cfrk_amd.UNITIG_LINK_DTYPE)
    assert (sized == link_ptr).all()                            # the sizes-only call left link_ptr complete
    for b in (ptr, ptr2, rows):
        b.free()
    d.free()
    return link_ptr, links


def _same_links(got, want):
    for name, a, b in zip(("link_ptr", "links"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), name


# ------------------------------------------------------------------ the grid

@pytest.mark.parametrize("min_count", [1, 2])
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", KS)
def test_unitig_links(ctx, k, canonical, min_count):
    units, layout, want_ptr, want = _ref(k, canonical, min_count)
    g = _job(ctx, _input(k), k, canonical)
    digest = g.digest()
    data, start, length, rec = _device_unitigs(ctx, g, min_count)
    assert (data == layout[0]).all() and (length == layout[2]).all()
    _same_links(_device_links(ctx, g, min_count, data, start, length, skew=3), (want_ptr, want))
    _same_links(g.unitig_links(data, start, length, min_count), (want_ptr, want))
    assert g.digest() == digest
    if min_count == 1:
        _same_links(g.unitig_links(data, start, length, 0), (want_ptr, want))     # 0 reads as 1


def test_unitig_links_k32_all_t(ctx):
    """the all-T key (the table's side word) is an ordinary end k-mer: one node that follows itself"""
    seqs = [("T" * 40, 2)]
    table = _table(seqs, 32, False)
    assert table == {"T" * 32: 18}
    units = ur.unitigs(table, 32, False, 1)
    assert [u[0] for u in units] == ["T" * 32]
    want = lr.links(units, table, 32, False, 1)
    assert want[0].tolist() == [0, 1] and want[1].tolist() == [(0, 0)]
    g = _job(ctx, seqs, 32, False)
    data, start, length, rec = g.unitigs(1)
    assert rec.tolist() == [(18, 1, 0)]
    _same_links(g.unitig_links(data, start, length), want)
    _same_links(_device_links(ctx, g, 1, data, start, length, skew=1), want)


# ------------------------------------------------------------------ a long chain and a long ring: nothing is walked

@pytest.fixture(scope="module")
def long_genome():
    return np.random.default_rng(31).integers(0, 4, 300000).astype(np.int8)


def test_long_chain_has_no_links(ctx, long_genome):
    import cfrk_amd
    G = long_genome
    g = cfrk_amd.GlobalCounter(ctx, 31, cfrk_amd.CFRK_CANONICAL, 400000)
    g.add(np.append(G, np.int8(-1)))
    data, start, length, rec = g.unitigs(1)
    assert list(length) == [len(G)] and rec.tolist() == [(len(G) - 30, len(G) - 30, 0)]
    link_ptr, links = g.unitig_links(data, start, length)
    assert link_ptr.tolist() == [0, 0] and len(links) == 0
    _same_links(_device_links(ctx, g, 1, data, start, length), (link_ptr, links))


def test_long_ring_has_its_two_self_links(ctx, long_genome):
    import cfrk_amd
    G = long_genome
    g = cfrk_amd.GlobalCounter(ctx, 31, cfrk_amd.CFRK_CANONICAL, 400000)
    g.add(np.concatenate([G, G[:30], [np.int8(-1)]]).astype(np.int8))
    data, start, length, rec = g.unitigs(1)
    assert list(length) == [len(G) + 30] and rec.tolist() == [(len(G), len(G), cfrk_amd.CFRK_UNITIG_CIRCULAR)]
    link_ptr, links = g.unitig_links(data, start, length)
    assert link_ptr.tolist() == [0, 2]
    assert links.tolist() == [(0, 0), (0, cfrk_amd.CFRK_LINK_FROM_MINUS | cfrk_amd.CFRK_LINK_TO_MINUS)]
    _same_links(_device_links(ctx, g, 1, data, start, length, skew=5), (link_ptr, links))


# ------------------------------------------------------------------ protocol

def test_unitig_links_protocol(ctx):
    import cfrk_amd
    k, canonical, min_count = 21, True, 1
    units, (data, start, length, rec), want_ptr, want = _ref(k, canonical, min_count)
    nS, n = len(units), len(want)
    assert n > 1
    g = _job(ctx, _input(k), k, canonical)
    digest = g.digest()
    L, h = ctx._L, ctx._h
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    out = C.c_int64(-1)
    # sizes only, host form: link_ptr complete, the count reported
    ptr = np.full(nS + 1, -1, np.int64)
    host = (h, min_count, vp(data), vp(start), vp(length), len(data), nS)
    assert L.cfrk_global_unitig_links(*host, vp(ptr), None, 0, C.byref(out)) == CFRK_ERR_SMALL_BUF
    assert out.value == n and ptr.tobytes() == want_ptr.tobytes()
    # one row short, host form: link_ptr complete, the rows untouched
    ptr[:] = -1
    rows = np.full(n - 1, 0x5A5A5A5A, np.uint64)
    assert L.cfrk_global_unitig_links(*host, vp(ptr), vp(rows), n - 1, C.byref(out)) == CFRK_ERR_SMALL_BUF
    assert out.value == n and ptr.tobytes() == want_ptr.tobytes() and (rows == 0x5A5A5A5A).all()
    # device form: sizes only, then one row short into guarded arrays
    d = _DeviceUnitigs(ctx, data, start, length, skew=7)
    for cap in (0, n - 1):
        d_ptr, d_rows = _Guarded(ctx, (nS + 1) * 8), _Guarded(ctx, cap * 8)
        with pytest.raises(cfrk_amd.CfrkError) as e:
            g.unitig_links_device(min_count, *d.args, d_ptr.ptr, d_rows.ptr if cap else 0, cap)
        assert e.value.code == CFRK_ERR_SMALL_BUF and e.value.n_links == n
        ctx.sync()
        assert d_ptr.fetch((nS + 1) * 8, np.int64).tobytes() == want_ptr.tobytes()
        d_rows.fetch(0)                                         # nothing written: every byte is still a guard byte
        d_ptr.free()
        d_rows.free()
    # room to spare
    d_ptr, d_rows = _Guarded(ctx, (nS + 1) * 8), _Guarded(ctx, (n + 5) * 8)
    assert g.unitig_links_device(min_count, *d.args, d_ptr.ptr, d_rows.ptr, n + 5) == n
    ctx.sync()
    assert d_rows.fetch(n * 8).tobytes() == want.tobytes()
    # nS = 0: link_ptr[0] = 0 and no links, with NULL inputs
    d_one = _Guarded(ctx, 8)
    assert g.unitig_links_device(min_count, 0, 0, 0, 0, 0, d_one.ptr, 0, 0) == 0
    ctx.sync()
    assert d_one.fetch(8, np.int64).tolist() == [0]
    d_one.free()
    ptr[:] = -1
    assert L.cfrk_global_unitig_links(h, min_count, None, None, None, 0, 0, vp(ptr), None, 0, C.byref(out)) == 0
    assert out.value == 0 and ptr[0] == 0 and (ptr[1:] == -1).all()
    e_ptr, e_links = g.unitig_links(np.zeros(0, np.int8), np.zeros(0, np.int64), np.zeros(0, np.int32))
    assert e_ptr.tolist() == [0] and len(e_links) == 0
    # CFRK_ERR_ARG, one case per clause, on both forms
    dev = (h, min_count) + d.args
    p, r = C.c_void_p(d_ptr.ptr), C.c_void_p(d_rows.ptr)
    for fn, a, lp, ln in ((L.cfrk_global_unitig_links, host, vp(ptr), vp(rows)), (L.cfrk_global_unitig_links_device, dev, p, r)):
        hd, mc, da, st, le, nN, ns = a
        cap = n + 5 if fn is L.cfrk_global_unitig_links_device else n - 1
        assert fn(hd, mc, da, st, le, -1, ns, lp, ln, cap, C.byref(out)) == CFRK_ERR_ARG         # negative sizes
        assert fn(hd, mc, da, st, le, nN, -1, lp, ln, cap, C.byref(out)) == CFRK_ERR_ARG
        assert fn(hd, mc, da, st, le, nN, ns, lp, ln, cap, None) == CFRK_ERR_ARG                 # NULL n_links_out
        assert fn(hd, mc, da, st, le, nN, ns, None, ln, cap, C.byref(out)) == CFRK_ERR_ARG       # NULL link_ptr
        assert fn(hd, mc, None, st, le, nN, ns, lp, ln, cap, C.byref(out)) == CFRK_ERR_ARG       # NULL data / start / length
        assert fn(hd, mc, da, None, le, nN, ns, lp, ln, cap, C.byref(out)) == CFRK_ERR_ARG
        assert fn(hd, mc, da, st, None, nN, ns, lp, ln, cap, C.byref(out)) == CFRK_ERR_ARG
        assert fn(hd, mc, da, st, le, nN, ns, lp, None, 1, C.byref(out)) == CFRK_ERR_ARG         # NULL links with room
        assert fn(hd, mc, da, st, le, nN, 1 << 32, lp, ln, cap, C.byref(out)) == CFRK_ERR_ARG    # nS >= 2^32
    ctx.sync()
    d_ptr.free()
    d_rows.free()
    d.free()
    assert g.digest() == digest
    # adds may follow
    g.add(np.array([0, 1, 2, 3] * 10 + [-1], np.int8))


def test_unitig_links_need_a_job():
    import cfrk_amd
    one = np.zeros(2, np.int64)
    out = C.c_int64()
    args = (1, None, None, None, 0, 0, one.ctypes.data_as(C.c_void_p), None, 0, C.byref(out))
    with cfrk_amd.Context(0) as c:
        assert c._L.cfrk_global_unitig_links(c._h, *args) == CFRK_ERR_STATE
        assert c._L.cfrk_global_unitig_links_device(c._h, *args) == CFRK_ERR_STATE
        reads, _, _ = orc.synth_reads(0, 2000, 150, 20000)
        g = cfrk_amd.GlobalCounter(c, 31, cfrk_amd.CFRK_CANONICAL | cfrk_amd.CFRK_RUNS_ONLY, 100000)
        g.add(reads)
        assert c._L.cfrk_global_unitig_links(c._h, *args) == CFRK_ERR_STATE
        assert c._L.cfrk_global_unitig_links_device(c._h, *args) == CFRK_ERR_STATE


# ------------------------------------------------------------------ the consistency check

def _refused(ctx, g, min_count, data, start, length, unitig):
    """the device form refuses the list with CFRK_ERR_LAYOUT naming `unitig`, and writes nothing outside its arrays"""
    import cfrk_amd
    d = _DeviceUnitigs(ctx, data, start, length, skew=2)
    room = 16 * d.nS
    d_ptr, d_rows = _Guarded(ctx, (d.nS + 1) * 8), _Guarded(ctx, room * 8)
    with pytest.raises(cfrk_amd.CfrkError) as e:
        g.unitig_links_device(min_count, *d.args, d_ptr.ptr, d_rows.ptr, room)
    assert e.value.code == CFRK_ERR_LAYOUT
    assert ("unitig %d " % unitig) in str(e.value)
    ctx.sync()
    d_ptr.fetch((d.nS + 1) * 8)                                 # (unspecified inside, intact around)
    d_rows.fetch(room * 8)
    d_ptr.free()
    d_rows.free()
    d.free()


def _first_missed(units, table, k, canonical):
    """the first unitig with a solid successor of a tail that no oriented unitig of the list begins with"""
    oris = (0, 1) if canonical else (0,)
    heads = {u[0][:k] if o == 0 else ur.rc(u[0][-k:]) for u in units for o in oris}
    for j, u in enumerate(units):
        for o in oris:
            a = u[0][-k:] if o == 0 else ur.rc(u[0][:k])
            for b in ur.BASES:
                z = a[1:] + b
                if (min(z, ur.rc(z)) if canonical else z) in table and z not in heads:
                    return j
    return None


@pytest.mark.parametrize("k, canonical", [(12, True), (21, True), (40, False)])
def test_unitig_links_consistency_check(ctx, k, canonical):
    units, (data, start, length, rec), want_ptr, want = _ref(k, canonical, 1)
    table = _table(_input(k), k, canonical)
    g = _job(ctx, _input(k), k, canonical)
    _same_links(_device_links(ctx, g, 1, data, start, length), (want_ptr, want))
    # a multi-k-mer unitig shortened by its last base: the new tail's successor is an interior k-mer, the head of nothing
    j = next(i for i, u in enumerate(units) if u[2] >= 3 and not u[3])
    cut = list(units)
    cut[j] = (units[j][0][:-1], units[j][1], units[j][2] - 1, False)
    with pytest.raises(AssertionError):                         # the reference misses the head as well
        lr.oriented_links(cut, table, k, canonical, 1)
    short = length.copy()
    short[j] -= 1
    _refused(ctx, g, 1, data, start, short, _first_missed(cut, table, k, canonical))
    # an invalid code in the last window
    bad = data.copy()
    bad[start[j] + length[j] - 2] = 4
    _refused(ctx, g, 1, bad, start, length, j)
    # a unitig of k - 1 bases
    short = length.copy()
    short[j] = k - 1
    _refused(ctx, g, 1, data, start, short, j)
    # ranges outside [0, nN) are offending unitigs, not accesses
    far = start.copy()
    far[j] = len(data) - 1
    _refused(ctx, g, 1, data, far, length, j)
    far[j] = -5
    _refused(ctx, g, 1, data, far, length, j)
    # the host form refuses the shortened unitig as well (its terminator is gone: the layout check)
    import cfrk_amd
    short = length.copy()
    short[j] -= 1
    with pytest.raises(cfrk_amd.CfrkError) as e:
        g.unitig_links(data, start, short)
    assert e.value.code == CFRK_ERR_LAYOUT
    with pytest.raises(cfrk_amd.CfrkError) as e:
        g.unitig_links(bad, start, length)
    assert e.value.code == CFRK_ERR_LAYOUT and ("unitig %d " % j) in str(e.value)


# ------------------------------------------------------------------ CLI

@pytest.mark.parametrize("k,canonical,min_count", [(5, False, 1), (21, True, 1), (31, True, 2), (40, False, 2)])
def test_cli_unitig_links(tmp_path, k, canonical, min_count):
    seqs = _input(k)
    fasta = tmp_path / "in.fa"
    with open(fasta, "w") as f:
        i = 0
        for s, t in seqs:
            for _ in range(t):
                f.write(">r%d\n%s\n" % (i, s))
                i += 1
    table = _table(seqs, k, canonical)
    units = ur.unitigs(table, k, canonical, min_count)
    link_ptr, links = lr.links(units, table, k, canonical, min_count)
    head = [_cli(), str(fasta)]
    tail = [str(k), "--global"] + (["--canonical"] if canonical else [])
    mc = ["--unitigs-min-count", str(min_count)]
    run = lambda out, more: subprocess.run(head + [str(tmp_path / out)] + tail + more, check=True, timeout=300)
    run("b.out", ["--unitigs-out", str(tmp_path / "plain.fa")] + mc)
    run("c.out", ["--unitigs-out", str(tmp_path / "tags.fa"), "--unitigs-links", "--unitigs-gfa", str(tmp_path / "both.gfa")] + mc)
    run("d.out", ["--unitigs-gfa", str(tmp_path / "alone.gfa")] + mc)
    read = lambda name: open(tmp_path / name, "rb").read()
    assert read("plain.fa") == ur.fasta_text(units)
    assert read("tags.fa") == lr.fasta_text_links(units, link_ptr, links)
    assert read("both.gfa") == lr.gfa_text(units, k, link_ptr, links) == read("alone.gfa")
    assert read("b.out") == read("c.out") == read("d.out")       # the counts' own output is what it is without the options
