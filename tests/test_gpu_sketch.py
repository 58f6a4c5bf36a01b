"""GPU: the distinct sketch (cfrk_distinct_sketch / _device) against the numpy restatement of tests/sketch_ref.py --
registers byte for byte, windows exactly --, its accumulation, its errors, the estimate against the product's own exact
count, and the CLI's --estimate-only / --auto-hint."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from . import hash_craft as hc
from . import sketch_ref as sr

pytestmark = pytest.mark.gpu

CFRK_ERR_ARG, CFRK_ERR_LAYOUT, CFRK_ERR_ALIGN = -1, -5, -7
CANON = 0x2
KS = [1, 8, 12, 13, 16, 31, 32, 33, 48, 63, 64]
M = sr.M


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


def _dev_sketch(ctx, data, k, flags=0, regs0=None, want_windows=True, nN=None):
    """device form on a fresh device copy of data -> (registers, windows)"""
    data = np.ascontiguousarray(data, np.int8)
    nN = len(data) if nN is None else nN
    d_data, d_regs = ctx.alloc(len(data) + 64), ctx.alloc(M)
    try:
        ctx.h2d(d_data, data)
        ctx.h2d(d_regs, np.zeros(M, np.uint8) if regs0 is None else regs0)
        w = ctx.distinct_sketch_device(d_data, nN, k, flags, d_regs, want_windows)
        ctx.sync()
        regs = np.empty(M, np.uint8)
        ctx.d2h(regs, d_regs)
    finally:
        ctx.free(d_data)
        ctx.free(d_regs)
    return regs, w


def _same(got, want):
    regs, w = got
    wregs, ww = want
    assert w == ww
    bad = np.nonzero(regs != wregs)[0]
    assert len(bad) == 0, f"{len(bad)} registers differ, first {bad[:5]}: got {regs[bad[:5]]}, want {wregs[bad[:5]]}"


@pytest.fixture(scope="module")
def grid():
    """about 300 reads: a 5000-base read first (bytes 0 .. 4999: windows across the tile edges at 2048 and 4096 and
    across every 32-base lane-chunk edge), lengths 0 .. 400, one read per k of exactly k bases, scattered invalid codes"""
    rng = np.random.default_rng(4242)
    reads = [rng.integers(0, 4, 5000).astype(np.int8)]
    for L in rng.integers(0, 401, 280):
        r = rng.integers(0, 4, int(L)).astype(np.int8)
        r[rng.random(int(L)) < 0.01] = rng.choice(np.array([-1, 4, 78, -128], np.int8))
        reads.append(r)
    for k in KS:
        reads.append(rng.integers(0, 4, k).astype(np.int8))           # exactly k bases
    reads += [np.zeros(0, np.int8), np.array([2], np.int8), np.full(200, 3, np.int8), np.full(70, 0, np.int8)]
    data, start, length = sr.layout(reads)
    # a k = 64 window lies across each tile edge and across lane-chunk edges, with valid codes only
    for edge in (2048, 4096, 32, 64, 2048 + 32):
        assert ((data[edge - 63:edge + 64] >= 0) & (data[edge - 63:edge + 64] <= 3)).all()
    assert len(data) % 16 != 0 and (length < 8).any() and (length == 64).any()
    return data, start, length


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", KS)
def test_registers_and_windows_match_the_restatement(ctx, grid, k, canonical):
    data, start, length = grid
    flags = CANON if canonical else 0
    want = sr.sketch_of_reads(data, k, flags)
    assert want[1] > 5000 - k
    _same(_dev_sketch(ctx, data, k, flags), want)
    _same(ctx.distinct_sketch(data, k, flags, start, length), want)              # the host form, layout checked


@pytest.mark.parametrize("k", [8, 32, 33, 64])
def test_short_and_ragged_sizes(ctx, k):
    rng = np.random.default_rng(k)
    data = rng.integers(0, 4, 2100).astype(np.int8)
    for nN in (0, k - 1, k, 31, 33, 2047, 2049, 1000 + 7):
        for flags in (0, CANON):
            want = sr.sketch_of_reads(data[:nN], k, flags)
            assert want[1] == max(nN - k + 1, 0)
            _same(_dev_sketch(ctx, data, k, flags, nN=nN), want)                  # bases behind nN are not read as data
            _same(ctx.distinct_sketch(data[:nN], k, flags), want)


def test_all_t_key_at_k32_is_an_ordinary_key(ctx):
    regs, w = _dev_sketch(ctx, np.full(32, 3, np.int8), 32, 0)
    h = int(hc.mix(hc.ALL_ONES)[0])
    assert w == 1 and np.count_nonzero(regs) == 1 and regs[h >> 50] != 0
    _same((regs, w), sr.sketch_of_reads(np.full(32, 3, np.int8), 32, 0))


@pytest.mark.parametrize("k", [32, 64])
@pytest.mark.parametrize("bucket", [0, M - 1])
@pytest.mark.parametrize("rank, low", [(51, 0), (50, 1), (1, 1 << 49)])
def test_extreme_ranks(ctx, k, bucket, rank, low):
    """keys crafted through the inverse of the hash: the low 50 bits zero (rank 51), one (rank 50), top bit set (rank 1)"""
    import cfrk_amd
    h = np.uint64((bucket << 50) | low)
    if k == 32:
        lo, hi = int(hc.inv_mix(h)[0]), 0
        assert cfrk_amd.hash_info(lo, 0)[2] == int(h)
    else:
        hi = 0x0123456789ABCDEF ^ bucket ^ rank
        lo = int((hc.inv_mix(h) ^ hc.mix(hi))[0])
        assert cfrk_amd.hash_info(lo, hi)[3] == int(h)
    read = hc.key_to_read(lo, hi, k)
    regs, w = _dev_sketch(ctx, read, k, 0)
    assert w == 1 and np.count_nonzero(regs) == 1 and regs[bucket] == rank
    _same((regs, w), sr.sketch_of_reads(read, k, 0))


@pytest.mark.parametrize("k", [21, 32, 47, 64])
def test_reverse_complement_is_one_register_when_canonical(ctx, k):
    rng = np.random.default_rng(90 + k)
    while True:
        kmer = rng.integers(0, 4, k).astype(np.int8)
        rc = (3 - kmer[::-1]).astype(np.int8)
        fwd = sr.sketch_of_reads(np.concatenate([kmer, [-1], rc]), k, 0)[0]
        if np.count_nonzero(fwd) == 2:
            break
    data = np.concatenate([kmer, [-1], rc, [-1]]).astype(np.int8)
    regs, w = _dev_sketch(ctx, data, k, 0)
    assert w == 2 and np.count_nonzero(regs) == 2
    regs_c, w = _dev_sketch(ctx, data, k, CANON)
    assert w == 2 and np.count_nonzero(regs_c) == 1
    _same((regs_c, 2), sr.sketch_of_reads(data, k, CANON))


@pytest.mark.parametrize("k", [31, 63])
def test_accumulation(ctx, k):
    a = sr.genome_reads(1, 20000, 200, 150)
    b = sr.genome_reads(2, 20000, 170, 133)
    ra, wa = _dev_sketch(ctx, a, k, CANON)
    rb, wb = _dev_sketch(ctx, b, k, CANON)
    both, wab = _dev_sketch(ctx, b, k, CANON, regs0=ra)                           # two calls into one d_regs
    assert wab == wb                                                              # windows of THIS call
    assert (both == np.maximum(ra, rb)).all() and (both != ra).any() and (both != rb).any()
    _same(_dev_sketch(ctx, np.concatenate([a, b]), k, CANON), (both, wa + wb))    # = the sketch of the concatenation
    # the host form accumulates into the caller's registers as well
    rh, wh = ctx.distinct_sketch(b, k, CANON, regs=ra.copy())
    assert wh == wb and (rh == both).all()
    # preloaded registers larger than anything in the data survive
    pre = np.zeros(M, np.uint8)
    pre[::3] = 60
    pre[1::3] = 1
    got, _ = _dev_sketch(ctx, a, k, CANON, regs0=pre)
    assert (got == np.maximum(pre, ra)).all() and (got[::3] == 60).all()


def test_windows_out_may_be_null(ctx):
    data = sr.genome_reads(3, 5000, 50, 100)
    want = sr.sketch_of_reads(data, 31, 0)
    regs, w = _dev_sketch(ctx, data, 31, 0, want_windows=False)
    assert w is None and (regs == want[0]).all()
    import cfrk_amd
    L = cfrk_amd.load_library()
    regs = np.zeros(M, np.uint8)
    assert L.cfrk_distinct_sketch(ctx._h, data.ctypes.data_as(C.c_void_p), None, None, len(data), 0, 31, 0,
                                  regs.ctypes.data_as(C.c_void_p), None) == 0
    assert (regs == want[0]).all()


def test_errors(ctx):
    import cfrk_amd
    L = cfrk_amd.load_library()
    h = ctx._h
    data = np.zeros(64, np.int8)
    regs = np.zeros(M, np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    w = C.c_uint64(7)
    d, r = ctx.alloc(256), ctx.alloc(M)
    try:
        dev = lambda d_data, nN, k, flags, d_regs: L.cfrk_distinct_sketch_device(
            h, C.c_void_p(d_data) if d_data else None, nN, k, flags, C.c_void_p(d_regs) if d_regs else None, C.byref(w))
        assert dev(d, 64, 0, 0, r) == CFRK_ERR_ARG
        assert dev(d, 64, 65, 0, r) == CFRK_ERR_ARG
        assert dev(d, 64, 31, 0x1, r) == CFRK_ERR_ARG                            # CFRK_COMPAT: not a sketch flag
        assert dev(d, 64, 31, CANON | 0x4, r) == CFRK_ERR_ARG
        assert dev(d, 64, 31, 0, None) == CFRK_ERR_ARG
        assert dev(None, 64, 31, 0, r) == CFRK_ERR_ARG
        assert dev(d, -1, 31, 0, r) == CFRK_ERR_ARG
        assert dev(d + 1, 64, 31, 0, r) == CFRK_ERR_ALIGN
        assert dev(None, 0, 31, 0, None) == 0 and w.value == 0                   # nN = 0 is fine
        assert dev(d + 16, 32, 31, CANON, r) == 0
    finally:
        ctx.sync()
        ctx.free(d)
        ctx.free(r)
    host = lambda data_p, nN, k, flags, regs_p: L.cfrk_distinct_sketch(h, data_p, None, None, nN, 0, k, flags, regs_p, None)
    assert host(vp(data), 64, 0, 0, vp(regs)) == CFRK_ERR_ARG
    assert host(vp(data), 64, 65, 0, vp(regs)) == CFRK_ERR_ARG
    assert host(vp(data), 64, 31, 0x10, vp(regs)) == CFRK_ERR_ARG
    assert host(vp(data), 64, 31, 0, None) == CFRK_ERR_ARG
    assert host(None, 64, 31, 0, vp(regs)) == CFRK_ERR_ARG
    assert host(vp(data), -1, 31, 0, vp(regs)) == CFRK_ERR_ARG
    assert host(None, 0, 31, 0, None) == 0
    # layout checked like cfrk_global_add's
    dd, st, ln = sr.layout([np.zeros(10, np.int8), np.ones(10, np.int8)])
    st = st.copy()
    st[1] += 1
    with pytest.raises(cfrk_amd.CfrkError) as e:
        ctx.distinct_sketch(dd, 5, 0, st, ln)
    assert e.value.code == CFRK_ERR_LAYOUT


@pytest.mark.parametrize("k", [12, 31, 63])
def test_an_open_job_is_left_alone(ctx, k):
    import cfrk_amd
    data = sr.genome_reads(5, 20000, 400, 150)
    other = sr.genome_reads(6, 9000, 300, 90)
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, 100000)
    g.add(data)
    _same(ctx.distinct_sketch(other, 31, 0), sr.sketch_of_reads(other, 31, 0))   # before the job's first read-out
    before = g.digest()
    q = g.query_reads(data[:500])
    _same(ctx.distinct_sketch(other, k, CANON), sr.sketch_of_reads(other, k, CANON))
    _same(_dev_sketch(ctx, other, 63, 0), sr.sketch_of_reads(other, 63, 0))
    assert g.digest() == before and (g.query_reads(data[:500]) == q).all()
    g.add(other)                                                                  # and the job goes on
    fresh = cfrk_amd.GlobalCounter(cfrk_amd.Context(0), k, cfrk_amd.CFRK_CANONICAL, 100000)
    fresh.add(data)
    fresh.add(other)
    assert g.digest() == fresh.digest()
    fresh.ctx.close()


@pytest.mark.parametrize("k, flags", [(31, CANON), (63, 0)])
def test_estimate_against_the_exact_count(ctx, k, flags):
    """2 * 10^5 synthetic reads x 150 (genome 10^6): the estimate within four standard errors of what GlobalCounter
    counts, the hint at least the distinct keys, and a job begun with the hint does not overflow"""
    import cfrk_amd
    R, L = 200_000, 150
    nN = R * (L + 1)
    d, r = ctx.alloc(nN + 64), ctx.alloc(M)
    try:
        ctx.synth_reads_device(0, R, L, 1_000_000, d)
        ctx.h2d(r, np.zeros(M, np.uint8))
        windows = ctx.distinct_sketch_device(d, nN, k, flags, r)
        regs = np.empty(M, np.uint8)
        ctx.d2h(regs, r)
        est, hint = cfrk_amd.sketch_estimate(regs), cfrk_amd.sketch_hint(regs)
        g = cfrk_amd.GlobalCounter(ctx, k, flags, hint)
        g.add_device(d, nN)
        distinct = g.finish()                                                     # (CFRK_ERR_TABLE_FULL would raise)
        _, _, cnt = g.export()
    finally:
        ctx.sync()
        ctx.free(d)
        ctx.free(r)
    err = abs(est - distinct) / distinct
    print(f"k={k}: distinct {distinct}, estimate {est:.0f}, relative error {err:.5f}, hint {hint}, windows {windows}")
    assert windows == int(cnt.sum(dtype=np.uint64))
    assert err <= sr.BOUND
    assert hint >= distinct


# ------------------------------------------------------------------ CLI

def _cli():
    from .conftest import ROOT
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "cfrk_amd", "cfrk")


def _write_fasta(path, reads):
    """reads: uint8/int8 array [R, L] of codes 0..3"""
    R, L = reads.shape
    lines = np.empty((R, L + 4), np.uint8)
    lines[:, 0], lines[:, 1], lines[:, 2], lines[:, -1] = ord(">"), ord("r"), ord("\n"), ord("\n")
    lines[:, 3:-1] = np.frombuffer(b"ACGT", np.uint8)[reads]
    lines.tofile(str(path))


def _timing(stderr):
    return [json.loads(l[len("cfrk-timing "):]) for l in stderr.splitlines() if l.startswith("cfrk-timing ")][0]


def test_cli_estimate_only(tmp_path):
    cli = _cli()
    rng = np.random.default_rng(31)
    genome = rng.integers(0, 4, 30000)
    pos = rng.integers(0, 30000 - 120, 2000)
    reads = genome[pos[:, None] + np.arange(120)[None, :]]
    fa = tmp_path / "g.fasta"
    _write_fasta(fa, reads)
    data = np.full((2000, 121), -1, np.int8)
    data[:, :120] = reads
    for k, extra in ((31, ["--canonical"]), (63, []), (31, ["--canonical", "--gpus", "2", "--same-device"])):
        flags = CANON if "--canonical" in extra else 0
        regs, w = sr.sketch_of_reads(data.reshape(-1), k, flags)
        want = f"cfrk-estimate distinct={sr.estimate(regs):.0f} windows={w} hint={sr.hint(regs)}"
        out = tmp_path / "none.txt"
        p = subprocess.run([cli, str(fa), str(out), str(k), "--global", "--estimate-only"] + extra, capture_output=True,
                           text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        assert want in p.stderr.splitlines()
        assert not out.exists()
    # --estimate: the same line, and the count goes on as usual
    out1, out2 = tmp_path / "a.txt", tmp_path / "b.txt"
    p = subprocess.run([cli, str(fa), str(out1), "31", "--global", "--canonical", "--estimate"], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0 and want in p.stderr.splitlines()
    subprocess.run([cli, str(fa), str(out2), "31", "--global", "--canonical"], check=True, timeout=300)
    assert out1.read_bytes() == out2.read_bytes() and out1.stat().st_size > 0


@pytest.mark.parametrize("k", [5, 16])
def test_cli_auto_hint_output_is_identical_on_the_golden_fasta(tmp_path, derived_fasta, k):
    cli = _cli()
    for name in ("seq1", "seq2"):
        for extra in ([], ["--gpus", "2", "--same-device"]):
            a, b = tmp_path / "plain.txt", tmp_path / "auto.txt"
            base = [cli, derived_fasta[name]]
            subprocess.run(base + [str(a), str(k), "--global"] + extra, check=True, timeout=300)
            p = subprocess.run(base + [str(b), str(k), "--global", "--auto-hint", "--timing"] + extra, capture_output=True,
                               text=True, timeout=300)
            assert p.returncode == 0, p.stderr
            assert a.read_bytes() == b.read_bytes()
            t = _timing(p.stderr)
            assert t["attempts"] == 1 and t["hint"] >= 1 << 20 and t["distinct_estimate"] > 0 and t["estimate_s"] >= 0


def test_cli_auto_hint_saves_the_retry_on_all_distinct_reads(tmp_path):
    """1.2 * 10^5 uniform random reads x 150 at k = 31: 1.4 * 10^7 distinct k-mers against the 1.1 * 10^6 that nN / 16
    announces -- the plain run counts more than once, --auto-hint once, and both write the same file"""
    cli = _cli()
    rng = np.random.default_rng(77)
    fa = tmp_path / "u.fasta"
    _write_fasta(fa, rng.integers(0, 4, (120_000, 150), dtype=np.uint8))
    a, b = tmp_path / "plain.bin", tmp_path / "auto.bin"
    base = [cli, str(fa)]
    p = subprocess.run(base + [str(a), "31", "--global", "--binary", "--timing"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    plain = _timing(p.stderr)
    p = subprocess.run(base + [str(b), "31", "--global", "--binary", "--timing", "--auto-hint"], capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    auto = _timing(p.stderr)
    print("plain:", plain, "\nauto:", auto)
    assert plain["attempts"] >= 2
    assert auto["attempts"] == 1
    assert auto["entries"] == plain["entries"] > 10_000_000 and auto["hint"] >= auto["entries"]
    assert a.stat().st_size == b.stat().st_size
    with open(a, "rb") as fa_, open(b, "rb") as fb_:
        while True:
            x, y = fa_.read(1 << 24), fb_.read(1 << 24)
            assert x == y
            if not x:
                break
