"""GPU: the abundance histogram (k-mer spectrum, cfrk_global_histogram) and the count-range export
(cfrk_global_export_range) against the oracle on every counting path, and the CLI's --histo / --histo-only /
--min-count / --max-count.  References are numpy over tests.oracle_lib.global_count."""
import os
import subprocess

import numpy as np
import pytest

from . import oracle_lib as orc
from . import refsem

pytestmark = pytest.mark.gpu

CFRK_ERR_ARG, CFRK_ERR_STATE, CFRK_ERR_SMALL_BUF = -1, -4, -9


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


def _random_reads(rng, n, lo, hi, p_invalid=0.02):
    reads = []
    for L in rng.integers(lo, hi, n):
        r = rng.integers(0, 4, int(L)).astype(np.int8)
        if p_invalid:
            r[rng.random(int(L)) < p_invalid] = -1
        reads.append(r)
    return reads


def _want_hist(wcnt, nbins):
    c = np.minimum(np.asarray(wcnt, np.uint64), nbins - 1).astype(np.int64)
    return np.bincount(c, minlength=nbins).astype(np.uint64)


def _oracle(data, k, canonical):
    return orc.global_count(data, k, orc.ORC_CANONICAL if canonical else 0)


def _check_hist(g, wcnt, nbins_list=(2, 8, 300)):
    for nb in nbins_list:
        h = g.histogram(nb)
        assert h.dtype == np.uint64 and len(h) == nb
        assert (h == _want_hist(wcnt, nb)).all(), nb
        assert h[0] == 0 and int(h.sum()) == len(wcnt)


# ------------------------------------------------------------------ histogram

@pytest.mark.parametrize("k", [1, 2, 5, 7, 8, 12, 15, 16, 17, 21, 26, 27, 31, 32, 33, 40, 47, 48, 55, 63, 64])
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("force_hash", [False, True])
def test_histogram_vs_oracle(ctx, k, canonical, force_hash):
    import cfrk_amd
    rng = np.random.default_rng(200 + k)
    reads = _random_reads(rng, 400, 1, 300)
    reads.append(np.full(200, 3, np.int8))      # poly-T: the all-ones key at k = 32 (held beside the table)
    reads.append(np.full(200, 0, np.int8))      # poly-A
    reads.append(np.zeros(0, np.int8))
    data, start, length = refsem.flatten(reads)
    flags = (cfrk_amd.CFRK_CANONICAL if canonical else 0) | (cfrk_amd.CFRK_FORCE_HASH if force_hash else 0)
    g = cfrk_amd.GlobalCounter(ctx, k, flags, 0)
    g.add(data, start, length)
    wlo, whi, wcnt = _oracle(data, k, canonical)
    _check_hist(g, wcnt)
    assert g.digest() == orc.digest(wlo, whi, wcnt, two_word=k > 32)
    _check_hist(g, wcnt, (5,))                  # (read-only: again after the digest)


@pytest.mark.parametrize("canonical", [False, True])
def test_histogram_k16_on_the_partitioned_path(ctx, canonical):
    import cfrk_amd
    rng = np.random.default_rng(216)
    reads = _random_reads(rng, 3000, 1, 300)
    reads.append(np.full(200, 0, np.int8))
    data, start, length = refsem.flatten(reads)
    g = cfrk_amd.GlobalCounter(ctx, 16, cfrk_amd.CFRK_CANONICAL if canonical else 0, 1 << 20)
    g.set_debug_flags(cfrk_amd.CFRK_DEBUG_NO_RADIX16)
    try:
        g.add(data, start, length)
        assert g.msp_info()["l2_records"] > 0
        wlo, whi, wcnt = _oracle(data, 16, canonical)
        _check_hist(g, wcnt)
        assert g.digest() == orc.digest(wlo, whi, wcnt)
    finally:
        g.set_debug_flags(0)


@pytest.mark.parametrize("k", [40, 63])
def test_histogram_with_leaves_shared_by_record(ctx, k):
    import cfrk_amd
    R, L, G = 20000, 150, 200_000
    data, _, _ = orc.synth_reads(0, R, L, G)
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, 2 * G)
    g.set_debug_flags(cfrk_amd.lib.CFRK_DEBUG_RECORD_SUBSETS)
    try:
        g.add(data)
    finally:
        g.set_debug_flags(0)
    wlo, whi, wcnt = _oracle(data, k, True)
    _check_hist(g, wcnt)
    assert g.digest() == orc.digest(wlo, whi, wcnt, two_word=True)


def test_histogram_after_two_adds_fold_into_the_table(ctx):
    import cfrk_amd
    d1, _, _ = orc.synth_reads(0, 4000, 150, 30000)
    d2, _, _ = orc.synth_reads(4000, 4000, 150, 30000)
    g = cfrk_amd.GlobalCounter(ctx, 25, cfrk_amd.CFRK_CANONICAL, 100000)
    g.add(d1)
    _check_hist(g, _oracle(d1, 25, True)[2], (300,))
    g.add(d2)
    wlo, whi, wcnt = _oracle(np.concatenate([d1, d2]), 25, True)
    _check_hist(g, wcnt)
    assert g.digest() == orc.digest(wlo, whi, wcnt)


@pytest.mark.parametrize("k", [31, 63])
def test_histogram_of_merged_input(ctx, k):
    import cfrk_amd
    data, _, _ = orc.synth_reads(0, 3000, 150, 20000)
    wlo, whi, wcnt = _oracle(data, k, True)
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, 100000)
    cnt32 = wcnt.astype(np.uint32)
    d_lo, d_hi, d_cnt = ctx.alloc(wlo.nbytes), ctx.alloc(whi.nbytes), ctx.alloc(cnt32.nbytes)
    try:
        ctx.h2d(d_lo, wlo); ctx.h2d(d_hi, whi); ctx.h2d(d_cnt, cnt32)
        g.merge_device(d_lo, d_hi if k > 32 else 0, d_cnt, len(wlo))
        ctx.sync()
    finally:
        ctx.free(d_lo); ctx.free(d_hi); ctx.free(d_cnt)
    _check_hist(g, wcnt)
    assert g.digest() == orc.digest(wlo, whi, wcnt, two_word=k > 32)


@pytest.mark.parametrize("k", [31, 63])
@pytest.mark.parametrize("force_hash", [False, True])
def test_histogram_counts_beyond_the_lds_bins_land_in_their_own_bin(ctx, k, force_hash):
    """a poly-A read of 20000 bases: one key counted ~20000 times, above the 16384 bins a workgroup keeps in LDS --
    with nbins = 2^16 + 1 it lands in its exact bin through the global atomics, with 16385 in the top bin"""
    import cfrk_amd
    rng = np.random.default_rng(77 + k)
    reads = _random_reads(rng, 2000, 50, 300)
    reads.append(np.zeros(20000, np.int8))
    data, start, length = refsem.flatten(reads)
    flags = cfrk_amd.CFRK_CANONICAL | (cfrk_amd.CFRK_FORCE_HASH if force_hash else 0)
    g = cfrk_amd.GlobalCounter(ctx, k, flags, 0)
    g.add(data, start, length)
    wlo, whi, wcnt = _oracle(data, k, True)
    big = int(wcnt.max())
    assert big == 20000 - k + 1 > 16384
    h = g.histogram(2 ** 16 + 1)
    assert h[big] == 1 and (h == _want_hist(wcnt, 2 ** 16 + 1)).all()
    h = g.histogram(16385)
    assert h[16384] == 1 and (h == _want_hist(wcnt, 16385)).all()


@pytest.mark.parametrize("k", [31, 63])
def test_histogram_and_range_export_of_saturated_counts(ctx, k):
    import cfrk_amd
    two = k > 32
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, 1024)
    keys = np.array([0, 5, 77, 0, 0, 5], np.uint64)
    his = np.array([0, 1, 2, 0, 0, 1], np.uint64)
    cnts = np.array([0x60000000, 7, 0xFFFFFFF0, 0x60000000, 0x60000000, 8], np.uint32)
    for i in range(0, 6, 2):
        d_lo, d_hi, d_cnt = ctx.alloc(16), ctx.alloc(16), ctx.alloc(8)
        ctx.h2d(d_lo, keys[i:i + 2]); ctx.h2d(d_hi, his[i:i + 2]); ctx.h2d(d_cnt, cnts[i:i + 2])
        g.merge_device(d_lo, d_hi if two else 0, d_cnt, 2)
        ctx.sync()
        ctx.free(d_lo); ctx.free(d_hi); ctx.free(d_cnt)
    with pytest.raises(cfrk_amd.CfrkError) as e:
        g.histogram(300)
    assert e.value.code == cfrk_amd.CFRK_ERR_COUNT_OVERFLOW
    h = g.histogram(300, allow_saturated=True)
    want = np.zeros(300, np.uint64)
    want[15] = 1
    want[299] = 2                                           # 0xFFFFFFF0 and the saturated key
    assert (h == want).all()
    h = g.histogram(1 << 24, allow_saturated=True)
    assert h[15] == 1 and h[(1 << 24) - 1] == 2 and int(h.sum()) == 3
    lo, hi, cnt = g.export(allow_saturated=True, min_count=cfrk_amd.CFRK_COUNT_MAX)
    assert list(lo) == [0] and list(hi) == [0] and list(cnt) == [cfrk_amd.CFRK_COUNT_MAX]
    with pytest.raises(cfrk_amd.CfrkError) as e:
        g.export(min_count=cfrk_amd.CFRK_COUNT_MAX)
    assert e.value.code == cfrk_amd.CFRK_ERR_COUNT_OVERFLOW


def test_histogram_at_scale_sums_to_the_digest(ctx):
    """10^6 reads of configs[2]'s generator, k = 31 canonical"""
    import cfrk_amd
    R, L, G, k = 1_000_000, 150, 100_000_000, 31
    nN = R * (L + 1)
    d = ctx.alloc(nN)
    ctx.synth_reads_device(0, R, L, G, d)
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, R * (L - k + 1))
    g.add_device(d, nN)
    host = np.empty(nN, np.int8)
    ctx.d2h(host, d)
    ctx.free(d)
    wlo, whi, wcnt = orc.global_count(host, k, orc.ORC_CANONICAL, threads=8)
    nb = int(wcnt.max()) + 2
    h = g.histogram(nb)
    assert (h == _want_hist(wcnt, nb)).all()
    dg = g.digest()
    assert int(h.sum()) == dg[0]
    assert int((np.arange(nb, dtype=np.uint64) * h).sum()) == dg[1]
    assert (g.histogram(16385) == _want_hist(wcnt, 16385)).all()


def test_histogram_errors(ctx):
    import ctypes as C
    import cfrk_amd
    L = cfrk_amd.load_library()
    h = np.zeros(8, np.uint64)
    fresh = cfrk_amd.Context(0)
    try:
        assert L.cfrk_global_histogram(fresh._h, h.ctypes.data_as(C.c_void_p), 8) == CFRK_ERR_STATE
        n = C.c_uint64()
        assert L.cfrk_global_export_range(fresh._h, 1, 9, None, None, None, 0, C.byref(n)) == CFRK_ERR_STATE
    finally:
        fresh.close()
    data, _, _ = orc.synth_reads(0, 2000, 150, 20000)
    g = cfrk_amd.GlobalCounter(ctx, 31, cfrk_amd.CFRK_CANONICAL | cfrk_amd.CFRK_RUNS_ONLY, 100000)
    g.add(data)
    with pytest.raises(cfrk_amd.CfrkError) as e:
        g.histogram(8)
    assert e.value.code == CFRK_ERR_STATE
    with pytest.raises(cfrk_amd.CfrkError) as e:
        g.export(min_count=2)
    assert e.value.code == CFRK_ERR_STATE
    g = cfrk_amd.GlobalCounter(ctx, 31, cfrk_amd.CFRK_CANONICAL, 100000)
    g.add(data)
    for nb in (0, 1, (1 << 24) + 1, 1 << 31):
        with pytest.raises(cfrk_amd.CfrkError) as e:
            g.histogram(nb)
        assert e.value.code == CFRK_ERR_ARG, nb
    assert L.cfrk_global_histogram(ctx._h, None, 8) == CFRK_ERR_ARG
    _check_hist(g, _oracle(data, 31, True)[2], (2, 1 << 24))


# ------------------------------------------------------------------ count-range export

@pytest.mark.parametrize("k", [7, 15, 31, 63])
@pytest.mark.parametrize("canonical", [False, True])
def test_range_export_vs_oracle(ctx, k, canonical):
    import cfrk_amd
    MAX = cfrk_amd.CFRK_COUNT_MAX
    rng = np.random.default_rng(500 + k)
    d1, _, _ = orc.synth_reads(0, 3000, 150, 30000)
    reads = _random_reads(rng, 500, 1, 300)
    reads.append(np.full(200, 3, np.int8))
    d2, _, _ = refsem.flatten(reads)
    data = np.concatenate([d1, d2])
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL if canonical else 0, 0)
    g.add(data)
    wlo, whi, wcnt = _oracle(data, k, canonical)
    full = g.export()
    assert (full[0] == wlo).all() and (full[1] == whi).all() and (full[2].astype(np.uint64) == wcnt).all()
    for mn, mx in [(0, MAX), (2, MAX), (1, 1), (3, 7), (8, 2)]:
        m = (wcnt >= max(mn, 1)) & (wcnt <= mx)
        lo, hi, cnt = g.export(min_count=mn, max_count=mx)
        assert len(lo) == int(m.sum()), (mn, mx)
        assert (lo == wlo[m]).all() and (hi == whi[m]).all() and (cnt.astype(np.uint64) == wcnt[m]).all()
        if (mn, mx) == (0, MAX):
            assert all((a == b).all() for a, b in zip((lo, hi, cnt), full))
        kept = int(m.sum())
        if kept:
            with pytest.raises(cfrk_amd.CfrkError) as e:
                g.export_range(mn, mx, kept - 1)
            assert e.value.code == CFRK_ERR_SMALL_BUF and e.value.n_out == kept
            lo2, hi2, cnt2 = g.export_range(mn, mx, kept)
            assert (lo2 == lo).all() and (hi2 == hi).all() and (cnt2 == cnt).all()
    assert g.digest() == orc.digest(wlo, whi, wcnt, two_word=k > 32)


# ------------------------------------------------------------------ CLI

def _cli():
    from .conftest import ROOT
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "cfrk_amd", "cfrk")


def _read_glb1(raw):
    assert raw[:8] == b"CFRKGLB1"
    k, flags = np.frombuffer(raw, "<u4", 2, 8)
    n, total = np.frombuffer(raw, "<u8", 2, 16)
    two = bool(flags & 2)
    dt = np.dtype([("hi", "<u8"), ("lo", "<u8"), ("c", "<u4")] if two else [("lo", "<u8"), ("c", "<u4")])
    assert len(raw) == 32 + int(n) * dt.itemsize
    rec = np.frombuffer(raw, dt, int(n), 32)
    assert int(rec["c"].astype(np.uint64).sum()) == int(total)
    return rec


def _parse_text(raw):
    """sparse text -> (list of key tuples, counts)"""
    keys, cnts = [], []
    for line in raw.decode().splitlines():
        f = line.split(":")
        keys.append(tuple(int(x) for x in f[:-1]))
        cnts.append(int(f[-1]))
    return keys, np.array(cnts, np.uint64)


def _spectrum_text(cnts):
    if len(cnts) == 0:
        return b""
    c, n = np.unique(np.asarray(cnts, np.uint64), return_counts=True)
    return b"".join(b"%d\t%d\n" % (int(a), int(b)) for a, b in zip(c, n))


@pytest.mark.parametrize("k", [5, 15, 31, 63])
def test_cli_histo_and_count_range(tmp_path, k):
    cli = _cli()
    rng = np.random.default_rng(600 + k)
    genome = rng.integers(0, 4, 8000)
    seqs = []
    for _ in range(2000):
        L = int(rng.integers(20, 220))
        a = int(rng.integers(0, len(genome) - L))
        seqs.append("".join("ACGT"[c] for c in genome[a:a + L]))
    seqs.append("A" * 20000)                                # one key counted > 16384 times: the host tail path
    fa = tmp_path / "g.fasta"
    fa.write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(seqs)))
    base = [cli, str(fa)]

    def run(out, *extra):
        subprocess.run(base + [str(out), str(k), "--global", "--canonical"] + list(extra), check=True, timeout=300)

    run(tmp_path / "full.txt", "--histo", str(tmp_path / "h1.txt"))
    keys, cnts = _parse_text((tmp_path / "full.txt").read_bytes())
    assert int(cnts.max()) > 16384
    spectrum = _spectrum_text(cnts)
    assert (tmp_path / "h1.txt").read_bytes() == spectrum
    m = (cnts >= 2) & (cnts <= 9)
    assert not m.all() and (m.any() or k == 5)              # (k = 5: every one of the 512 keys is common)
    lines = (tmp_path / "full.txt").read_bytes().splitlines(keepends=True)
    want_txt = b"".join(l for l, keep in zip(lines, m) if keep)
    run(tmp_path / "f.txt", "--min-count", "2", "--max-count", "9")
    assert (tmp_path / "f.txt").read_bytes() == want_txt
    run(tmp_path / "f.bin", "--min-count", "2", "--max-count", "9", "--binary")
    rec = _read_glb1((tmp_path / "f.bin").read_bytes())
    assert len(rec) == int(m.sum()) and (rec["c"].astype(np.uint64) == cnts[m]).all()
    kk = [keys[i] for i in np.nonzero(m)[0]]
    if k <= 32:
        assert [(int(x),) for x in rec["lo"]] == kk
    else:
        assert [(int(h), int(l)) for h, l in zip(rec["hi"], rec["lo"])] == kk
    # two owners on one device: the same bytes
    run(tmp_path / "g2.txt", "--gpus", "2", "--same-device", "--histo", str(tmp_path / "h2.txt"),
        "--min-count", "2", "--max-count", "9")
    assert (tmp_path / "h2.txt").read_bytes() == spectrum
    assert (tmp_path / "g2.txt").read_bytes() == want_txt
    run(tmp_path / "g2.bin", "--gpus", "2", "--same-device", "--min-count", "2", "--max-count", "9", "--binary")
    assert (tmp_path / "g2.bin").read_bytes() == (tmp_path / "f.bin").read_bytes()
    # spectrum only: the output path is not created
    for extra in ([], ["--gpus", "2", "--same-device"]):
        (tmp_path / "h3.txt").unlink(missing_ok=True)
        run(tmp_path / "none.txt", "--histo", str(tmp_path / "h3.txt"), "--histo-only", *extra)
        assert (tmp_path / "h3.txt").read_bytes() == spectrum
        assert not (tmp_path / "none.txt").exists()
