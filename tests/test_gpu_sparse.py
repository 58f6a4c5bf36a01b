"""GPU: per-read sparse k-mer counts (cfrk_per_read_sparse / _device) through the Python mirror, host and device forms,
against the oracle: the non-zero bins of the native dense rows for small k, tests.oracle_lib.global_count of every read
alone for large k, long reads on the slow path, consistency with global mode, the call contract, and `cfrk --sparse`."""
import os
import subprocess

import numpy as np
import pytest

from . import oracle_lib as orc
from . import refsem
from .test_sparse_cpu import py_format_rows

pytestmark = pytest.mark.gpu

CFRK_ERR_ARG, CFRK_ERR_LAYOUT, CFRK_ERR_SMALL_BUF = -1, -5, -9


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


def _device_form(ctx, data, start, length, k, flags):
    """the device form on copies of the host arrays (d_data deliberately at an odd address): sizes-only call, then the
    exact-size call -> (row_ptr, keys, counts)"""
    import cfrk_amd
    nN, nS = len(data), len(length)
    bufs = [ctx.alloc(nN + 65), ctx.alloc(nS * 8 + 8), ctx.alloc(nS * 4 + 8), ctx.alloc((nS + 1) * 8)]
    d_data, d_start, d_length, d_row = bufs[0] + 1, bufs[1], bufs[2], bufs[3]
    try:
        if nN:
            ctx.h2d(d_data, data)
        if nS:
            ctx.h2d(d_start, start)
            ctx.h2d(d_length, length)
        row_ptr = np.full(nS + 1, -7, np.int64)
        try:
            nnz = ctx.per_read_sparse_device(d_data, d_start, d_length, nN, nS, k, flags, d_row, 0, 0, 0)
            assert nnz == 0
        except cfrk_amd.CfrkError as e:
            assert e.code == CFRK_ERR_SMALL_BUF
            nnz = e.nnz
            assert nnz > 0
        ctx.sync()
        ctx.d2h(row_ptr, d_row)
        assert row_ptr[nS] == nnz
        sized = row_ptr.copy()
        keys = np.empty(nnz, np.uint64)
        counts = np.empty(nnz, np.uint32)
        bufs += [ctx.alloc(nnz * 8 + 8), ctx.alloc(nnz * 4 + 8)]
        assert ctx.per_read_sparse_device(d_data, d_start, d_length, nN, nS, k, flags, d_row, bufs[4], bufs[5], nnz) == nnz
        ctx.sync()
        ctx.d2h(row_ptr, d_row)
        assert (row_ptr == sized).all()
        if nnz:
            ctx.d2h(keys, bufs[4])
            ctx.d2h(counts, bufs[5])
        return row_ptr, keys, counts
    finally:
        ctx.sync()
        for b in bufs:
            ctx.free(b)


def _flags(canonical):
    import cfrk_amd
    return cfrk_amd.CFRK_CANONICAL if canonical else 0


def _oracle_rows(reads, k, canonical):
    """CSR of tests.oracle_lib.global_count of every read alone"""
    sizes, keys, counts = [], [], []
    for r in reads:
        lo, _, cnt = orc.global_count(np.concatenate([r, [-1]]).astype(np.int8), k, orc.ORC_CANONICAL if canonical else 0)
        sizes.append(len(lo))
        keys.append(lo.astype(np.uint64))
        counts.append(cnt.astype(np.uint32))
    row_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return row_ptr, np.concatenate(keys + [np.zeros(0, np.uint64)]), np.concatenate(counts + [np.zeros(0, np.uint32)])


def _check_contract(row_ptr, keys, counts, nS):
    assert len(row_ptr) == nS + 1 and row_ptr[0] == 0
    assert (np.diff(row_ptr) >= 0).all()
    assert row_ptr[nS] == len(keys) == len(counts)
    if len(keys) > 1:
        inner = np.ones(len(keys) - 1, bool)
        ends = row_ptr[1:-1]
        ends = ends[(ends > 0) & (ends < len(keys))]
        inner[ends - 1] = False                                  # pairs that straddle two rows
        assert (keys[1:][inner] > keys[:-1][inner]).all()
    assert (counts > 0).all()


def _same(got, want):
    for g, w in zip(got, want):
        assert len(g) == len(w) and (np.asarray(g) == np.asarray(w)).all()


def _both_forms(ctx, reads, k, canonical, want):
    data, start, length = refsem.flatten(reads)
    got = ctx.per_read_sparse(data, start, length, k, _flags(canonical))
    _check_contract(*got, len(reads))
    _same(got, want)
    got = _device_form(ctx, data, start, length, k, _flags(canonical))
    _check_contract(*got, len(reads))
    _same(got, want)


# ------------------------------------------------------------------ 1: small k, against the native dense rows

def _small_k_reads(k):
    rng = np.random.default_rng(100 + k)
    rnd = lambda L: rng.integers(0, 4, L).astype(np.int8)
    mid = rnd(120)
    mid[[0, 1, 50, 51, 52, 90, 118, 119]] = -1                  # invalid bases in the middle and at both ends
    reads = [np.zeros(0, np.int8), rnd(1), rnd(k - 1), rnd(k), rnd(k), np.full(40, -1, np.int8), mid,
             np.full(77, 2, np.int8), rnd(3000), np.full(k, 3, np.int8)]
    for L in rng.integers(1, 400, 14):
        r = rnd(int(L))
        r[rng.random(int(L)) < 0.03] = -1
        reads.append(r)
    return reads


@pytest.mark.parametrize("k", range(1, 11))
def test_rows_equal_nonzeros_of_native_dense(ctx, k):
    reads = _small_k_reads(k)
    data, start, length = refsem.flatten(reads)
    dense = orc.per_read_dense(data, start, length, k, 0)
    sizes = (dense != 0).sum(axis=1)
    r, c = np.nonzero(dense)
    want = (np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), c.astype(np.uint64), dense[r, c].astype(np.uint32))
    homopolymer = 7
    assert sizes[homopolymer] == 1 and dense[homopolymer].max() == 77 - k + 1
    _both_forms(ctx, reads, k, False, want)


# ------------------------------------------------------------------ 2: large k, against the oracle per read

def _genome_reads(k):
    rng = np.random.default_rng(200 + k)
    genome = rng.integers(0, 4, 20000).astype(np.int8)
    reads = []
    for L in rng.integers(30, 301, 2000):
        a = int(rng.integers(0, len(genome) - int(L)))
        r = genome[a:a + int(L)].copy()
        if rng.random() < 0.1:
            r[int(rng.integers(0, int(L)))] = -1
        reads.append(r)
    reads.append(np.tile(np.array([0, 1], np.int8), 120))       # period 2
    reads.append(np.tile(np.array([2, 0, 3], np.int8), 90))     # period 3
    reads.append(np.full(32 + 40, 3, np.int8))                  # all T: the all-ones key at k = 32
    half = rng.integers(0, 4, 60).astype(np.int8)
    reads.append(np.concatenate([half, (3 - half)[::-1]]))      # its own reverse complement
    reads.append(np.zeros(0, np.int8))
    return reads


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [11, 15, 16, 21, 31, 32])
def test_rows_equal_oracle_per_read(ctx, k, canonical):
    reads = _genome_reads(k)
    want = _oracle_rows(reads, k, canonical)
    if k == 32:
        allT = len(reads) - 3
        a = want[0][allT]
        assert want[1][a] == np.uint64(2 ** 64 - 1 if not canonical else 0) and want[2][a] == 41
    _both_forms(ctx, reads, k, canonical, want)


# ------------------------------------------------------------------ 3: long reads

@pytest.mark.parametrize("k, canonical", [(21, True), (31, False)])
def test_long_reads_next_to_short_ones(ctx, k, canonical):
    import cfrk_amd
    cap = cfrk_amd.CFRK_SPARSE_FAST_WINDOWS
    assert cap >= 1024
    rng = np.random.default_rng(300 + k)
    small = rng.integers(0, 4, 5000).astype(np.int8)
    genome = rng.integers(0, 4, 50000).astype(np.int8)
    cut = lambda g, L: np.resize(g[int(rng.integers(0, len(g))):], L).astype(np.int8)
    reads = []
    for w in (cap - 1, cap, cap + 1, 255, 256, 257):            # windows: the two LDS group sizes and their neighbours
        reads.append(cut(genome, w + k - 1))
        reads.append(cut(genome, 100))
    reads.append(cut(genome, 20000))
    reads.append(cut(genome, 150))
    big = cut(small, 200000)                                    # from a 5000-base genome: counts far above 1
    big[[7, 99999, 150000]] = -1
    reads.append(big)
    reads.append(np.full(3 * cap, 1, np.int8))                  # a long homopolymer: one key
    reads.append(cut(genome, 60))
    want = _oracle_rows(reads, k, canonical)
    assert want[2].max() > 30
    _both_forms(ctx, reads, k, canonical, want)


# ------------------------------------------------------------------ 4: consistency with global mode

def test_rows_sum_to_the_global_result(ctx):
    import cfrk_amd
    R, L, k = 100_000, 150, 31
    nN = R * (L + 1)
    bufs = [ctx.alloc(nN + 64), ctx.alloc(R * 8), ctx.alloc(R * 4), ctx.alloc((R + 1) * 8)]
    room = R * (L - k + 1)                                      # the window bound: always enough
    bufs += [ctx.alloc(room * 8), ctx.alloc(room * 4)]
    try:
        ctx.synth_reads_device(0, R, L, 200_000, bufs[0], bufs[1], bufs[2])
        nnz = ctx.per_read_sparse_device(bufs[0], bufs[1], bufs[2], nN, R, k, cfrk_amd.CFRK_CANONICAL, bufs[3], bufs[4],
                                         bufs[5], room)
        ctx.sync()
        row_ptr = np.empty(R + 1, np.int64)
        keys = np.empty(nnz, np.uint64)
        counts = np.empty(nnz, np.uint32)
        data = np.empty(nN, np.int8)
        ctx.d2h(row_ptr, bufs[3])
        ctx.d2h(keys, bufs[4])
        ctx.d2h(counts, bufs[5])
        ctx.d2h(data, bufs[0])
        g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, 400_000)
        g.add_device(bufs[0], nN)
        lo, _, cnt = g.export()
    finally:
        ctx.sync()
        for b in bufs:
            ctx.free(b)
    _check_contract(row_ptr, keys, counts, R)
    bad = np.concatenate([[0], np.cumsum((data < 0) | (data > 3))])
    valid_windows = int(((bad[k:] - bad[:-k]) == 0).sum())
    assert int(counts.sum(dtype=np.uint64)) == valid_windows
    u, inv = np.unique(keys, return_inverse=True)
    summed = np.bincount(inv, weights=counts.astype(np.float64), minlength=len(u)).astype(np.uint64)
    assert len(u) == len(lo) and (u == lo).all() and (summed == cnt.astype(np.uint64)).all()


# ------------------------------------------------------------------ 5: contract

def test_small_buffer_sizes_only_and_bad_arguments(ctx):
    import cfrk_amd
    import ctypes as C
    rng = np.random.default_rng(5)
    reads = [rng.integers(0, 4, int(L)).astype(np.int8) for L in rng.integers(0, 200, 50)]
    data, start, length = refsem.flatten(reads)
    k = 13
    want = _oracle_rows(reads, k, False)
    nnz_want = len(want[1])
    L_, h = ctx._L, ctx._h
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    nnz = C.c_uint64(123)
    row_ptr = np.full(len(reads) + 1, -1, np.int64)
    keys = np.full(nnz_want, 77, np.uint64)
    counts = np.full(nnz_want, 77, np.uint32)

    def call(k_=k, flags=0, row=row_ptr, cap=nnz_want, st=start, ln=length):
        return L_.cfrk_per_read_sparse(h, p(data), p(st), p(ln), len(data), len(reads), k_, flags,
                                       p(row) if row is not None else None, p(keys), p(counts), cap, C.byref(nnz))

    # one entry short: the sizes are complete, keys and counts untouched; the exact size then succeeds
    assert call(cap=nnz_want - 1) == CFRK_ERR_SMALL_BUF
    assert nnz.value == nnz_want and (row_ptr == want[0]).all()
    assert (keys == 77).all() and (counts == 77).all()
    assert call() == 0 and nnz.value == nnz_want
    _same((row_ptr, keys, counts), want)
    # sizes only: NULL keys / counts with cap 0
    row_ptr[:] = -1
    rc = L_.cfrk_per_read_sparse(h, p(data), p(start), p(length), len(data), len(reads), k, 0, p(row_ptr), None, None, 0,
                                 C.byref(nnz))
    assert rc == CFRK_ERR_SMALL_BUF and nnz.value == nnz_want and (row_ptr == want[0]).all()
    # nS = 0
    rp0 = np.full(1, -1, np.int64)
    assert L_.cfrk_per_read_sparse(h, None, None, None, 0, 0, k, 0, p(rp0), None, None, 0, C.byref(nnz)) == 0
    assert rp0[0] == 0 and nnz.value == 0
    r0 = ctx.per_read_sparse(np.zeros(0, np.int8), np.zeros(0, np.int64), np.zeros(0, np.int32), k)
    assert list(r0[0]) == [0] and len(r0[1]) == 0 and len(r0[2]) == 0
    # bad arguments
    assert call(k_=0) == CFRK_ERR_ARG and call(k_=33) == CFRK_ERR_ARG
    assert call(row=None) == CFRK_ERR_ARG
    assert call(flags=cfrk_amd.CFRK_COMPAT) == CFRK_ERR_ARG and call(flags=cfrk_amd.CFRK_FLOAT_INDEX) == CFRK_ERR_ARG
    assert call(flags=cfrk_amd.CFRK_CANONICAL | cfrk_amd.CFRK_COMPAT) == CFRK_ERR_ARG
    d_any = ctx.alloc(4096)
    try:
        for kk, fl, row in ((0, 0, d_any), (33, 0, d_any), (k, 0, 0), (k, cfrk_amd.CFRK_COMPAT, d_any),
                            (k, cfrk_amd.CFRK_FLOAT_INDEX, d_any)):
            with pytest.raises(cfrk_amd.CfrkError) as e:
                ctx.per_read_sparse_device(d_any, d_any, d_any, 16, 1, kk, fl, row, 0, 0, 0)
            assert e.value.code == CFRK_ERR_ARG
    finally:
        ctx.free(d_any)
    # broken layout: host form only
    bad_start = start.copy()
    bad_start[10] += 1
    assert call(st=bad_start) == CFRK_ERR_LAYOUT
    bad_len = length.copy()
    bad_len[20] += 1
    assert call(ln=bad_len) == CFRK_ERR_LAYOUT
    assert call() == 0
    _same((row_ptr, keys, counts), want)


def test_open_global_job_is_left_alone(ctx):
    import cfrk_amd
    data, start, length = orc.synth_reads(0, 3000, 150, 40000)
    for k, flags in ((31, cfrk_amd.CFRK_CANONICAL), (12, 0), (21, cfrk_amd.CFRK_FORCE_HASH)):
        g = cfrk_amd.GlobalCounter(ctx, k, flags, 200000)
        g.add(data, start, length)
        before = g.digest()
        rows = ctx.per_read_sparse(data, start, length, 21, cfrk_amd.CFRK_CANONICAL)
        assert rows[0][-1] > 0
        rows2 = _device_form(ctx, data, start, length, 9, 0)
        assert rows2[0][-1] > 0
        assert g.digest() == before
        g.add(data, start, length)
        wlo, whi, wcnt = orc.global_count(np.concatenate([data, data]), k, orc.ORC_CANONICAL if flags & cfrk_amd.CFRK_CANONICAL else 0)
        assert g.digest() == orc.digest(wlo, whi, wcnt)


# ------------------------------------------------------------------ 6: CLI

def _cli():
    from .conftest import ROOT
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "cfrk_amd", "cfrk")


@pytest.mark.parametrize("canonical", [False, True])
def test_cli_sparse_end_to_end(tmp_path, canonical):
    cli = _cli()
    k = 21
    rng = np.random.default_rng(600 + canonical)
    genome = rng.integers(0, 4, 30000).astype(np.int8)
    reads, text = [], []
    for i in range(3100):
        L = int(rng.integers(1, 400))
        a = int(rng.integers(0, len(genome) - L))
        r = genome[a:a + L].copy()
        if rng.random() < 0.2:                                   # a run of N
            b = int(rng.integers(0, L))
            r[b:b + int(rng.integers(1, 30))] = -1
        s = "".join("ACGTN"[c] for c in r)
        if rng.random() < 0.3:
            s = s.lower()
        width = int(rng.integers(20, 90))                        # multi-line records
        text.append(f">r{i} x\n" + "\n".join(s[j:j + width] for j in range(0, L, width)) + "\n")
        reads.append(r)
    fa = tmp_path / "in.fasta"
    fa.write_text("".join(text))
    want = py_format_rows(*_oracle_rows(reads, k, canonical))
    extra = ["--canonical"] if canonical else []
    out1, out2 = tmp_path / "a.cfrk", tmp_path / "b.cfrk"
    subprocess.run([cli, str(fa), str(out1), str(k), "4", "500", "--sparse"] + extra, check=True, timeout=300)
    subprocess.run([cli, str(fa), str(out2), str(k), "4", "500", "--sparse", "--gpus", "1"] + extra, check=True, timeout=300)
    got = out1.read_bytes()
    assert got.count(b"\n") == len(reads)
    assert got == want
    assert out2.read_bytes() == want
