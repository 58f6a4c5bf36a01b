"""GPU: digital normalisation (cfrk_global_normalize / _device, GlobalCounter.normalize, the CLI's --normalize-out) held
to the plain-Python rule of tests/normalize_ref.py: keep bytes, n_kept and the job's full export and digest are EQUAL,
never close.  The reads come from both strands of two small genomes at lengths on every size-class boundary of the
kernels (0, 1, 256 / 257 and 2048 / 2049 windows), with a few invalid codes, in a fixed shuffled order; most of the short
reads are dropped at cutoff 3.  The key lists of a read set are computed once per (k, strand rule) and shared."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from . import hash_craft as hc
from . import normalize_ref as nr
from .test_gpu_hash_edges import HINT, LG, _assert_construction, _assert_hash, _keys

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [4, 12, 13, 21, 31, 32, 33, 47, 64]


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ inputs (built once, shared, never changed)

def _revcomp(a):
    return (3 - a[::-1]).astype(np.int8)


@functools.lru_cache(maxsize=None)
def _genomes():
    rng = np.random.default_rng(2024)
    return rng.integers(0, 4, 400).astype(np.int8), rng.integers(0, 4, 6000).astype(np.int8)


@functools.lru_cache(maxsize=None)
def _read_set(k):
    """about 300 reads -> (data, start, length, from_small): lengths on the class boundaries, both strands, a few invalid
    codes, shuffled"""
    small, large = _genomes()
    rng = np.random.default_rng([k, 7])
    lens = [k - 1, k, k + 1] * 4 + [50] * 90 + [150] * 160 + [k + 254, k + 255, k + 256] * 6 + \
           [k + 2046, k + 2047, k + 2048, 3000] * 3
    lens = [lens[i] for i in rng.permutation(len(lens))]
    rows, from_small = [], []
    for j, L in enumerate(lens):
        g = small if L <= len(small) else large
        p = int(rng.integers(0, len(g) - L + 1))
        r = g[p:p + L].copy()
        if rng.integers(0, 2):
            r = _revcomp(r)
        if j % 23 == 5 and L > 0:
            r[int(rng.integers(0, L))] = -1 if j % 2 else 4
        rows.append(r)
        from_small.append(g is small)
    length = np.array([len(r) for r in rows], np.int32)
    start = np.concatenate([[0], np.cumsum(length[:-1].astype(np.int64) + 1)]).astype(np.int64)
    data = np.full(int(length.sum()) + len(rows), -1, np.int8)
    for s, r in zip(start, rows):
        data[s:s + len(r)] = r
    for a in (data, start, length):
        a.setflags(write=False)
    return data, start, length, np.array(from_small)


@functools.lru_cache(maxsize=None)
def _set_keys(k, canonical):
    data, start, length, _ = _read_set(k)
    return tuple(tuple(x) for x in nr.all_read_keys(data, start, length, k, canonical))


def _flags(canonical, extra=0):
    import cfrk_amd
    return (cfrk_amd.CFRK_CANONICAL if canonical else 0) | extra


def _assert_job(g, counts, two, what):
    wlo, whi, wcnt = nr.export_arrays(counts)
    lo, hi, cnt = g.export()
    assert len(lo) == len(wlo), (what, "distinct", len(lo), len(wlo))
    assert (lo == wlo).all() and (cnt == wcnt).all() and (not two or (hi == whi).all()), what
    assert g.digest() == nr.digest(counts, two), what


def _assert_call(got, want, what):
    keep, n = got
    wkeep, wn, _ = want
    bad = np.nonzero(keep != wkeep)[0]
    assert len(bad) == 0, (what, "keep differs at reads", bad[:10], keep[bad[:10]], wkeep[bad[:10]])
    assert n == wn, (what, n, wn)


# ------------------------------------------------------------------ the rule, every k and class boundary

def _matrix():
    nS = len(_read_set(31)[2])
    cases = []
    for k in KS:
        for canonical in (False, True):
            cases += [(k, canonical, 3, 5), (k, canonical, 1, 64), (k, canonical, 20, nS)]
    cases += [(13, True, 3, nS + 1), (32, False, 3, nS + 1), (64, True, 1, nS + 1), (31, True, 3, 1), (47, False, 3, 1),
              (31, False, 20, 5), (47, True, 20, 64), (12, False, 3, nS)]
    return cases


@pytest.mark.parametrize("k,canonical,cutoff,batch", _matrix())
def test_matches_reference(ctx, k, canonical, cutoff, batch):
    import cfrk_amd
    data, start, length, from_small = _read_set(k)
    g = cfrk_amd.GlobalCounter(ctx, k, _flags(canonical), 1 << 15)
    got = g.normalize(data, start, length, cutoff, batch)
    want = nr.normalize_keys(_set_keys(k, canonical), cutoff, batch)
    _assert_call(got, want, (k, canonical, cutoff, batch))
    _assert_job(g, want[2], k > 32, (k, canonical, cutoff, batch))
    if cutoff == 3 and batch <= 5:
        short = from_small & (length >= k)
        assert got[0][short].mean() < 0.5, "the input does not exercise the drop"
    # read statistics of the normalised job: its median of a kept-or-not read is what a further call would judge by
    st = g.read_stats(data, start, length, cutoff)
    keys = _set_keys(k, canonical)
    for i in (0, len(keys) // 2, len(keys) - 1):
        if keys[i]:
            assert st["median"][i] == nr.lower_median([want[2].get(x, 0) for x in keys[i]])


def test_all_t_side_word(ctx):
    """k = 32, non-canonical: the all-T key lives in the side word, which the judge reads and the insert writes"""
    import cfrk_amd
    rng = np.random.default_rng(3)
    rows = [np.full(L, 3, np.int8) for L in (32, 33, 40, 32, 290, 32, 40, 2100, 33, 32)] + \
           [rng.integers(0, 4, 60).astype(np.int8) for _ in range(4)]
    rows = [rows[i] for i in rng.permutation(len(rows))]
    length = np.array([len(r) for r in rows], np.int32)
    start = np.concatenate([[0], np.cumsum(length[:-1].astype(np.int64) + 1)]).astype(np.int64)
    data = np.full(int(length.sum()) + len(rows), -1, np.int8)
    for s, r in zip(start, rows):
        data[s:s + len(r)] = r
    for cutoff, batch in ((3, 1), (3, 2), (12, 3), (0xFFFFFFFF, 4)):
        g = cfrk_amd.GlobalCounter(ctx, 32, cfrk_amd.CFRK_FORCE_HASH, 1 << 12)
        want = nr.normalize(data, start, length, 32, False, cutoff, batch)
        _assert_call(g.normalize(data, start, length, cutoff, batch), want, ("all-T", cutoff, batch))
        assert want[2].get(hc.ALL_ONES, 0) > 0
        _assert_job(g, want[2], False, ("all-T", cutoff, batch))


@pytest.mark.parametrize("partitioned", [False, True])
def test_job_that_holds_counts(ctx, partitioned):
    """the small genome pre-counted four times (through the HBM table, or by a partitioned path whose result the call
    must fold into the table first): its reads are dropped from the first round on"""
    import cfrk_amd
    k, canonical, cutoff, batch = 31, True, 3, 16
    small, _ = _genomes()
    pre = np.concatenate([np.append(small, np.int8(-1))] * 4)
    pre_start = np.arange(4, dtype=np.int64) * (len(small) + 1)
    pre_len = np.full(4, len(small), np.int32)
    data, start, length, from_small = _read_set(k)
    g = cfrk_amd.GlobalCounter(ctx, k, _flags(canonical, 0 if partitioned else cfrk_amd.CFRK_FORCE_HASH), 1 << 15)
    g.add(pre, pre_start, pre_len)
    counts = nr.add_keys(nr.all_read_keys(pre, pre_start, pre_len, k, canonical))
    clean = np.array([len(x) > 0 and all(counts.get(y, 0) >= 4 for y in x) for x in _set_keys(k, canonical)])
    want = nr.normalize_keys(_set_keys(k, canonical), cutoff, batch, counts)
    got = g.normalize(data, start, length, cutoff, batch)
    _assert_call(got, want, ("pre-counted", partitioned))
    assert clean[from_small].sum() > 100 and not got[0][clean & from_small].any()
    _assert_job(g, want[2], False, ("pre-counted", partitioned))
    # ... and the job goes on: another add, another normalise call
    g.add(pre, pre_start, pre_len)
    nr.add_keys(nr.all_read_keys(pre, pre_start, pre_len, k, canonical), counts)
    want = nr.normalize_keys(_set_keys(k, canonical), 9, 64, counts)
    _assert_call(g.normalize(data, start, length, 9, 64), want, ("pre-counted, second call", partitioned))
    _assert_job(g, want[2], False, ("pre-counted, second call", partitioned))


# ------------------------------------------------------------------ crafted collisions: long probes in table_find*

def _key_reads(lo, hi, reps, k, rng):
    """key i as a read of exactly k bases, reps[i] times, shuffled"""
    rows = np.full((len(lo), k + 1), -1, np.int8)
    for i, (l, h) in enumerate(zip(lo, hi)):
        rows[i, :k] = hc.key_to_read(l, h, k)
    rows = rows[rng.permutation(np.repeat(np.arange(len(lo)), reps))]
    n = len(rows)
    return np.ascontiguousarray(rows.reshape(-1)), np.arange(n, dtype=np.int64) * (k + 1), np.full(n, k, np.int32)


@pytest.mark.parametrize("k,kind", [(31, "wrap"), (31, "cluster"), (32, "wrap"), (32, "cluster"), (47, "wrap"),
                                    (47, "cluster"), (47, "words")])
def test_crafted_collisions(ctx, k, kind):
    """keys that home on the table's last slots (chains through the wrap, clusters of hundreds, two-word keys that differ
    in one word only) as one-window reads: every judge walks the chain of its key, absent keys to the chain's end"""
    import cfrk_amd
    two = k > 32
    lo, hi = _keys(kind, k)
    _assert_hash(lo[:8], hi[:8], two)
    _assert_construction(kind, lo, hi, two)
    rng = np.random.default_rng([k, ["wrap", "cluster", "words"].index(kind)])
    reps = rng.integers(1, 7, len(lo))
    data, start, length = _key_reads(lo, hi, reps, k, rng)
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_FORCE_HASH, HINT)
    assert g.hash_geometry() == (LG, 0), "table sizing rule changed"
    counts = {}
    for cutoff, batch in ((3, 64), (5, 7)):
        want = nr.normalize(data, start, length, k, False, cutoff, batch, counts)
        _assert_call(g.normalize(data, start, length, cutoff, batch), want, (k, kind, cutoff, batch))
        _assert_job(g, counts, two, (k, kind, cutoff, batch))
    assert max(counts.values()) >= 5 and len(counts) == len(lo)


# ------------------------------------------------------------------ properties, product against product

@pytest.mark.parametrize("k,canonical", [(21, True), (32, False), (47, True)])
def test_scheduling_free_properties(ctx, k, canonical):
    import cfrk_amd
    data, start, length, _ = _read_set(k)
    has_window = np.array([len(x) > 0 for x in _set_keys(k, canonical)])
    # cutoff 2^32 - 1 keeps every read with a valid window: a plain add of the same reads
    g = cfrk_amd.GlobalCounter(ctx, k, _flags(canonical), 1 << 15)
    keep, n = g.normalize(data, start, length, 0xFFFFFFFF, 50)
    assert (keep.astype(bool) == has_window).all() and n == has_window.sum()
    all_lo, all_hi, all_cnt = g.export()
    all_digest = g.digest()
    ctx2 = cfrk_amd.Context(0)
    try:
        g2 = cfrk_amd.GlobalCounter(ctx2, k, _flags(canonical), 1 << 15)
        g2.add(data, start, length)
        lo, hi, cnt = g2.export()
        assert (lo == all_lo).all() and (hi == all_hi).all() and (cnt == all_cnt).all() and g2.digest() == all_digest
    finally:
        ctx2.close()
    # cutoff 0 keeps nothing and leaves the job as it was
    keep, n = g.normalize(data, start, length, 0, 50)
    assert n == 0 and not keep.any() and g.digest() == all_digest
    # one call over 2 m B reads = two calls over its halves
    B, m = 16, 4
    h = m * B
    end = int(start[2 * h])
    ga = cfrk_amd.GlobalCounter(ctx, k, _flags(canonical), 1 << 15)
    keep_a, n_a = ga.normalize(data[:end], start[:2 * h], length[:2 * h], 3, B)
    exp_a, dig_a = ga.export(), ga.digest()
    gb = cfrk_amd.GlobalCounter(ctx, k, _flags(canonical), 1 << 15)
    mid = int(start[h])
    k1, n1 = gb.normalize(data[:mid], start[:h], length[:h], 3, B)
    k2, n2 = gb.normalize(data[mid:end], start[h:2 * h] - mid, length[h:2 * h], 3, B)
    assert (np.concatenate([k1, k2]) == keep_a).all() and n1 + n2 == n_a and 0 < n_a < 2 * h
    assert all((x == y).all() for x, y in zip(gb.export(), exp_a)) and gb.digest() == dig_a


# ------------------------------------------------------------------ device form, errors

class _Dev:
    """the reads on the device (the data one byte off any alignment), room for the keep bytes"""

    def __init__(self, ctx, data, start, length):
        self.ctx, self.nN, self.nS = ctx, len(data), len(length)
        self.bufs = [ctx.alloc(len(data) + 16), ctx.alloc(max(8, start.nbytes)), ctx.alloc(max(4, length.nbytes)),
                     ctx.alloc(self.nS + 2)]
        self.data, self.start, self.length, self.keep = self.bufs[0] + 1, self.bufs[1], self.bufs[2], self.bufs[3] + 1
        guard = np.full(self.nS + 2, 0xAB, np.uint8)
        ctx.h2d(self.bufs[3], guard)
        padded = np.full(len(data) + 16, -1, np.int8)
        padded[1:1 + len(data)] = data
        ctx.h2d(self.bufs[0], padded)
        if self.nS:
            ctx.h2d(self.start, np.ascontiguousarray(start, np.int64))
            ctx.h2d(self.length, np.ascontiguousarray(length, np.int32))

    def keep_bytes(self):
        out = np.zeros(self.nS + 2, np.uint8)
        self.ctx.d2h(out, self.bufs[3])
        assert out[0] == 0xAB and out[-1] == 0xAB, "a byte beside the keep array was written"
        return out[1:-1]

    def free(self):
        for p in self.bufs:
            self.ctx.free(p)


def test_device_form_ranges_and_host_form(ctx):
    import cfrk_amd
    k, canonical, cutoff, batch = 21, True, 3, 5
    data, start, length, _ = _read_set(k)
    start, length = start.copy(), length.copy()
    nN = len(data)
    start[3], start[40], start[77] = -5, nN - 10, -(1 << 40)          # before the buffer, runs past its end, far away
    start[120], length[150], start[200] = nN + 100, -3, 1 << 60
    length[10] = 0x7FFFFFFF
    keys = nr.all_read_keys(data, start, length, k, canonical)
    assert sum(len(x) == 0 for x in keys) >= 7
    want = nr.normalize_keys(keys, cutoff, batch)
    d = _Dev(ctx, data, start, length)
    try:
        g = cfrk_amd.GlobalCounter(ctx, k, _flags(canonical), 1 << 15)
        n = g.normalize_device(d.data, d.start, d.length, nN, d.nS, cutoff, d.keep, batch)
        keep = d.keep_bytes()
        _assert_call((keep, n), want, "device form")
        assert not keep[[3, 40, 77, 120, 150, 200, 10]].any()
        _assert_job(g, want[2], False, "device form")
        before = g.digest()
        assert g.normalize_device(0, 0, 0, nN, 0, cutoff, 0, batch) == 0          # nS = 0: fine, nothing changes
        assert g.normalize_device(d.data, d.start, d.length, 0, 0, cutoff, d.keep, 1) == 0
        assert g.digest() == before and (d.keep_bytes() == keep).all()
    finally:
        d.free()
    # the host form on the untouched table gives what the device form gives on it
    data, start, length, _ = _read_set(k)
    d = _Dev(ctx, data, start, length)
    try:
        g = cfrk_amd.GlobalCounter(ctx, k, _flags(canonical), 1 << 15)
        n = g.normalize_device(d.data, d.start, d.length, nN, d.nS, cutoff, d.keep, batch)
        keep, dev_export, dev_digest = d.keep_bytes().copy(), g.export(), g.digest()
    finally:
        d.free()
    g = cfrk_amd.GlobalCounter(ctx, k, _flags(canonical), 1 << 15)
    hkeep, hn = g.normalize(data, start, length, cutoff, batch)
    assert (hkeep == keep).all() and hn == n and g.digest() == dev_digest
    assert all((x == y).all() for x, y in zip(g.export(), dev_export))
    # ... and refuses a table that contradicts the terminators, counting nothing
    bad = length.copy()
    bad[17] += 1
    with pytest.raises(cfrk_amd.CfrkError) as e:
        g.normalize(data, start, bad, cutoff, batch)
    assert e.value.code == -5 and g.digest() == dev_digest


def test_error_codes(ctx):
    import cfrk_amd
    L = cfrk_amd.load_library()
    data, start, length, _ = _read_set(31)
    d = _Dev(ctx, data, start, length)
    n = C.c_int64(-1)
    vp = C.c_void_p
    call = lambda h, nN, nS, batch, dat=d.data, st=d.start, ln=d.length, kp=d.keep, out=C.byref(n): \
        L.cfrk_global_normalize_device(h, vp(dat), vp(st), vp(ln), nN, nS, 3, batch, vp(kp), out)
    try:
        fresh = cfrk_amd.Context(0)
        try:
            assert call(fresh._h, d.nN, d.nS, 8) == -4                                   # before begin
        finally:
            fresh.close()
        g = cfrk_amd.GlobalCounter(ctx, 31, cfrk_amd.CFRK_RUNS_ONLY, 1 << 15)
        assert call(ctx._h, d.nN, d.nS, 8) == -4                                        # a job of runs
        with pytest.raises(cfrk_amd.CfrkError) as e:
            g.normalize(data, start, length, 3)
        assert e.value.code == -4
        g = cfrk_amd.GlobalCounter(ctx, 31, 0, 1 << 15)
        assert call(ctx._h, -1, d.nS, 8) == -1 and call(ctx._h, d.nN, -1, 8) == -1      # negative sizes
        assert call(ctx._h, d.nN, d.nS, 0) == -1 and call(ctx._h, d.nN, d.nS, -4) == -1  # batch_reads < 1
        assert call(ctx._h, d.nN, d.nS, 8, out=None) == -1                              # NULL n_kept
        for null in ("dat", "st", "ln", "kp"):
            assert call(ctx._h, d.nN, d.nS, 8, **{null: None}) == -1
        assert L.cfrk_global_normalize(ctx._h, None, None, None, 0, 0, 3, 8, None, C.byref(n)) == 0 and n.value == 0
        assert g.finish() == 0, "a refused call counted something"
        assert call(ctx._h, d.nN, d.nS, 8) == 0 and n.value > 0
    finally:
        d.free()


def test_table_full(ctx):
    """1024 slots, about 1500 distinct keys: the call ends on the bounded probe loops with the error code, and finish
    says the same"""
    import cfrk_amd
    rng = np.random.default_rng(9)
    rows = np.full((10, 182), -1, np.int8)
    rows[:, :181] = rng.integers(0, 4, (10, 181))
    data = rows.reshape(-1)
    start, length = np.arange(10, dtype=np.int64) * 182, np.full(10, 181, np.int32)
    assert len(nr.add_keys(nr.all_read_keys(data, start, length, 31, False))) == 1510
    g = cfrk_amd.GlobalCounter(ctx, 31, cfrk_amd.CFRK_FORCE_HASH, 64)
    assert g.hash_geometry()[0] == 10
    with pytest.raises(cfrk_amd.CfrkError) as e:
        g.normalize(data, start, length, 5, 4)
    assert e.value.code == -6
    with pytest.raises(cfrk_amd.CfrkError) as e:
        g.finish()
    assert e.value.code == -6


# ------------------------------------------------------------------ CLI

def _cli():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cfrk_amd", "host")], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "cfrk_amd", "cfrk")


def test_cli_normalize_out(ctx, tmp_path):
    """a FASTQ file through --normalize-out: NFILE is the kept records cut from the input text, out.cfrk and --histo
    describe the kept reads; the default writer names the kept reads by record number; without the new options the
    count output is that of a plain add"""
    import cfrk_amd
    from .test_gpu_spectrum import _read_glb1, _spectrum_text
    cli = _cli()
    k, cutoff, batch = 21, 3, 16
    data, start, length, _ = _read_set(k)
    rng = np.random.default_rng(77)
    letters = np.frombuffer(b"ACGTN", np.uint8)
    records, seqs = [], []
    for i, (s, L) in enumerate(zip(start, length)):
        codes = data[s:s + L]
        seq = letters[np.where((codes < 0) | (codes > 3), 4, codes)].tobytes()
        qual = (rng.integers(2, 41, L) + 33).astype(np.uint8).tobytes()
        records.append(b"@read%d len=%d\n%s\n+\n%s\n" % (i, L, seq, qual))
        seqs.append(seq)
    fq = tmp_path / "in.fastq"
    fq.write_bytes(b"".join(records))
    want = nr.normalize_keys(_set_keys(k, True), cutoff, batch)
    assert 0 < want[1] < len(records)
    base = [cli, str(fq)]
    glob = [str(k), "--global", "--canonical"]
    norm = ["--normalize-cutoff", str(cutoff), "--normalize-batch", str(batch)]
    nf, out, histo = tmp_path / "kept.fastq", tmp_path / "out.bin", tmp_path / "h.txt"
    subprocess.run(base + [str(out)] + glob + norm + ["--normalize-out", str(nf), "--normalize-names", "--normalize-format", "fastq",
                                                      "--histo", str(histo), "--binary"], check=True, timeout=300)
    assert nf.read_bytes() == b"".join(r for r, kp in zip(records, want[0]) if kp)
    wlo, _, wcnt = nr.export_arrays(want[2])
    rec = _read_glb1(out.read_bytes())
    assert (rec["lo"] == wlo).all() and (rec["c"] == wcnt).all()
    assert histo.read_bytes() == _spectrum_text(wcnt)
    # the default writer: FASTA, named by record number
    nf2, out2 = tmp_path / "kept.fa", tmp_path / "out2.bin"
    subprocess.run(base + [str(out2)] + glob + norm + ["--normalize-out", str(nf2), "--binary"], check=True, timeout=300)
    assert nf2.read_bytes() == b"".join(b">%d\n%s\n" % (i, s) for i, (s, kp) in enumerate(zip(seqs, want[0])) if kp)
    assert out2.read_bytes() == out.read_bytes()
    # names as FASTA
    nf3 = tmp_path / "kept_named.fa"
    subprocess.run(base + [str(tmp_path / "out3.bin")] + glob + norm + ["--normalize-out", str(nf3), "--normalize-names", "--binary"],
                   check=True, timeout=300)
    assert nf3.read_bytes() == b"".join(b">read%d len=%d\n%s\n" % (i, len(s), s) for i, (s, kp) in enumerate(zip(seqs, want[0])) if kp)
    # without the new options: the counts of a plain add of the same reads
    plain = tmp_path / "plain.bin"
    subprocess.run(base + [str(plain)] + glob + ["--binary"], check=True, timeout=300)
    g = cfrk_amd.GlobalCounter(ctx, k, cfrk_amd.CFRK_CANONICAL, 1 << 15)
    g.add(data, start, length)
    lo, _, cnt = g.export()
    rec = _read_glb1(plain.read_bytes())
    assert (rec["lo"] == lo).all() and (rec["c"] == cnt).all()
    # refusals
    for extra in (["--gpus", "2", "--same-device"], ["--device-parse"]):
        r = subprocess.run(base + [str(tmp_path / "x.bin")] + glob + norm + ["--normalize-out", str(tmp_path / "x.fa")] + extra,
                           stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 1 and b"--normalize-out" in r.stderr
    r = subprocess.run(base + [str(tmp_path / "x.bin"), str(k)] + norm + ["--normalize-out", str(tmp_path / "x.fa")],
                       stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 1 and b"need --global" in r.stderr
    r = subprocess.run([cli, "--query-db", str(plain), "--query", str(fq), "--query-out", str(tmp_path / "q.txt")] + norm +
                       ["--normalize-out", str(tmp_path / "x.fa")], stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 1 and b"--normalize" in r.stderr
    assert not (tmp_path / "x.fa").exists()
