"""tests/far_ref.py held equal to the plain references, without a GPU: the helpers are the oracle of
tests/test_gpu_far_offsets.py, where the texts are too large for anything but arithmetic.  Here the tiled texts are 40
to 60 copies of a block of about 3 KB of odd size, so that the block's records meet the 16 KiB tiles of the device
parsers in every phase, and small enough for the host parser, fastq_ref, text_out_ref and filter_ref to parse whole."""
import numpy as np
import pytest

from . import far_ref as far
from . import fastq_ref as fq
from . import filter_ref as fr
from . import ingest_cases as ic
from . import text_out_ref as tr

FASTQ_LENGTHS = (150, 1, 37, 150, 400, 2, 150, 211, 16, 150, 15, 17, 150, 93)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype}{got.shape} against {want.dtype}{want.shape}"
    assert np.array_equal(got, want), f"{what}: first difference at {int(np.flatnonzero(got != want)[0])}"


def _ranges(nN, rng):
    yield 0, nN
    yield 0, 0
    yield nN - 1, nN
    for _ in range(40):
        a = int(rng.integers(0, nN))
        yield a, int(rng.integers(a, nN + 1))


@pytest.mark.parametrize("reps", [40, 53, 60])
def test_tiled_fasta(reps):
    block = far.fasta_block(3, 14)
    assert 2500 < len(block) < 4000 and len(block) % 2 == 1
    rc, parse = ic.host_parse(block, ic.NATIVE)
    assert rc == 0
    text = far.tiled_text(block, reps)
    assert text.dtype == np.uint8 and text.tobytes() == block * reps
    rc, (data, start, length) = ic.host_parse(text.tobytes(), ic.NATIVE)
    assert rc == 0
    t_start, t_length, nN, nS, data_range = far.tiled_fasta_expect(block, parse, reps)
    assert (nN, nS) == (len(data), len(start))
    _same(t_start, start, "start")
    _same(t_length, length, "length")
    for a, b in _ranges(nN, np.random.default_rng(reps)):
        _same(data_range(a, b), data[a:b], f"data[{a}:{b}]")
    _same(far.tiled_index_expect(tr.index_ref(block, tr.TEXT_FASTA), len(block), reps), tr.index_ref(text.tobytes(), tr.TEXT_FASTA),
          "FASTA index rows")
    # the tiles of the device parser see a record start in many different phases
    assert len({int(o) % ic.T for o in tr.index_ref(text.tobytes(), tr.TEXT_FASTA)["head_off"]}) > 10 * reps


def test_tiled_fasta_compat_layout():
    """the reference's reader (newlines stay in the data as -1, the record's last byte is its terminator) keeps the
    arithmetic: a byte per base and line break, the reads one behind the other"""
    block, reps = far.fasta_block(3, 14), 41
    rc, parse = ic.host_parse(block, ic.COMPAT)
    assert rc == 0
    rc, (data, start, length) = ic.host_parse(block * reps, ic.COMPAT)
    assert rc == 0
    t_start, t_length, nN, nS, data_range = far.tiled_fasta_expect(block, parse, reps)
    assert (nN, nS) == (len(data), len(start))
    _same(t_start, start, "start")
    _same(t_length, length, "length")
    _same(data_range(0, nN), data, "data")


@pytest.mark.parametrize("reps", [40, 57])
@pytest.mark.parametrize("min_qual", [0, 20])
def test_tiled_fastq(reps, min_qual):
    block = far.fastq_block(5, FASTQ_LENGTHS)
    assert 2500 < len(block) < 4000 and len(block) % 2 == 1
    res = fq.parse(block, min_qual)
    assert res[0] == "ok"
    text = far.tiled_text(block, reps).tobytes()
    whole = fq.parse(text, min_qual)
    assert whole[0] == "ok"
    _, data, start, length = whole
    t_start, t_length, nN, nS, data_range = far.tiled_fastq_expect(block, res[1:], reps)
    assert (nN, nS) == (len(data), len(start))
    _same(t_start, start, "start")
    _same(t_length, length, "length")
    for a, b in _ranges(nN, np.random.default_rng(reps + min_qual)):
        _same(data_range(a, b), data[a:b], f"data[{a}:{b}]")
    if min_qual:
        assert (data == -1).sum() > nS, "min_qual masks bases of this block"
    _same(far.tiled_index_expect(tr.index_ref(block, tr.TEXT_FASTQ), len(block), reps), tr.index_ref(text, tr.TEXT_FASTQ),
          "FASTQ index rows")


def test_block_helpers_refuse_a_block_that_is_not_whole_records():
    block = far.fastq_block(5, FASTQ_LENGTHS)
    parse = fq.parse(block, 0)[1:]
    with pytest.raises(AssertionError):
        far.tiled_fastq_expect(block[:-1], parse, 3)
    with pytest.raises(AssertionError):
        far.tiled_fastq_expect(block[1:], parse, 3)
    fa = far.fasta_block(3, 14)
    with pytest.raises(AssertionError):
        far.tiled_fasta_expect(fa[:-1], ic.host_parse(fa, ic.NATIVE)[1], 3)


@pytest.mark.parametrize("seed", range(6))
def test_select_expect_equals_filter_ref(seed):
    rng = np.random.default_rng(seed)
    nS = int(rng.integers(1, 400))
    length = rng.integers(0, 60, nS).astype(np.int32)
    start = np.concatenate([[0], np.cumsum(length.astype(np.int64) + 1)[:-1]]).astype(np.int64)
    nN = int(length.astype(np.int64).sum()) + nS
    data = rng.integers(-1, 4, nN).astype(np.int8)
    spans = np.zeros(nS, fr.SPAN_DTYPE)
    spans["offset"] = rng.integers(-1, 30, nS)
    spans["length"] = rng.integers(-1, 40, nS)            # some spans do not lie inside their read: dropped
    whole = rng.random(nS) < 0.3
    spans["offset"][whole], spans["length"][whole] = 0, length[whole]
    keep = (rng.random(nS) < 0.8).astype(np.uint8)
    for use_span, use_keep, min_len in ((True, True, 0), (True, False, 7), (False, True, 0), (False, False, 25), (True, True, 12)):
        sp, kp = spans if use_span else None, keep if use_keep else None
        _, w_start, w_length, w_index = fr.ref_select(data, start, length, sp, kp, min_len)
        g_start, g_length, g_index, g_nN, g_nS = far.select_expect(start, length, kp, sp, min_len, nN)
        _same(g_start, w_start, "start_out")
        _same(g_length, w_length, "length_out")
        _same(g_index, w_index, "index_out")
        assert g_nS == len(w_index) and g_nN == int(w_length.astype(np.int64).sum()) + len(w_index)


def test_select_expect_drops_ranges_outside_the_buffer():
    start = np.array([0, -3, 90, 100, 40], np.int64)
    length = np.array([10, 5, 10, 1, 0], np.int32)
    s, l, i, nN, nS = far.select_expect(start, length, nN=100)
    assert i.tolist() == [0, 2, 4] and l.tolist() == [10, 10, 0] and s.tolist() == [0, 11, 22] and (nN, nS) == (23, 3)


def test_pick_reads_holds_what_the_far_tests_need():
    N, L = far.FAR_N, 150
    R = N // (L + 1)
    start, length = far.pick_reads(N, R, L, 7)
    again = far.pick_reads(N, R, L, 7)
    assert np.array_equal(start, again[0]) and np.array_equal(length, again[1])
    assert start.dtype == np.int64 and length.dtype == np.int32 and len(start) == len(length) and len(start) % 2 == 0
    have = set(zip(start.tolist(), length.tolist()))
    assert len(have) == len(start), "no entry twice"
    # the seam reads and eight neighbours on each side
    for seam in far.SEAMS:
        i = seam // (L + 1)
        assert i * (L + 1) <= seam - 1 and seam < i * (L + 1) + L, "one read of the generator holds both bytes of the seam"
        assert i in far.seam_reads(N, L)
        for j in range(i - 8, i + 9):
            assert (j * (L + 1), L) in have
    # the ends
    assert (0, L) in have and ((R - 1) * (L + 1), L) in have
    assert any(s + n == N and n > 0 for s, n in have), "a range that ends on byte N - 1"
    # the composites, by size class of their windows at k = 12 .. 47: the 64-lane class (257 .. 2048 windows) twice,
    # the long class with more than 4 * 8192 windows once
    for s, n in far.COMPOSITES:
        assert (s, n) in have and s // (L + 1) != (s + n - 1) // (L + 1)
    for k in (12, 31, 47):
        w = [n - k + 1 for _, n in far.COMPOSITES]
        assert 256 < w[0] <= 2048 and 2048 < w[1] and 4 * 8192 < w[2]
    assert far.COMPOSITES[0][0] < (1 << 32) < sum(far.COMPOSITES[0]) and far.COMPOSITES[1][0] < (1 << 31) < sum(far.COMPOSITES[1])
    # 2 000 reads from above 2^31 besides the seams' neighbours
    plain = [(s, n) for s, n in have if n == L and s % (L + 1) == 0 and 0 <= s < N]
    assert sum(1 for s, _ in plain if s >= 1 << 31) >= 2000
    assert sum(1 for s, _ in plain if s >= 1 << 32) > 0
    # the four entries without a result
    inv = far.invalid_entries(N, L)
    assert all(e in have for e in inv)
    assert inv[0][0] >= N and inv[1][0] < N < sum(inv[1]) and inv[2][0] < 0 and inv[3][1] == 0
    # shuffled
    assert not np.array_equal(np.sort(start), start)
