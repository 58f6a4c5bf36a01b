"""The word arithmetic of the partition front end on inputs chosen for it: the canonical m-mer taken as the minimum of two
TOP-aligned windows (msp_dev.h: msp_minimizers), the chunk loader's invalid mask built nibble by nibble from gathers that
carry junk above the nibble (common.h: dev_load_chunk32), and the validity smear on three 32-bit words (msp.hip: p1_tile).

  1. ties in the top bits: reads whose m-mers equal their own reverse complement, or whose forward and reverse windows
     share their top 2m bits and differ below;
  2. nibble order and junk: two invalid bytes in one 4-byte word or on either side of a word boundary, byte values whose
     flag arithmetic differs (bit 7, bits 2..6, both);
  3. the smear's width across two lanes: two invalid bytes k - 1 .. k + W bases apart, the first at the edges and the
     middle of a chunk, in the middle of a wave and around a wave seam.

Expected values never come from the partitioned path: records and record counts are tests/msp_ref.py, counts are
tests/oracle_lib.global_count.  Every buffer is 2 - 8 KB and stays, by the reference's own count, below 2048 records per
level-1 sub-region and at or below 96 per leaf stream (the smallest sizes msp_count_tiles gives them), so nothing parks.
"""
import numpy as np
import pytest

from . import msp_ref
from .test_gpu_partition_seams import MIN_REGION, MIN_STRIDE, check_small, export_decoded, same_records, stream_loads

pytestmark = pytest.mark.gpu

PERIOD1 = 1952                    # bytes a wave of msp_p1b_kernel owns: 61 lanes of 32
JUNK = [4, 0x08, 0x40, 0x7C, 0x80, 0xFC, 0xFF]


@pytest.fixture(scope="module")
def ctx():
    import cfrk_amd
    c = cfrk_amd.Context(0)
    yield c
    c.close()


def nothing_parks(data, k):
    """from the reference alone: no leaf stream over its smallest stride, no level-1 sub-region at its smallest size"""
    fullest, _, fullest_region = stream_loads(data, k)
    return fullest <= MIN_STRIDE and fullest_region < MIN_REGION


def code(v):
    return np.array(v, np.uint8).astype(np.int8)


# ---------------------------------------------------------------------------- 1: ties in the top bits

def tie_reads(rng):
    """(AT)n, (ACGT)n, (AACGTT)n -- every unit its own reverse complement, so at even m every other m-mer is a palindrome
    and at odd m the forward window of one position is the reverse window of a neighbour -- and a random 40-mer followed by
    its reverse complement: palindromic m-mers across the joint, at every even m.  Each read ends in a terminator."""
    a40 = rng.integers(0, 4, 40)
    reads = [np.tile([0, 3], 50), np.tile([0, 1, 2, 3], 25), np.tile([0, 0, 1, 2, 3, 3], 17), np.concatenate([a40, 3 - a40[::-1]])]
    return np.concatenate([np.concatenate([r, [-1]]) for r in reads]).astype(np.int8)


# k = 26, 30, 31, 32: m = 12, 13, 14, 16; two-word keys: m = 14 at odd k, 13 at even k
@pytest.mark.parametrize("k", [26, 30, 31, 32, 33, 34])
def test_ties_in_the_top_bits_of_the_two_windows(ctx, k):
    assert msp_ref.params(k).m == {26: 12, 30: 13, 31: 14, 32: 16, 33: 14, 34: 13}[k]
    reads = tie_reads(np.random.default_rng(3700 + k))
    for pad in (0, 17):
        data = np.concatenate([np.full(pad, -1, np.int8), reads, np.full(2048 - pad - len(reads), -1, np.int8)])
        rr = msp_ref.runs(data, k)
        assert len(rr) >= 40 and nothing_parks(data, k)
        got, hdr = export_decoded(ctx, data, k)
        same_records(got, hdr, rr)
        check_small(ctx, data, k)


# ---------------------------------------------------------------------------- 2: nibble order, junk in the gather

def pairs_in_a_chunk():
    """byte offsets (a, b) inside a 32-byte chunk: both in one 4-byte word -- all six pairs, in words 0, 3, 4 and 7 (the
    first and last word of either 16-byte load) -- and the last byte of a word with the first of the next, all seven"""
    out = [(4 * w + i, 4 * w + j) for w in (0, 3, 4, 7) for i in range(4) for j in range(i + 1, 4)]
    out += [(4 * w + 3, 4 * w + 4) for w in range(7)]
    assert len(out) == 31
    return out


@pytest.mark.parametrize("k", [17, 31])
def test_two_invalid_bytes_in_and_across_the_words_of_a_chunk(ctx, k):
    rng = np.random.default_rng(3800 + k)
    read = rng.integers(0, 4, 4096).astype(np.int8)
    used = {(JUNK[n % 7], JUNK[(n // 7 + n + 3) % 7]) for n in range(31)}
    assert {a for a, _ in used} == set(JUNK) == {b for _, b in used} and len(used) >= 21     # every value first and second
    for n, (a, b) in enumerate(pairs_in_a_chunk()):
        data = read.copy()
        chunk = 32 * (20 + n)                               # (a chunk of its own per pair, all in the wave's middle)
        data[chunk + a] = code(JUNK[n % 7])
        data[chunk + b] = code(JUNK[(n // 7 + n + 3) % 7])
        assert nothing_parks(data, k)
        check_small(ctx, data, k, canonical=n % 2 == 0)


# ---------------------------------------------------------------------------- 3: the smear across two lanes

def smear_cases(k, base, nbytes):
    """two invalid bytes d apart, d = k - 1, k, k + 1, k + W - 1, k + W, the first at byte 0, 15, 16, 31 from `base`: the
    second lies one or two lanes ahead; the k-mers between them are none, none, one, W - 1 and W"""
    W = msp_ref.params(k).W
    rng = np.random.default_rng(3900 + k + base)
    read = rng.integers(0, 4, nbytes).astype(np.int8)
    for i, p in enumerate((0, 15, 16, 31)):
        for j, d in enumerate((k - 1, k, k + 1, k + W - 1, k + W)):
            data = read.copy()
            data[base + p] = code(JUNK[(i + j) % 7])
            data[base + p + d] = code(JUNK[(2 * i + j + 1) % 7])
            yield p, d, data


@pytest.mark.parametrize("where", ["mid_wave", "wave_seam"])
@pytest.mark.parametrize("k", [16, 17, 24, 31, 32])
def test_two_invalid_bytes_a_smear_apart(ctx, k, where):
    base, nbytes = (32 * 9, 2048) if where == "mid_wave" else (PERIOD1 - 40, 4096)
    for p, d, data in smear_cases(k, base, nbytes):
        assert nothing_parks(data, k)
        check_small(ctx, data, k, canonical=(p + d) % 2 == 0)
