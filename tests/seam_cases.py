"""Inputs that put a chosen feature at a chosen offset from a chosen seam of the partition front ends -- TEST INFRASTRUCTURE ONLY.

The partition kernels cut the flat read buffer into 32-byte lane chunks; a wave owns 61 of them (msp.hip: P1_OWN, a seam
every 1952 bytes) or 60 (msp2.hip: Q1_OWN, 1920 bytes), the plain 64-lane loaders 64 (2048 bytes); eight waves make a
workgroup tile, and under CFRK_DEBUG_SMALL_PIPELINE a batch of >= 6 tiles is cut into chunks of tiles.  Seam j is buffer
offset j * period.  ladder() builds ONE buffer in which item i -- a feature and an offset delta -- sits at delta from the
seam chosen for it, with invalid codes in between, and asserts that every feature landed where it was asked.
"""
import collections

import numpy as np

PERIOD1, PERIOD2, PERIOD64 = 61 * 32, 60 * 32, 64 * 32
WAVES_PER_TILE = 8
INVALID = np.array(list(range(4, 128)) + list(range(-128, 0)), np.int8)     # every byte value that is no base: 252 of them
WHOLE_CHUNKS = np.array([0x04, 0x7C, -128, -1], np.int8)                    # 0x04, 0x7C, 0x80, 0xFF fill whole 32-byte chunks
MAX_LEN = 300_000

# kind: what the builder asserts at the anchor; data: the feature's bytes; anchor: the index into data (len(data) allowed:
# the byte behind the feature) that lands at seam + delta
Feature = collections.namedtuple("Feature", "kind data anchor")
Placed = collections.namedtuple("Placed", "kind seam delta offset start end")
Ladder = collections.namedtuple("Ladder", "data period placed")


def padding(n, phase=0):
    """n invalid codes: position i holds INVALID[(i + phase) % 252], except that every third 32-byte chunk is filled
    with one of 0x04, 0x7C, 0x80, 0xFF"""
    i = np.arange(n)
    pad = INVALID[(i + phase) % len(INVALID)].copy()
    chunk = i // 32
    whole = chunk % 3 == 0
    pad[whole] = WHOLE_CHUNKS[(chunk[whole] // 3) % 4]
    return pad


def is_base(x):
    return (x >= 0) & (x <= 3)


def bases(rng, n):
    return rng.integers(0, 4, n).astype(np.int8)


# ---------------------------------------------------------------------------- features

def reach(k, W):
    """positions on either side of an invalid base, a read end or a seam that a run's k-mers and window can span"""
    return k + W + 2


def read_start(rng, k, W):
    """a read whose FIRST BASE is the anchor; long enough to cross the seam from every delta of its range"""
    return Feature("start", bases(rng, 3 * reach(k, W) + 80), 0)


def read_end(rng, k, W):
    """a read whose TERMINATOR (last base + 1) is the anchor"""
    r = bases(rng, 3 * reach(k, W) + 80)
    return Feature("end", r, len(r))


def invalid_inside(rng, k, W, code):
    """one invalid code (the anchor) in the middle of a long random read: reach + 40 bases on either side and more"""
    assert not 0 <= code <= 3
    half = 2 * reach(k, W) + 80
    r = bases(rng, 2 * half + 1)
    r[half] = code
    return Feature("invalid", r, half)


def tandem(rng, period, length=160, flank=40):
    """a tandem repeat of the given period (hash ties inside a window) between random flanks; anchor: its first base;
    the kind is tandem<period>_<length>"""
    unit = bases(rng, period)
    while period > 1 and (unit == unit[0]).all():
        unit = bases(rng, period)
    rep = np.tile(unit, length // period + 1)[:length]
    return Feature("tandem%d_%d" % (period, length), np.concatenate([bases(rng, flank), rep, bases(rng, flank)]), flank)


def short_read(rng, length):
    """a whole read of `length` bases; anchor: its first base"""
    return Feature("read%d" % length, bases(rng, length), 0)


def invalid_codes():
    """the invalid codes the features take turns with: the edges of dev_bad4's bit arithmetic first, then all the others"""
    first = [-1, 4, 0x7C, -128, 127, 5, 8, 16, 32, 64, -2, -127, 0x7B, 0x43, -125]
    return first + [int(c) for c in INVALID if int(c) not in first]


def items_for(rng, k, W):
    """every feature of the ladder at every delta of its range -> [(Feature, delta)]"""
    R = reach(k, W)
    codes = invalid_codes()
    out = []
    for d in range(-R, 35):
        out.append((read_start(rng, k, W), d))
        out.append((read_end(rng, k, W), d))
    for i, d in enumerate(range(-R, R + 33)):            # -(k+W+2) .. k+W+34: the smear's whole reach across lanes 61..63 -> 0, 1
        out.append((invalid_inside(rng, k, W, codes[(i + k) % len(codes)]), d))
    for period in (1, 2, 3, 5):
        for a in range(32):                              # the repeat starts at every chunk alignment and crosses the seam
            out.append((tandem(rng, period), -64 + a))
    for L in (k - 1, k, k + W - 1):                      # shorter than k, exactly k, exactly one window: straddling the seam
        for d in (-(L - 1), -(L // 2), -1):
            out.append((short_read(rng, L), d))
    return out


def tile_items_for(rng, k, W):
    """a reduced set for seams that are dear (one per 15 KB tile): the deltas at which something changes"""
    R = reach(k, W)
    codes = invalid_codes()
    out = []
    for i, d in enumerate([-R, -33, -32, -1, 0, 1, 32, k, R + 32]):
        out.append((invalid_inside(rng, k, W, codes[(3 * i + k) % len(codes)]), d))
    for f, d in ((read_start, -R), (read_start, -1), (read_start, 0), (read_end, -1), (read_end, 0), (read_end, 34)):
        out.append((f(rng, k, W), d))
    for period in (1, 2, 3, 5):       # (100 bases: a homopolymer is then < 96 runs, which every leaf stream holds without parking)
        out.append((tandem(rng, period, length=100), -64 + (7 * period + k) % 32))
    return out


# ---------------------------------------------------------------------------- the builder

def ladder(period, items, seams=None, first_seam=1, min_len=0, max_len=MAX_LEN, tail=64, phase=0):
    """ONE buffer: item i = (feature, delta) has its anchor at seams[i] * period + delta (default seams: first_seam,
    first_seam + 1, ...); invalid codes (padding()) everywhere else, at least two between features, `tail` behind the
    last one, more up to min_len.  -> Ladder(data, period, placed)"""
    if seams is None:
        seams = list(range(first_seam, first_seam + len(items)))
    assert len(seams) == len(items) and list(seams) == sorted(set(seams)) and (not seams or seams[0] >= 1)
    spans = []
    for (f, delta), j in zip(items, seams):
        at = j * period + delta
        spans.append((at - f.anchor, at - f.anchor + len(f.data)))
    n = max([min_len] + [e + tail for _, e in spans])
    assert n <= max_len, "a ladder of %d bytes" % n
    data = padding(n, phase)
    prev_end = -2
    placed = []
    for (f, delta), j, (s, e) in zip(items, seams, spans):
        assert s >= prev_end + 2, "features overlap: %s at seam %d, delta %d" % (f.kind, j, delta)
        assert is_base(f.data[[0, -1]]).all()
        data[s:e] = f.data
        prev_end = e
        placed.append(Placed(f.kind, j, delta, j * period + delta, s, e))
    check_ladder(Ladder(data, period, placed), items)
    return Ladder(data, period, placed)


def check_ladder(lad, items=None):
    """what the builder promises, read back from the finished buffer"""
    data, period = lad.data, lad.period
    base = is_base(data)
    covered = np.zeros(len(data), bool)
    for i, p in enumerate(lad.placed):
        assert p.offset == p.seam * period + p.delta and p.start <= p.offset <= p.end
        assert not base[p.start - 1] and not base[p.end]                 # the feature is fenced by invalid codes
        covered[p.start:p.end] = True
        if items is not None:
            assert (data[p.start:p.end] == items[i][0].data).all()
        if p.kind == "start":                                            # first base of a read at seam + delta
            assert p.offset == p.start and base[p.start:p.end].all()
        elif p.kind == "end":                                            # terminator (last base + 1) at seam + delta
            assert p.offset == p.end and base[p.start:p.end].all()
        elif p.kind == "invalid":                                        # the one invalid code of its read at seam + delta
            assert not base[p.offset] and base[p.start:p.offset].all() and base[p.offset + 1:p.end].all()
        elif p.kind.startswith("tandem"):                                # the repeat's first base at seam + delta, the repeat across the seam
            q, L = (int(x) for x in p.kind[6:].split("_"))
            assert p.offset < p.seam * period < p.offset + L - 32 and base[p.start:p.end].all()
            assert (data[p.offset:p.offset + L - q] == data[p.offset + q:p.offset + L]).all()
        else:                                                            # a whole read that straddles the seam
            L = int(p.kind[4:])
            assert p.kind.startswith("read") and p.end - p.start == L and p.offset == p.start
            assert p.start < p.seam * period < p.end and base[p.start:p.end].all()
    pad = data[~covered]
    assert not is_base(pad).any()
    assert set(int(x) for x in np.unique(pad)) == set(int(x) for x in INVALID), "the padding misses an invalid byte value"
    whole = data[:len(data) // 32 * 32].reshape(-1, 32)
    for v in WHOLE_CHUNKS:
        assert (whole == v).all(axis=1).any(), "no whole chunk of 0x%02X" % (int(v) & 0xFF)


def ladders(period, items, first_seam=1, per_buffer=None, min_len=0):
    """the items over as many buffers as it takes (each under MAX_LEN), consecutive seams from first_seam on in each:
    every eighth item sits on a tile seam, and first_seam chooses which"""
    if per_buffer is None:
        per_buffer = MAX_LEN // period - first_seam - 1
    return [ladder(period, items[i:i + per_buffer], first_seam=first_seam, min_len=min_len, phase=i)
            for i in range(0, len(items), per_buffer)]


def tile_ladder(period, items, first_tile=1, every=1):
    """the items on TILE seams (seam index = 0 mod 8): tiles first_tile, first_tile + every, ..."""
    seams = [WAVES_PER_TILE * (first_tile + every * i) for i in range(len(items))]
    return ladder(period, items, seams=seams)


def tiles_of(nbytes, period, two_word=False):
    """workgroup tiles the partition kernel launches over a buffer (msp2.hip plans for nN + 32: a k-mer may start in
    the chunk before its window)"""
    span = WAVES_PER_TILE * period
    return (nbytes + (32 if two_word else 0) + span - 1) // span


def pipeline_chunk_tiles(ntiles):
    """CFRK_DEBUG_SMALL_PIPELINE (msp.hip: msp_count_tiles): min(5, ntiles / 3) chunks of ceil(ntiles / chunks) tiles;
    -> the tiles at which a chunk starts (none: the batch is not cut)"""
    nchunks = min(5, ntiles // 3)
    if nchunks < 2:
        return []
    per = -(-ntiles // nchunks)
    return list(range(per, ntiles, per))


# ---------------------------------------------------------------------------- the buffer's end, the buffer's start

def end_buffers(rng, period, k, W, seam=1, deltas=range(-33, 34)):
    """buffers that END at seam * period + e for every e (all residues mod 32; the byte-wise tail chunk, `off < nN` and
    msp2.hip's `off < nN + 32`), a long read running into the end: with a trailing terminator (the last byte is an invalid
    code) and without (the last byte is a base) -> [(e, terminated, data)]"""
    out = []
    for e in deltas:
        nN = seam * period + e
        for terminated in (False, True):
            data = padding(nN, phase=e + 40)
            L = 3 * reach(k, W) + 40
            stop = nN - 1 if terminated else nN
            data[stop - L:stop] = bases(rng, L)
            assert len(data) == nN and is_base(data[-1]) != terminated and is_base(data[stop - 1]) and not is_base(data[stop - L - 1])
            out.append((e, terminated, data))
    return out


def head_buffers(rng, k, W, offsets=range(0, 41)):
    """the very first wave (lane 0 loads chunk -1): a read's first base, a read's terminator and an invalid base inside a
    read at offsets 0..40 of the buffer -> [(kind, offset, data)]"""
    out = []
    L = 2 * reach(k, W) + 60
    codes = invalid_codes()
    for o in offsets:
        d = np.concatenate([padding(o, o), bases(rng, L), padding(8, 3)])
        assert is_base(d[o]) and (o == 0 or not is_base(d[o - 1]))
        out.append(("start", o, d))
        if o >= 1:
            d = np.concatenate([bases(rng, o), padding(3, o), bases(rng, L), padding(8, 5)])   # (a read shorter than k for small o)
            assert not is_base(d[o]) and is_base(d[o - 1])
            out.append(("end", o, d))
        d = bases(rng, L + 41)
        d[o] = codes[(o + k) % len(codes)]
        d = np.concatenate([d, padding(8, 7)])
        assert not is_base(d[o]) and is_base(d[o + 1])
        out.append(("invalid", o, d))
    return out
