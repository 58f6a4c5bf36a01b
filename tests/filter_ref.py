"""numpy references of the read filter: the solid span of a read from its windows' oracle counts, the select as plain
array slicing, and the FASTA text of a selected read set.  The window restatement (_windows, _lookup) is
test_gpu_query.py's; the library's own calls are never the reference."""
import numpy as np

SPAN_PREFIX, SPAN_LONGEST = 0, 1
SPAN_DTYPE = np.dtype([("offset", "<i4"), ("length", "<i4")])


def span_rule(solid, k, mode):
    """solid: one bool per window of a read -> (offset, length) in bases.  A run of solid windows a..b covers the bases
    [a, b + k); PREFIX takes the run that begins at window 0, LONGEST the longest run and the earliest on a tie; no
    solid window gives (0, 0)."""
    s = np.asarray(solid, bool)
    if not s.any():
        return 0, 0
    edge = np.diff(np.concatenate([[0], s.astype(np.int8), [0]]))
    first, behind = np.nonzero(edge == 1)[0], np.nonzero(edge == -1)[0]
    runs = behind - first
    if mode == SPAN_PREFIX:
        return (0, int(runs[0]) + k - 1) if first[0] == 0 else (0, 0)
    assert mode == SPAN_LONGEST
    j = int(np.argmax(runs))                                     # (the first of equal maxima)
    return int(first[j]), int(runs[j]) + k - 1


def window_counts(data, k, canonical, want):
    """-> (count uint32 per start position, valid bool per start position) over the whole buffer"""
    from .test_gpu_query import _lookup, _windows
    lo, hi, valid = _windows(data, k, canonical)
    return _lookup(want, lo, hi), valid


def ref_spans(data, start, length, k, min_count, max_count, mode, counts, valid):
    out = np.zeros(len(start), SPAN_DTYPE)
    solid_all = valid & (counts >= min_count) & (counts <= max_count)
    for i, (s, L) in enumerate(zip(start, length)):
        m = max(int(L) - k + 1, 0)
        out[i] = span_rule(solid_all[s:s + m], k, mode)
    return out


def ref_select(data, start, length, spans=None, keep=None, min_len=0):
    """-> (data, start, length, index) of the kept reads, trimmed to their spans, in the native layout"""
    pieces, lens, index = [], [], []
    for i, (s, L) in enumerate(zip(start, length)):
        off, n = (0, int(L)) if spans is None else (int(spans[i]["offset"]), int(spans[i]["length"]))
        if keep is not None and not keep[i]:
            continue
        if off < 0 or n < 0 or off + n > int(L) or n < min_len:
            continue
        pieces.append(data[s + off:s + off + n])
        pieces.append(np.array([-1], np.int8))
        lens.append(n)
        index.append(i)
    o_len = np.array(lens, np.int32)
    o_start = (np.concatenate([[0], np.cumsum(o_len.astype(np.int64) + 1)[:-1]]) if lens else np.zeros(0)).astype(np.int64)
    o_data = np.concatenate(pieces).astype(np.int8) if pieces else np.zeros(0, np.int8)
    return o_data, o_start, o_len, np.array(index, np.int64)


def fasta_text(data, start, length, index):
    lut = np.full(256, ord("N"), np.uint8)
    lut[:4] = np.frombuffer(b"ACGT", np.uint8)
    out = []
    for s, L, i in zip(start, length, index):
        out.append(b">%d\n" % int(i))
        out.append(lut[data[s:s + L].view(np.uint8)].tobytes())
        out.append(b"\n")
    return b"".join(out)
