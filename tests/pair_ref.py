"""Paired-end reads (the pairs section of include/cfrk_abi.h) in plain Python -- TEST INFRASTRUCTURE ONLY.

The rules of the header, word for word: which read survives, how the two mates' survival is joined (BOTH with orphans,
EITHER without), what the identifier of a header line is and when two mates carry the same one, and paired
normalisation as normalize_ref.normalize_keys' loop with the join between judge and insert.  Nothing here knows how the
device does it."""
import numpy as np

from tests import normalize_ref as nref

BOTH, EITHER = 0, 1


def survives(keep, span, length, min_len):
    """one read: keep byte (None: no keep array), span (offset, length) or None, length of the read or None"""
    if keep is not None and int(keep) == 0:
        return False
    if span is not None:
        off, n = int(span[0]), int(span[1])
        if off < 0 or n < 0 or off + n > int(length):
            return False
        return n >= min_len
    return length is None or int(length) >= min_len


def survive_all(n, keep=None, spans=None, length=None, min_len=0):
    at = lambda a, i: None if a is None else a[i]
    return [survives(at(keep, i), at(spans, i), at(length, i), min_len) for i in range(n)]


def join(sa, sb, mode):
    """survival of the A mates and of the B mates -> (pair, orphan_a, orphan_b uint8 arrays, counts (pairs, orphans A,
    orphans B, dropped))"""
    assert mode in (BOTH, EITHER) and len(sa) == len(sb)
    n = len(sa)
    pair, oa, ob = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    for j, (a, b) in enumerate(zip(sa, sb)):
        if mode == EITHER:
            pair[j] = 1 if (a or b) else 0
        else:
            pair[j] = 1 if (a and b) else 0
            oa[j] = 1 if (a and not b) else 0
            ob[j] = 1 if (b and not a) else 0
    dropped = sum(1 for j in range(n) if not (pair[j] or oa[j] or ob[j]))
    return pair, oa, ob, (int(pair.sum()), int(oa.sum()), int(ob.sum()), dropped)


def identifier(text, rec):
    """bytes of the header line behind the marker up to the first space or tab; None when the header range does not lie
    inside the text"""
    off, n, size = int(rec["head_off"]), int(rec["head_len"]), len(text)
    if off < 0 or n < 0 or off > size or n > size - off:
        return None
    name = bytes(text[off + 1:off + n]) if n > 1 else b""
    for i, c in enumerate(name):
        if c in b" \t":
            return name[:i]
    return name


def pair_good(text_a, rec_a, text_b, rec_b):
    a, b = identifier(text_a, rec_a), identifier(text_b, rec_b)
    if a is None or b is None:
        return False
    if a.endswith(b"/1") and b.endswith(b"/2"):
        a, b = a[:-2], b[:-2]
    return a == b and len(a) > 0


def check_pairs(text_a, recs_a, text_b, recs_b):
    """-> (first_bad or -1, n_bad); recs_a[j] and recs_b[j] are the mates of pair j"""
    bad = [j for j in range(len(recs_a)) if not pair_good(text_a, recs_a[j], text_b, recs_b[j])]
    return (bad[0] if bad else -1), len(bad)


def normalize_pairs_keys(keys, cutoff, batch, mode, counts=None):
    """normalize_ref.normalize_keys for interleaved pairs (reads 2j, 2j + 1): per round judge every mate, join the two
    verdicts of every pair, insert every kept read's keys -> (keep, n_kept, counts)"""
    counts = {} if counts is None else counts
    nS = len(keys)
    assert nS % 2 == 0 and batch % 2 == 0 and batch >= 2
    keep = np.zeros(nS, np.uint8)
    for r0 in range(0, nS, batch):
        r1 = min(r0 + batch, nS)
        verdict = [bool(keys[i]) and nref.lower_median([counts.get(x, 0) for x in keys[i]]) < cutoff for i in range(r0, r1)]
        pair, _, _, _ = join(verdict[0::2], verdict[1::2], mode)
        for j, p in enumerate(pair):
            keep[r0 + 2 * j] = keep[r0 + 2 * j + 1] = p
        for i in range(r0, r1):
            if keep[i]:
                for x in keys[i]:
                    counts[x] = min(counts.get(x, 0) + 1, nref.COUNT_MAX)
    return keep, int(keep.sum()), counts


def normalize_pairs(data, start, length, k, canonical, cutoff, batch, mode, counts=None):
    return normalize_pairs_keys(nref.all_read_keys(data, start, length, k, canonical), cutoff, batch, mode, counts)
