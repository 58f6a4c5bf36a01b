"""Plain-Python statement of the unitig contract (include/cfrk_abi.h, "unitigs"): dictionaries and strings, nothing
shared with the product.  k-mers are strings over ACGT; a count table is {k-mer string: count} holding the keys as
the job stores them (canonical k-mers in a canonical job)."""
import numpy as np

BASES = "ACGT"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def rc(s):
    return "".join(COMP[c] for c in reversed(s))


def count_kmers(seqs, k, canonical, times=1, table=None):
    """{k-mer: count} of every window of every string, each counted `times` times"""
    table = {} if table is None else table
    for s in seqs:
        for i in range(len(s) - k + 1):
            w = s[i:i + k]
            if canonical:
                w = min(w, rc(w))
            table[w] = table.get(w, 0) + times
    return table


def key_of(s):
    """(lo, hi) of a k-mer: first base most significant, A < C < G < T"""
    v = 0
    for c in s:
        v = v * 4 + BASES.index(c)
    return v & 0xFFFFFFFFFFFFFFFF, v >> 64


def str_of(lo, hi, k):
    v = (int(hi) << 64) | int(lo)
    return "".join(BASES[(v >> (2 * (k - 1 - i))) & 3] for i in range(k))


def neighbor_mask(table, key, k, canonical, min_count=1):
    """bit b: key[1:] + b is there with count >= min_count; bit 4 + b: b + key[:-1] is"""
    t = max(1, min_count)

    def there(s):
        if canonical:
            s = min(s, rc(s))
        return table.get(s, 0) >= t
    m = 0
    for b in range(4):
        if there(key[1:] + BASES[b]):
            m |= 1 << b
        if there(BASES[b] + key[:-1]):
            m |= 16 << b
    return m


def unitigs(table, k, canonical, min_count=1):
    """-> [(sequence, kc, n_kmers, circular)] in ascending order of the first k-mer"""
    t = max(1, min_count)
    solid = {x: c for x, c in table.items() if c >= t}
    O = set(solid)
    if canonical:
        O |= {rc(x) for x in solid}
    node = (lambda a: min(a, rc(a))) if canonical else (lambda a: a)
    pal = (lambda a: a == rc(a)) if canonical else (lambda a: False)
    succ = lambda a: [a[1:] + b for b in BASES if a[1:] + b in O]
    pred = lambda a: [b + a[:-1] for b in BASES if b + a[:-1] in O]
    nxt, prv = {}, {}
    for a in O:
        s = succ(a)
        if len(s) != 1:
            continue
        b = s[0]
        if pred(b) != [a] or node(a) == node(b) or pal(a) or pal(b):
            continue
        nxt[a] = b
        prv[b] = a
    out, seen = [], set()

    def emit(path, circular):
        seq = path[0] + "".join(a[-1] for a in path[1:])
        out.append((path[0], seq, sum(solid[node(a)] for a in path), len(path), circular))

    for a in sorted(O):                                 # paths, from their heads
        if a in prv:
            continue
        path = [a]
        while path[-1] in nxt:
            path.append(nxt[path[-1]])
        seen.update(path)
        if canonical:
            last = rc(path[-1])
            if not (a < last or (a == last and len(path) == 1)):
                continue                                # the mirror image is the one that is emitted
            assert a != last or pal(a)
        emit(path, False)
    for a in sorted(O):                                 # what is left lies on cycles; sorted: the smallest comes first
        if a in seen:
            continue
        path = [a]
        while nxt[path[-1]] != a:
            path.append(nxt[path[-1]])
        seen.update(path)
        if canonical:
            mirror = {rc(x) for x in path}
            assert not (mirror & set(path))
            seen.update(mirror)                         # a < every k-mer of both: this cycle is the one emitted
        emit(path, True)
    out.sort()
    assert len({o[0] for o in out}) == len(out)
    return [o[1:] for o in out]


UNITIG_DTYPE = np.dtype([("kc", "<u8"), ("n_kmers", "<u4"), ("flags", "<u4")])


def layout(units):
    """the struct-read layout of a unitig list -> (data int8, start int64, length int32, rec)"""
    data, start, length = [], [], []
    rec = np.zeros(len(units), UNITIG_DTYPE)
    pos = 0
    for j, (seq, kc, n, circ) in enumerate(units):
        start.append(pos)
        length.append(len(seq))
        data.extend(BASES.index(c) for c in seq)
        data.append(-1)
        pos += len(seq) + 1
        rec[j] = (kc, n, 1 if circ else 0)
    return np.array(data, np.int8), np.array(start, np.int64), np.array(length, np.int32), rec


def fasta_text(units):
    """what --unitigs-out writes"""
    lines = []
    for j, (seq, kc, n, circ) in enumerate(units):
        tenths = (kc * 10 + n // 2) // n                # kc / n to one decimal, halves rounded up
        lines.append(">%d LN:i:%d KC:i:%d km:f:%d.%d%s\n%s\n" % (j, len(seq), kc, tenths // 10, tenths % 10,
                                                                 " CL:i:1" if circ else "", seq))
    return "".join(lines).encode()
