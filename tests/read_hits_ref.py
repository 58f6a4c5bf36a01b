"""Plain-Python statement of the position and hit contract (include/cfrk_abi.h, "Unitig positions and read hits"):
dictionaries and strings over unitig_ref.unitigs(), nothing shared with the product.  Reads are strings over ACGT with
any other character (N) as an invalid code.  Every call asserts the consequences the contract lists."""
import numpy as np

from . import unitig_ref as ur

POS_NONE = 0xFFFFFFFF
UNITIG_POS_DTYPE = np.dtype([("unitig", "<u4"), ("at", "<u4")])
READ_HIT_DTYPE = np.dtype([("unitig", "<u4"), ("unitig_at", "<u4"), ("read_off", "<u4"), ("n_windows", "<u4")])


class Graph:
    """the unitigs of a count table at a threshold, and where every solid key lies on them"""

    def __init__(self, table, k, canonical, min_count=1):
        self.k, self.canonical = k, canonical
        t = max(1, min_count)
        self.solid = {x for x, c in table.items() if c >= t}
        self.O = set(self.solid) | ({ur.rc(x) for x in self.solid} if canonical else set())
        self.units = ur.unitigs(table, k, canonical, min_count)
        self.seqs = [u[0] for u in self.units]
        self.where = {}                                     # node -> (j, p)
        for j, s in enumerate(self.seqs):
            for p in range(len(s) - k + 1):
                n = self.node(s[p:p + k])
                assert n not in self.where, "a solid key lies in one unitig once"
                self.where[n] = (j, p)
                if canonical and s[p:p + k] == ur.rc(s[p:p + k]):
                    assert len(s) == k, "a palindromic k-mer is a single-node unitig"
        assert set(self.where) == self.solid

    def node(self, a):
        return min(a, ur.rc(a)) if self.canonical else a

    def locate(self, x):
        """the position of oriented k-mer x exactly as given -> (j, p, minus) or None"""
        if len(x) != self.k or any(c not in ur.BASES for c in x) or x not in self.O:
            return None
        j, p = self.where[self.node(x)]
        kmer = self.seqs[j][p:p + self.k]
        minus = 0 if x == kmer else 1
        assert minus == 0 or (self.canonical and x == ur.rc(kmer))
        return j, p, minus

    def hits(self, read):
        """the hits of one read -> [(unitig, unitig_at, read_off, n_windows)]"""
        k = self.k
        W = max(0, len(read) - k + 1)
        pos = [self.locate(read[w:w + k]) for w in range(W)]

        def colinear(a, b):
            if a is None or b is None or a[0] != b[0] or a[2] != b[2]:
                return False
            return b[1] == (a[1] - 1 if a[2] else a[1] + 1)
        out, w = [], 0
        while w < W:
            if pos[w] is None:
                w += 1
                continue
            b = w
            while b + 1 < W and colinear(pos[b], pos[b + 1]):
                b += 1
            j, _, minus = pos[w]
            off, n = min(pos[w][1], pos[b][1]), b - w + 1
            out.append((j, off << 1 | minus, w, n))
            w = b + 1
        # the consequences
        located = sum(1 for w in range(W) if all(c in ur.BASES for c in read[w:w + k]) and read[w:w + k] in self.O)
        assert sum(h[3] for h in out) == located == sum(p is not None for p in pos)
        for a, b in zip(out, out[1:]):
            assert a[2] + a[3] <= b[2]
        for j, at, a, n in out:
            piece = self.seqs[j][(at >> 1):(at >> 1) + n + k - 1]
            assert len(piece) == n + k - 1
            assert read[a:a + n + k - 1] == (ur.rc(piece) if at & 1 else piece)
        if len(read) < k:
            assert not out
        return out

    def locate_rows(self, kmers):
        out = np.full(len(kmers), POS_NONE, np.uint32).repeat(2).view(UNITIG_POS_DTYPE)
        for i, x in enumerate(kmers):
            r = self.locate(x)
            if r is not None:
                out[i] = (r[0], r[1] << 1 | r[2])
        return out

    def hit_rows(self, reads):
        """CSR over reads -> (hit_ptr int64[n + 1], hits READ_HIT_DTYPE)"""
        ptr, rows = [0], []
        for r in reads:
            rows.extend(self.hits(r))
            ptr.append(len(rows))
        return np.array(ptr, np.int64), np.array(rows, READ_HIT_DTYPE).reshape(-1)

    def gaf_text(self, reads):
        """what --unitigs-map-out writes: one line per hit in CSR order, the segment names those of --unitigs-gfa"""
        lines = []
        for i, r in enumerate(reads):
            for j, at, a, n in self.hits(r):
                m, ln, off = n + self.k - 1, len(self.seqs[j]), at >> 1
                ps = ln - off - m if at & 1 else off
                lines.append("%d\t%d\t%d\t%d\t+\t%s%d\t%d\t%d\t%d\t%d\t%d\t255\tcg:Z:%d=\n" % (
                    i, len(r), a, a + m, "<" if at & 1 else ">", j, ln, ps, ps + m, m, m, m))
        return "".join(lines).encode()


def read_codes(reads):
    """strings -> (data, start, length) in the struct-read layout; a character outside ACGT is the code -1"""
    data, start, length = [], [], []
    for s in reads:
        start.append(len(data))
        length.append(len(s))
        data.extend(ur.BASES.index(c) if c in ur.BASES else -1 for c in s)
        data.append(-1)
    return np.array(data, np.int8), np.array(start, np.int64), np.array(length, np.int32)
