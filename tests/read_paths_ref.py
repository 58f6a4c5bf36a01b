"""Plain-Python statement of the path and link-support contract (include/cfrk_abi.h, "Read paths and link support"):
lists and tuples over the hit rows of tests/read_hits_ref.py and the link rows of tests/unitig_links_ref.py, nothing shared
with the product.  A hit is (unitig, unitig_at, read_off, n_windows); a link row is (to, flags).  Every call asserts the
consequences the contract lists; those that need the graph and the reads are asserted by graph_paths()."""
import numpy as np

from . import unitig_ref as ur

FROM_MINUS, TO_MINUS = 1, 2
READ_PATH_DTYPE = np.dtype([("hit_first", "<u4"), ("n_hits", "<u4"), ("read_off", "<u4"), ("n_windows", "<u4")])
STAT_NAMES = ("n_paths", "n_steps", "n_gaps", "n_unlinked")


def link_rows(link_ptr, links):
    """the CSR -> one list per unitig of (r, to, flags), r the index into links"""
    flat = [(int(t), int(f)) for t, f in np.asarray(links).tolist()]
    return [[(r,) + flat[r] for r in range(int(link_ptr[j]), int(link_ptr[j + 1]))] for j in range(len(link_ptr) - 1)]


def enters_at_head(hit, n_kmers):
    j, at, _, n = hit
    m, off = at & 1, at >> 1
    return (off + n - 1 if m else off) == (n_kmers[j] - 1 if m else 0)


def leaves_at_end(hit, n_kmers):
    j, at, _, n = hit
    m, off = at & 1, at >> 1
    return (off if m else off + n - 1) == (0 if m else n_kmers[j] - 1)


def step(h, g, n_kmers, rows):
    """consecutive hits h, g of one read -> ("gap", None), ("unlinked", None) or ("step", r)"""
    if g[2] != h[2] + h[3]:
        return "gap", None
    if leaves_at_end(h, n_kmers) and enters_at_head(g, n_kmers):
        want = (FROM_MINUS if h[1] & 1 else 0) | (TO_MINUS if g[1] & 1 else 0)
        for r, to, flags in rows[h[0]]:
            if to == g[0] and flags == want:
                return "step", r
    return "unlinked", None


def paths(hits_of_read, n_kmers, rows):
    """the hits of one read -> (paths [(hit_first, n_hits, read_off, n_windows)], links of its steps [r], gaps, unlinked)"""
    out, steps, gaps, unlinked = [], [], 0, 0
    for i, h in enumerate(hits_of_read):
        what, r = step(hits_of_read[i - 1], h, n_kmers, rows) if i else ("first", None)
        if what == "step":
            first, n, off, win = out[-1]
            out[-1] = (first, n + 1, off, win + h[3])
            steps.append(r)
        else:
            out.append((i, 1, h[2], h[3]))
            gaps += what == "gap"
            unlinked += what == "unlinked"
    assert sum(p[1] for p in out) == len(hits_of_read)
    assert [p[0] for p in out] == sorted({p[0] for p in out})
    assert len(out) + len(steps) == len(hits_of_read) and len(out) == (1 + gaps + unlinked if hits_of_read else 0)
    return out, steps, gaps, unlinked


def path_rows(hit_ptr, hits, n_kmers, link_ptr, links, support=None):
    """CSR in, CSR out -> (path_ptr int64[nR + 1], paths READ_PATH_DTYPE, support uint32[n_links], stats dict).  support
    is added to (a copy of) the array given."""
    rows = link_rows(link_ptr, links)
    flat = [tuple(int(x) for x in h) for h in np.asarray(hits).tolist()]
    sup = np.zeros(len(links), np.uint32) if support is None else np.array(support, np.uint32)
    before = int(sup.astype(np.uint64).sum())
    ptr, out, st = [0], [], dict.fromkeys(STAT_NAMES, 0)
    for i in range(len(hit_ptr) - 1):
        p, steps, gaps, unlinked = paths(flat[int(hit_ptr[i]):int(hit_ptr[i + 1])], n_kmers, rows)
        out += p
        ptr.append(len(out))
        for r in steps:
            sup[r] += 1
        st["n_paths"] += len(p)
        st["n_steps"] += len(steps)
        st["n_gaps"] += gaps
        st["n_unlinked"] += unlinked
    assert int(sup.astype(np.uint64).sum()) - before == st["n_steps"]
    assert st["n_paths"] + st["n_steps"] == int(hit_ptr[-1])
    return np.array(ptr, np.int64), np.array(out, READ_PATH_DTYPE).reshape(-1), sup, st


def spelled(G, hits_of_path):
    """the sequence a chain of hits walks: the first unitig whole, of every further one what follows its first k - 1
    bases, reverse-complemented for '-'"""
    s = ""
    for i, (j, at, _, _) in enumerate(hits_of_path):
        u = ur.rc(G.seqs[j]) if at & 1 else G.seqs[j]
        s += u if i == 0 else u[G.k - 1:]
    return s


def first_ps(G, hit):
    j, at, _, n = hit
    m = n + G.k - 1
    return len(G.seqs[j]) - (at >> 1) - m if at & 1 else at >> 1


def graph_paths(G, link_ptr, links, reads, complete=True, support=None):
    """the reads on graph G (read_hits_ref.Graph) through the link CSR -> (hit_ptr, hits, path_ptr, paths, support, stats),
    with the consequences that need the sequences asserted; complete: the CSR is G's whole link set"""
    k = G.k
    n_kmers = [len(s) - k + 1 for s in G.seqs]
    hit_ptr, hits = G.hit_rows(reads)
    path_ptr, prow, sup, st = path_rows(hit_ptr, hits, n_kmers, link_ptr, links, support)
    flat = [tuple(int(x) for x in h) for h in hits.tolist()]
    for i, read in enumerate(reads):
        mine = flat[int(hit_ptr[i]):int(hit_ptr[i + 1])]
        got = [tuple(int(x) for x in p) for p in prow[int(path_ptr[i]):int(path_ptr[i + 1])].tolist()]
        for first, n, off, win in got:
            chain = mine[first:first + n]
            ps, m = first_ps(G, chain[0]), win + k - 1
            assert spelled(G, chain)[ps:ps + m] == read[off:off + m] and len(read[off:off + m]) == m
        if complete:
            # the maximal runs of located windows, from locate() alone
            W = max(0, len(read) - k + 1)
            loc = [G.locate(read[w:w + k]) is not None for w in range(W)]
            runs, w = [], 0
            while w < W:
                if not loc[w]:
                    w += 1
                    continue
                b = w
                while b + 1 < W and loc[b + 1]:
                    b += 1
                runs.append((w, b - w + 1))
                w = b + 1
            assert [(p[2], p[3]) for p in got] == runs, (i, got, runs)
    if complete:
        assert st["n_unlinked"] == 0
    return hit_ptr, hits, path_ptr, prow, sup, st


def gaf_paths_text(unitig_lengths, k, read_lengths, hit_ptr, hits, path_ptr, prow):
    """what --unitigs-map-out writes with --unitigs-map-paths: one line per path in CSR order"""
    flat = [tuple(int(x) for x in h) for h in np.asarray(hits).tolist()]
    lines = []
    for i, rl in enumerate(read_lengths):
        for first, n, off, win in np.asarray(prow)[int(path_ptr[i]):int(path_ptr[i + 1])].tolist():
            chain = flat[int(hit_ptr[i]) + first:int(hit_ptr[i]) + first + n]
            m = win + k - 1
            j, at, _, hn = chain[0]
            ln, hm = unitig_lengths[j], hn + k - 1
            ps = ln - (at >> 1) - hm if at & 1 else at >> 1
            pl = sum(unitig_lengths[h[0]] for h in chain) - (n - 1) * (k - 1)
            name = "".join(("<" if h[1] & 1 else ">") + str(h[0]) for h in chain)
            lines.append("%d\t%d\t%d\t%d\t+\t%s\t%d\t%d\t%d\t%d\t%d\t255\tcg:Z:%d=\n" % (i, rl, off, off + m, name, pl, ps, ps + m, m, m, m))
    return "".join(lines).encode()


def mirror_row(rows, u, r):
    """the first row (v,!ov) -> (u,!ou) for link r = (u,ou) -> (v,ov) of row u, None when v has no such row"""
    _, v, f = next(x for x in rows[u] if x[0] == r)
    want = (0 if f & TO_MINUS else FROM_MINUS) | (0 if f & FROM_MINUS else TO_MINUS)
    return next((x[0] for x in rows[v] if x[1] == u and x[2] == want), None) if v < len(rows) else None


def gfa_support_text(units, k, link_ptr, links, support, canonical):
    """what --unitigs-gfa writes with --unitigs-link-support: the GFA with RC:i: on every L line"""
    rows = link_rows(link_ptr, links)
    out = ["H\tVN:Z:1.0\n"]
    for j, (seq, kc, n, _) in enumerate(units):
        tenths = (kc * 10 + n // 2) // n
        out.append("S\t%d\t%s\tLN:i:%d\tKC:i:%d\tkm:f:%d.%d\n" % (j, seq, len(seq), kc, tenths // 10, tenths % 10))
    for j, row in enumerate(rows):
        for r, to, f in row:
            c = int(support[r])
            if canonical:
                mr = mirror_row(rows, j, r)
                if mr is not None and mr != r:
                    c += int(support[mr])
            out.append("L\t%d\t%s\t%d\t%s\t%dM\tRC:i:%d\n" % (j, "-" if f & FROM_MINUS else "+", to, "-" if f & TO_MINUS else "+", k - 1, c))
    return "".join(out).encode()


def stats_text(n_reads, n_hits, st):
    """what --unitigs-map-stats writes"""
    return ("%d\t%d\t%d\t%d\t%d\t%d\n" % (n_reads, n_hits, st["n_paths"], st["n_steps"], st["n_gaps"], st["n_unlinked"])).encode()
