"""The component rules of include/cfrk_abi.h ("Unitig components", "Read components") in plain Python: a dictionary
union-find over the link rows and a loop over a read's hits, and the two text formats of the cfrk command."""
import numpy as np

COMP_NONE = 0xFFFFFFFF
SPLIT, DROPPED = 1, 2
UNITIG_COMPONENT_DTYPE = np.dtype([("kc", "<u8"), ("n_kmers", "<u8"), ("n_links", "<u8"), ("first", "<u4"), ("n_unitigs", "<u4")])
READ_COMPONENT_DTYPE = np.dtype([("comp", "<u4"), ("hit", "<u4"), ("n_windows", "<u4"), ("flags", "<u4")])


def components(rec, link_ptr, links, drop=None):
    """records (kc, n_kmers, flags), the link CSR, drop[nS] or None -> (comp uint32[nS], table, stats)"""
    nS = len(rec)
    kept = [drop is None or not drop[j] for j in range(nS)]
    parent = {}

    def find(x):
        while parent.setdefault(x, x) != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    to = links["to"].tolist()
    ptr = [int(x) for x in link_ptr]
    n_links = [0] * nS
    for j in range(nS):
        if not kept[j]:
            continue
        for t in range(ptr[j], ptr[j + 1]):
            if kept[to[t]]:
                n_links[j] += 1
                a, b = find(j), find(to[t])
                if a != b:
                    parent[max(a, b)] = min(a, b)
    comp = np.full(nS, COMP_NONE, np.uint32)
    rows, number = [], {}
    kc, nk = rec["kc"].tolist(), rec["n_kmers"].tolist()
    for j in range(nS):                                     # ascending: a component is first met at its smallest unitig
        if not kept[j]:
            continue
        r = find(j)
        if r not in number:
            number[r] = len(rows)
            rows.append([0, 0, 0, j, 0])
        c = number[r]
        comp[j] = c
        row = rows[c]
        row[0] = (row[0] + kc[j]) & (2 ** 64 - 1)
        row[1] += nk[j]
        row[2] += n_links[j]
        row[4] += 1
    table = np.array([tuple(r) for r in rows], UNITIG_COMPONENT_DTYPE).reshape(len(rows))
    stats = {"n_components": len(rows), "n_unitigs": sum(kept), "n_kmers": sum(r[1] for r in rows), "n_links": sum(r[2] for r in rows)}
    return comp, table, stats


def components_bfs(nS, link_ptr, links, drop=None):
    """the same partition by a breadth-first search over the undirected graph -> comp"""
    kept = [drop is None or not drop[j] for j in range(nS)]
    adj = [[] for _ in range(nS)]
    to = links["to"].tolist()
    for j in range(nS):
        for t in range(int(link_ptr[j]), int(link_ptr[j + 1])):
            if kept[j] and kept[to[t]]:
                adj[j].append(to[t])
                adj[to[t]].append(j)
    comp = np.full(nS, COMP_NONE, np.uint32)
    n = 0
    for s in range(nS):
        if not kept[s] or comp[s] != COMP_NONE:
            continue
        comp[s] = n
        queue = [s]
        while queue:
            nxt = []
            for u in queue:
                for v in adj[u]:
                    if comp[v] == COMP_NONE:
                        comp[v] = n
                        nxt.append(v)
            queue = nxt
        n += 1
    return comp


def read_components(hit_ptr, hits, comp):
    """the hit CSR and comp[nS] -> (rows READ_COMPONENT_DTYPE[nR], stats)"""
    nR = len(hit_ptr) - 1
    rows = np.zeros(nR, READ_COMPONENT_DTYPE)
    stats = {"n_assigned": 0, "n_unassigned": 0, "n_split": 0, "n_dropped": 0}
    unitig, nwin = hits["unitig"].tolist(), hits["n_windows"].tolist()
    comp = [int(c) for c in comp]
    for i in range(nR):
        best, flags = None, 0
        a, b = int(hit_ptr[i]), int(hit_ptr[i + 1])
        for h in range(a, b):
            if comp[unitig[h]] == COMP_NONE:
                flags |= DROPPED
            elif best is None or nwin[h] > nwin[best]:
                best = h
        if best is None:
            rows[i] = (COMP_NONE, COMP_NONE, 0, flags)
            stats["n_unassigned"] += 1
        else:
            c = comp[unitig[best]]
            if any(comp[unitig[h]] not in (COMP_NONE, c) for h in range(a, b)):
                flags |= SPLIT
            rows[i] = (c, best - a, nwin[best], flags)
            stats["n_assigned"] += 1
        stats["n_split"] += bool(flags & SPLIT)
        stats["n_dropped"] += bool(flags & DROPPED)
    return rows, stats


def mean_text(kc, n):
    """kc / n_kmers with one decimal, as the km:f: tag prints it"""
    n = n or 1
    tenths = (kc * 10 + n // 2) // n
    return "%d.%d" % (tenths // 10, tenths % 10)


def components_text(table, k):
    """CFILE: one line per component, `id first n_unitigs n_kmers bases kc mean n_links`"""
    out = []
    for c, (kc, nk, nl, first, nu) in enumerate(table.tolist()):
        out.append("%d\t%d\t%d\t%d\t%d\t%d\t%s\t%d\n" % (c, first, nu, nk, nk + nu * (k - 1), kc, mean_text(kc, nk), nl))
    return "".join(out)


def read_components_text(rows):
    """RFILE: one line per read, `id hit n_windows flags`; a read with no component gets `*` for its id and hit"""
    out = []
    for c, h, n, f in rows.tolist():
        out.append("*\t*\t0\t%d\n" % f if c == COMP_NONE else "%d\t%d\t%d\t%d\n" % (c, h, n, f))
    return "".join(out)


def tagged_fasta(text, comp):
    """UFILE with --unitigs-component-tags: ` CC:i:<id>` behind the km:f: (and CL:i:1) tag, in front of any L: tag"""
    out, j = [], 0
    for line in text.decode().split("\n"):
        if line.startswith(">"):
            if comp[j] != COMP_NONE:
                at = line.find(" L:")
                at = len(line) if at < 0 else at
                line = line[:at] + " CC:i:%d" % comp[j] + line[at:]
            j += 1
        out.append(line)
    return "\n".join(out).encode()


def tagged_gfa(text, comp):
    """GFILE with --unitigs-component-tags: `CC:i:<id>` as the last tag of every S line"""
    out, j = [], 0
    for line in text.decode().split("\n"):
        if line.startswith("S\t"):
            if comp[j] != COMP_NONE:
                line += "\tCC:i:%d" % comp[j]
            j += 1
        out.append(line)
    return "\n".join(out).encode()
