"""Plain-Python statement of the compaction contract (include/cfrk_abi.h, "Unitig compaction"): the unitigs of the graph
without the dropped unitigs, from the unitig list of tests/unitig_ref.py and the link rows of tests/unitig_links_ref.py
alone.  Strings, sets and dictionaries; no dictionary of k-mers, nothing shared with the product."""
import numpy as np

from . import unitig_links_ref as lr
from . import unitig_ref as ur

POS_NONE = 0xFFFFFFFF
POS_DTYPE = np.dtype([("unitig", "<u4"), ("at", "<u4")])


def oriented(seq, o):
    return ur.rc(seq) if o else seq


def merges(units, link_ptr, links, drop, k, canonical):
    """-> {(u, ou): (v, ov)}: the merges among the surviving oriented unitigs"""
    nS = len(units)
    out_, in_ = {}, {}
    for j in range(nS):
        for to, f in links[link_ptr[j]:link_ptr[j + 1]].tolist():
            if drop[j] or drop[to]:
                continue
            a, b = (j, 1 if f & lr.FROM_MINUS else 0), (to, 1 if f & lr.TO_MINUS else 0)
            out_.setdefault(a, []).append(b)
            in_.setdefault(b, []).append(a)
    pal = lambda u: canonical and units[u][2] == 1 and units[u][0] == ur.rc(units[u][0])
    nxt = {}
    for x, outs in out_.items():
        if len(outs) != 1:
            continue
        y = outs[0]
        if in_[y] != [x]:
            continue
        (u, ou), (v, ov) = x, y
        if units[u][3] or units[v][3]:
            continue                                    # an input cycle is a component of its own
        if v == u and (ov != ou or units[u][2] == 1):
            continue                                    # a hairpin; the self-link of a single node
        if pal(u) or pal(v):
            continue
        assert oriented(units[u][0], ou)[-(k - 1):] == oriented(units[v][0], ov)[:k - 1] or k == 1
        nxt[x] = y
    return nxt


def compact(units, link_ptr, links, drop, k, canonical):
    """units as ur.unitigs() returns them, the rows as lr.links() does, drop[nS] -> (units of the graph without the dropped
    ones, in the same form and order, into POS_DTYPE[nS], {"merged": components of two or more members, "closed": cycles that
    close only now, "closed_mirror": those of them whose smallest k-mer lies on the mirror of the ring as first met})"""
    nS = len(units)
    drop = [bool(d) for d in (drop if drop is not None else [0] * nS)]
    oris = (0, 1) if canonical else (0,)
    nxt = merges(units, link_ptr, links, drop, k, canonical)
    prv = {y: x for x, y in nxt.items()}
    assert len(prv) == len(nxt)
    spell = lambda chain: "".join(oriented(units[u][0], o)[(k - 1 if i else 0):] for i, (u, o) in enumerate(chain))
    comps, seen = [], set()                             # (first k-mer, seq, kc, n, circ, [(member, offset in k-mers)])
    n_merged = n_closed = n_mirror = 0

    def offsets(chain):
        at, off = [], 0
        for u, _ in chain:
            at.append(off)
            off += units[u][2]
        return at

    for u in range(nS):                                 # paths, from their heads
        for o in oris:
            x = (u, o)
            if drop[u] or x in prv or x in seen:
                continue
            if units[u][3]:                             # an input cycle: copied, written as (u,+)
                seen.update((u, p) for p in oris)
                comps.append((units[u][0][:k], units[u][0], units[u][1], units[u][2], True, [(x, 0)]))
                continue
            chain = [x]
            while chain[-1] in nxt:
                chain.append(nxt[chain[-1]])
            mirror = [(v, 1 - p) for v, p in reversed(chain)]
            seen.update(chain)
            if canonical:
                assert not set(mirror) & set(chain) or (len(chain) == 1 and units[u][0] == ur.rc(units[u][0]))
                seen.update(mirror)
                if spell(mirror)[:k] < spell(chain)[:k]:
                    chain = mirror
            seq = spell(chain)
            n_merged += len(chain) > 1
            comps.append((seq[:k], seq, sum(units[v][1] for v, _ in chain), sum(units[v][2] for v, _ in chain), False,
                          list(zip(chain, offsets(chain)))))
    for u in range(nS):                                 # what is left lies on cycles of merges
        for o in oris:
            x = (u, o)
            if drop[u] or x in seen:
                continue
            ring = [x]
            while nxt[ring[-1]] != x:
                ring.append(nxt[ring[-1]])
            seen.update(ring)
            cands = [ring]
            if canonical:
                mirror = [(v, 1 - p) for v, p in reversed(ring)]
                assert not set(mirror) & set(ring)
                seen.update(mirror)
                cands.append(mirror)
            best = None
            for r in cands:
                n = sum(units[v][2] for v, _ in r)
                full = spell(r)                         # n + k - 1 bases: the first k - 1 once more at the end
                assert full[:k - 1] == full[n:]
                loop = full[:n]
                for p in range(n):
                    kmer = (loop * (k // n + 2))[p:p + k]
                    if best is None or kmer < best[0]:
                        best = (kmer, r, p, n, loop)
            kmer, r, p, n, loop = best
            rot = loop[p:] + loop[:p]
            seq = (rot * (k // n + 2))[:n + k - 1]
            assert seq[:k] == kmer
            n_closed += 1
            n_mirror += r is not ring
            n_merged += len(r) > 1
            comps.append((kmer, seq, sum(units[v][1] for v, _ in r), n, True, [(m, (a - p) % n) for m, a in zip(r, offsets(r))]))
    comps.sort(key=lambda c: c[0])
    assert len({c[0] for c in comps}) == len(comps)
    into = np.full(nS, POS_NONE, POS_DTYPE)
    for j, c in enumerate(comps):
        for (u, o), off in c[5]:
            assert into[u]["unitig"] == POS_NONE
            into[u] = (j, off << 1 | o)
    assert all((into[u]["unitig"] == POS_NONE) == drop[u] for u in range(nS))
    return [c[1:5] for c in comps], into, {"merged": n_merged, "closed": n_closed, "closed_mirror": n_mirror}


def check_into(units, new_units, into, drop, k):
    """input j covers s_new[off : off + length[j]] (mod n_kmers in a circular output), or its reverse complement"""
    for j, (seq, _, _, _) in enumerate(units):
        if drop is not None and drop[j]:
            assert tuple(into[j].tolist()) == (POS_NONE, POS_NONE)
            continue
        t, at = int(into[j]["unitig"]), int(into[j]["at"])
        new, _, n, circ = new_units[t]
        off, minus = at >> 1, at & 1
        want = ur.rc(seq) if minus else seq
        if circ:
            loop = new[:n]
            got = "".join(loop[(off + i) % n] for i in range(len(seq)))
        else:
            got = new[off:off + len(seq)]
        assert got == want, (j, t, at)
