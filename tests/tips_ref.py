"""Plain-Python statement of the tip rule and the graph mask (include/cfrk_abi.h, "Unitig tips" and "Graph mask"): sets
and Python integers over the unitig list of tests/unitig_ref.py and the link rows of tests/unitig_links_ref.py, nothing
shared with the product.  A masked graph is simply the graph of the dictionary without the masked keys."""
import numpy as np

from . import unitig_links_ref as lr
from . import unitig_ref as ur

RATIO_Q8_MAX = 65536


def masked_table(table, keys, canonical=False):
    """the dictionary without `keys` (k-mer strings; canonicalised in a canonical job; absent ones are ignored)"""
    gone = {min(x, ur.rc(x)) for x in keys} if canonical else set(keys)
    return {x: c for x, c in table.items() if x not in gone}


def _oriented(link_ptr, links, nS, canonical):
    """the CSR rows as a set of ((u, ou), (v, ov)), o = 0 for + and 1 for -"""
    assert len(link_ptr) == nS + 1 and link_ptr[0] == 0 and link_ptr[nS] == len(links)
    L = set()
    for j in range(nS):
        assert link_ptr[j] <= link_ptr[j + 1]
        for to, f in links[link_ptr[j]:link_ptr[j + 1]].tolist():
            assert to < nS and f & ~3 == 0 and (canonical or f == 0)
            L.add(((j, 1 if f & lr.FROM_MINUS else 0), (to, 1 if f & lr.TO_MINUS else 0)))
    if canonical:
        assert all(((v, 1 - ov), (u, 1 - ou)) in L for (u, ou), (v, ov) in L)     # the rows hold every link's mirror
    return L


def _decide(n, kc, circ, L, max_kmers, ratio_q8):
    """-> (candidate[j], tip[j]) of the graph with the oriented links L"""
    nS = len(n)
    out_, in_ = {}, {}
    for a, b in L:
        out_.setdefault(a, set()).add(b)
        in_.setdefault(b, set()).add(a)
    right = [len(out_.get((j, 0), ())) for j in range(nS)]
    left = [len(in_.get((j, 0), ())) for j in range(nS)]
    cand = [not circ[j] and n[j] <= max_kmers and ((left[j] == 0) != (right[j] == 0)) for j in range(nS)]

    def beats(w, j):
        if 256 * kc[w] * n[j] < ratio_q8 * kc[j] * n[w]:
            return False
        a, b = kc[w] * n[j], kc[j] * n[w]                   # mean(w) > mean(j) iff a > b
        return not cand[w] or a > b or (a == b and w < j)

    tip = []
    for j in range(nS):
        if not cand[j]:
            tip.append(False)
            continue
        if right[j] == 0:       # attachments: in(j,+); siblings: the other targets of the attaching oriented unitig
            sib = {w for u in in_[(j, 0)] for w, _ in out_.get(u, ()) if w != j}
        else:                   # attachments: out(j,+); siblings: the other sources of the attached oriented unitig
            sib = {w for v in out_[(j, 0)] for w, _ in in_.get(v, ()) if w != j}
        tip.append(any(beats(w, j) for w in sib))
    return cand, tip


def tips(units, link_ptr, links, canonical, max_kmers, ratio_q8):
    """units as ur.unitigs() returns them, the rows as lr.links() does -> np.uint8[nS], 1 for a tip"""
    assert 0 <= ratio_q8 <= RATIO_Q8_MAX and max_kmers >= 0
    nS = len(units)
    n, kc, circ = [u[2] for u in units], [u[1] for u in units], [bool(u[3]) for u in units]
    L = _oriented(link_ptr, links, nS, canonical)
    cand, tip = _decide(n, kc, circ, L, max_kmers, ratio_q8)
    assert all(c or not t for c, t in zip(cand, tip))           # tips are candidates
    if canonical:
        # every unitig replaced by its mirror image: (j,+) and (j,-) change places in every link, nothing else changes
        flipped = {((u, 1 - ou), (v, 1 - ov)) for (u, ou), (v, ov) in L}
        assert _decide(n, kc, circ, flipped, max_kmers, ratio_q8) == (cand, tip)
    if max_kmers == 0:
        assert not any(tip)
    return np.array(tip, np.uint8).reshape(nS)


def candidates(units, link_ptr, links, canonical, max_kmers):
    n, kc, circ = [u[2] for u in units], [u[1] for u in units], [bool(u[3]) for u in units]
    return _decide(n, kc, circ, _oriented(link_ptr, links, len(units), canonical), max_kmers, 0)[0]


def unit_kmers(seq, k, canonical):
    out = [seq[i:i + k] for i in range(len(seq) - k + 1)]
    return [min(x, ur.rc(x)) for x in out] if canonical else out


def graph(table, k, canonical, min_count=1):
    """-> (units, link_ptr, links) of a dictionary"""
    units = ur.unitigs(table, k, canonical, min_count)
    return (units,) + lr.links(units, table, k, canonical, min_count)


def clip(table, k, canonical, min_count=1, max_kmers=None, ratio_q8=512, rounds=4):
    """the clip loop: unitigs -> links -> tips -> drop the tips' k-mers, until a round finds no tip or `rounds` rounds are
    done -> (units of the clipped graph, [(unitigs, tips, masked keys so far)], the reduced dictionary)"""
    max_kmers = k if max_kmers is None else max_kmers
    report, masked = [], set()
    units, link_ptr, links = graph(table, k, canonical, min_count)
    for _ in range(rounds):
        tip = tips(units, link_ptr, links, canonical, max_kmers, ratio_q8)
        for j in np.flatnonzero(tip):
            new = unit_kmers(units[j][0], k, canonical)
            assert all(x in table and x not in masked for x in new)
            masked.update(new)
        report.append((len(units), int(tip.sum()), len(masked)))
        if not tip.any():
            break
        table = masked_table(table, masked)
        units, link_ptr, links = graph(table, k, canonical, min_count)
    return units, report, table


def report_text(report):
    """what --tip-report writes"""
    return "".join("%d\t%d\t%d\t%d\n" % ((i + 1,) + r) for i, r in enumerate(report)).encode()
