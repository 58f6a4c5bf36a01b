"""Plain-Python statement of the bubble rule and the simplify loop (include/cfrk_abi.h, "Unitig bubbles"): sets and Python
integers over the unitig list of tests/unitig_ref.py and the link rows of tests/unitig_links_ref.py, nothing shared with
the product.  The properties the header states are asserted here, on every graph the reference is asked about."""
import numpy as np

from . import tips_ref as tr
from . import unitig_ref as ur

NONE = 0xFFFFFFFF


def _arms(n, circ, L, max_kmers, canonical):
    """-> {oriented arm x: (src(x), dst(x))}"""
    out_, in_ = {}, {}
    for a, b in L:
        out_.setdefault(a, set()).add(b)
        in_.setdefault(b, set()).add(a)
    arms = {}
    for j in range(len(n)):
        for o in ((0, 1) if canonical else (0,)):
            x = (j, o)
            if circ[j] or n[j] > max_kmers or len(in_.get(x, ())) != 1 or len(out_.get(x, ())) != 1:
                continue
            (src,), (dst,) = in_[x], out_[x]
            if src[0] != j and dst[0] != j:
                arms[x] = (src, dst)
    return arms


def _decide(n, kc, circ, L, canonical, max_kmers, max_diff, ratio_q8):
    """-> (arm[j], pop[j], partner[j]) of the graph with the oriented links L"""
    nS = len(n)
    arms = _arms(n, circ, L, max_kmers, canonical)
    if canonical:                                       # (j,-) is an arm iff (j,+) is, ends swapped and mirrored
        mirror = lambda a: (a[0], 1 - a[1])
        for (j, o), (src, dst) in arms.items():
            assert arms.get((j, 1 - o)) == (mirror(dst), mirror(src))
    classes = {}
    for x, ends in arms.items():
        classes.setdefault(ends, []).append(x)

    def above(s, j):                                    # s ranks above j
        a, b = kc[s] * n[j], kc[j] * n[s]
        return a > b or (a == b and s < j)

    pop, partner = [False] * nS, [NONE] * nS
    for j in range(nS):
        if (j, 0) not in arms:
            continue
        beat = [(s, p) for s, p in classes[arms[(j, 0)]]
                if s != j and abs(n[j] - n[s]) <= max_diff and 256 * kc[s] * n[j] >= ratio_q8 * kc[j] * n[s] and above(s, j)]
        if not beat:
            continue
        best = beat[0][0]
        for s, _ in beat:
            if above(s, best):
                best = s
        pop[j] = True
        partner[j] = best << 1 | min(p for s, p in beat if s == best)
    # the best-ranked arm of every (src, dst) class stays
    for members in classes.values():
        top = members[0][0]
        for s, _ in members:
            if above(s, top):
                top = s
        assert not pop[top]
    return [(j, 0) in arms for j in range(nS)], pop, partner


def bubbles(units, link_ptr, links, canonical, max_kmers, max_diff, ratio_q8):
    """units as ur.unitigs() returns them, the rows as lr.links() does -> (pop np.uint8[nS], partner np.uint32[nS])"""
    assert 0 <= ratio_q8 <= tr.RATIO_Q8_MAX and max_kmers >= 0 and max_diff >= 0
    nS = len(units)
    n, kc, circ = [u[2] for u in units], [u[1] for u in units], [bool(u[3]) for u in units]
    L = tr._oriented(link_ptr, links, nS, canonical)
    arm, pop, partner = _decide(n, kc, circ, L, canonical, max_kmers, max_diff, ratio_q8)
    assert all(a or not p for a, p in zip(arm, pop))
    assert all((w == NONE) == (not p) and (p == 0 or w >> 1 < nS) for p, w in zip(pop, partner))
    if canonical:
        # every unitig replaced by its mirror image: (j,+) and (j,-) change places in every link, nothing else changes
        flipped = {((u, 1 - ou), (v, 1 - ov)) for (u, ou), (v, ov) in L}
        assert _decide(n, kc, circ, flipped, canonical, max_kmers, max_diff, ratio_q8) == (arm, pop, partner)
    else:
        assert all(w == NONE or w & 1 == 0 for w in partner)
    # a popped unitig has no dead end: it is no candidate of the tip rule, whatever the tip rule's parameters
    cand, _ = tr._decide(n, kc, circ, L, 1 << 32, 0)
    assert not any(p and c for p, c in zip(pop, cand))
    if max_kmers == 0:
        assert not any(pop)
    return np.array(pop, np.uint8).reshape(nS), np.array(partner, np.uint32).reshape(nS)


def arms(units, link_ptr, links, canonical, max_kmers):
    n, circ = [u[2] for u in units], [bool(u[3]) for u in units]
    found = _arms(n, circ, tr._oriented(link_ptr, links, len(units), canonical), max_kmers, canonical)
    return [(j, 0) in found for j in range(len(units))]


def simplify(table, k, canonical, min_count=1, tips=True, bubbles_=True, rounds=4, tip_max_kmers=None, tip_ratio_q8=512,
             bubble_max_kmers=None, bubble_max_diff=0, bubble_ratio_q8=0):
    """the loop: unitigs -> links -> each enabled rule on that same graph -> drop the k-mers of tip | pop, until a round
    finds neither or `rounds` rounds are done -> (units of the simplified graph, [(unitigs, tips, bubbles, masked keys so
    far)], the reduced dictionary, [(round, popped j, partner, popped unit, partner's unit)])"""
    tip_max_kmers = k if tip_max_kmers is None else tip_max_kmers
    bubble_max_kmers = k if bubble_max_kmers is None else bubble_max_kmers
    report, rows, masked = [], [], set()
    units, link_ptr, links = tr.graph(table, k, canonical, min_count)
    for rnd in range(1, rounds + 1):
        nS = len(units)
        tip = tr.tips(units, link_ptr, links, canonical, tip_max_kmers, tip_ratio_q8) if tips else np.zeros(nS, np.uint8)
        if bubbles_:
            pop, partner = bubbles(units, link_ptr, links, canonical, bubble_max_kmers, bubble_max_diff, bubble_ratio_q8)
        else:
            pop, partner = np.zeros(nS, np.uint8), np.full(nS, NONE, np.uint32)
        assert not (tip & pop).any()
        for j in np.flatnonzero(tip | pop):
            new = tr.unit_kmers(units[j][0], k, canonical)
            assert all(x in table and x not in masked for x in new)
            masked.update(new)
        for j in np.flatnonzero(pop).tolist():
            rows.append((rnd, j, int(partner[j]), units[j], units[int(partner[j]) >> 1]))
        report.append((nS, int(tip.sum()), int(pop.sum()), len(masked)))
        if not (tip.any() or pop.any()):
            break
        table = tr.masked_table(table, masked)
        units, link_ptr, links = tr.graph(table, k, canonical, min_count)
    return units, report, table, rows


def report_text(report):
    """what --tip-report writes with --unitigs-pop-bubbles: five fields"""
    return "".join("%d\t%d\t%d\t%d\t%d\n" % ((i + 1,) + r) for i, r in enumerate(report)).encode()


def _km(kc, n):
    tenths = (kc * 10 + n // 2) // n                    # kc / n to one decimal, halves rounded up: the S line's km
    return "%d.%d" % (tenths // 10, tenths % 10)


def bubble_lines(rows):
    """what --bubble-report writes: round, popped name, kept name, kept strand, LN popped, LN kept, km popped, km kept, kind,
    popped sequence, kept sequence oriented like the popped one"""
    out = []
    for rnd, j, partner, (seq, kc, n, _), (kseq, kkc, kn, _) in rows:
        kept = ur.rc(kseq) if partner & 1 else kseq
        if len(seq) != len(kept):
            kind = "indel"
        else:
            kind = "snp" if sum(a != b for a, b in zip(seq, kept)) == 1 else "mnp"
        out.append("%d\t%d\t%d\t%s\t%d\t%d\t%s\t%s\t%s\t%s\t%s\n" % (rnd, j, partner >> 1, "-" if partner & 1 else "+", len(seq), len(kept),
                                                                 _km(kc, n), _km(kkc, kn), kind, seq, kept))
    return "".join(out).encode()
