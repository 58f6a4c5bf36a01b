"""Plain-Python statement of the bulge rule (include/cfrk_abi.h, "Unitig bulges"): an arm beside a chain of unitigs.  Lists
and Python integers over the unitig list of tests/unitig_ref.py and the link rows of tests/unitig_links_ref.py, nothing
shared with the product.  The rows keep their order, because the order of the search is part of the contract: `visits`
is compared too.  The properties the header states are asserted here, on every real graph the reference is asked about;
rows that are no real link set get the bare statement of the rule (bulges_rows)."""
import numpy as np

from . import bubbles_ref as br
from . import tips_ref as tr
from . import unitig_links_ref as lr
from . import unitig_ref as ur

MAX_HOPS, MAX_VISITS = 64, 65536


def _out_rows(link_ptr, links, nS, canonical):
    """{oriented unitig: [oriented target, ...]} in row order; a canonical row is split by CFRK_LINK_FROM_MINUS"""
    out = {}
    for j in range(nS):
        for to, f in links[link_ptr[j]:link_ptr[j + 1]].tolist():
            frm = (j, 1 if canonical and f & lr.FROM_MINUS else 0)
            out.setdefault(frm, []).append((to, 1 if canonical and f & lr.TO_MINUS else 0))
    return out


def _arms(n, circ, out, canonical, max_kmers):
    """{j: (src, dst)} for the arms (j,+), read off the rows as the header says: in(j,+) of a canonical job is the mirrored
    FROM_MINUS part of row j, otherwise every link of every row that names j"""
    nS = len(n)
    ins = {}
    if canonical:
        for j in range(nS):
            ins[j] = [(v, 1 - ov) for v, ov in out.get((j, 1), ())]
    else:
        for (u, _), row in out.items():
            for v, _ in row:
                ins.setdefault(v, []).append((u, 0))
    arms = {}
    for j in range(nS):
        o, i = out.get((j, 0), ()), ins.get(j, ())
        if circ[j] or n[j] > max_kmers or len(i) != 1 or len(o) != 1 or i[0][0] == j or o[0][0] == j:
            continue
        arms[j] = (i[0], o[0])
    return arms


def _eligible(n, kc, w, j, ratio_q8):
    a, b = kc[w] * n[j], kc[j] * n[w]
    return 256 * a >= ratio_q8 * b and (a > b or (a == b and w < j))


def _search(n, kc, out, j, s, t, max_diff, max_hops, max_visits, ratio_q8):
    """the depth-first search of the header -> (found, path, visits); visits = max_visits + 1 for an undecided arm"""
    lo, hi = n[j] - max_diff, n[j] + max_diff
    banned = {j, s[0], t[0]}
    visits = 0
    path, cursor, total = [], [0], 0            # cursor[d]: the next link of out(cur at depth d)
    while True:
        d = len(path)
        cur = path[-1] if path else s
        row = out.get(cur, ())
        if cursor[d] == len(row):               # this row is done: back to the one above, or the search is over
            if not path:
                return False, [], visits
            total -= n[path.pop()[0]]
            cursor.pop()
            continue
        if visits == max_visits:
            return False, [], max_visits + 1
        visits += 1
        y = row[cursor[d]]
        cursor[d] += 1
        if y == t and d >= 1 and total >= lo:
            return True, list(path), visits
        if (_eligible(n, kc, y[0], j, ratio_q8) and y[0] not in banned and all(y[0] != w for w, _ in path) and d < max_hops
                and total + n[y[0]] <= hi):
            path.append(y)
            cursor.append(0)
            total += n[y[0]]


def _decide(n, kc, circ, out, canonical, max_kmers, max_diff, max_hops, max_visits, ratio_q8):
    """-> (arms {j: (s, t)}, pop[j], visits[j], paths {j: [oriented unitig, ...]})"""
    nS = len(n)
    arms = _arms(n, circ, out, canonical, max_kmers)
    pop, visits, paths = [False] * nS, [0] * nS, {}
    for j, (s, t) in arms.items():
        found, path, visits[j] = _search(n, kc, out, j, s, t, max_diff, max_hops, max_visits, ratio_q8)
        if found:
            pop[j], paths[j] = True, path
    return arms, pop, visits, paths


def _pack(nS, arms, pop, visits, paths):
    path_ptr = np.zeros(nS + 1, np.int64)
    for j, p in paths.items():
        path_ptr[j + 1] = len(p)
    np.cumsum(path_ptr, out=path_ptr)
    flat = [w << 1 | o for j in sorted(paths) for w, o in paths[j]]
    return np.array(pop, np.uint8).reshape(nS), np.array(visits, np.uint32).reshape(nS), path_ptr, np.array(flat, np.uint32).reshape(len(flat))


def _check_args(max_kmers, max_diff, max_hops, max_visits, ratio_q8):
    assert max_kmers >= 0 and max_diff >= 0 and 0 <= max_hops <= MAX_HOPS and 0 <= max_visits <= MAX_VISITS
    assert 0 <= ratio_q8 <= tr.RATIO_Q8_MAX


def _result(nS, arms, pop, visits, paths, max_visits):
    pop_a, visits_a, path_ptr, path = _pack(nS, arms, pop, visits, paths)
    stats = (len(arms), int(sum(pop)), sum(1 for j in arms if visits[j] == max_visits + 1))
    return pop_a, visits_a, path_ptr, path, stats


def bulges_rows(rec, link_ptr, links, canonical, max_kmers, max_diff, max_hops, max_visits, ratio_q8):
    """the rule on records (kc, n_kmers, flags) and rows as given, real link set or not -> (pop, visits, path_ptr, path,
    (arms, popped, undecided)).  Only what makes the statement well defined is asked of the rows."""
    _check_args(max_kmers, max_diff, max_hops, max_visits, ratio_q8)
    nS = len(rec)
    n, kc, circ = [int(x) for x in rec["n_kmers"]], [int(x) for x in rec["kc"]], [bool(x & 1) for x in rec["flags"]]
    assert len(link_ptr) == nS + 1 and link_ptr[0] == 0 and link_ptr[nS] == len(links) and (links["to"] < nS).all()
    out = _out_rows(link_ptr, links, nS, canonical)
    return _result(nS, *_decide(n, kc, circ, out, canonical, max_kmers, max_diff, max_hops, max_visits, ratio_q8), max_visits)


def _reaches(L_out, s, t, allowed):
    """is there a walk s -> .. -> t whose interior unitigs are all `allowed`"""
    seen, todo = set(), [s]
    while todo:
        a = todo.pop()
        for b in L_out.get(a, ()):
            if b == t:
                return True
            if b not in seen and allowed(b[0]):
                seen.add(b)
                todo.append(b)
    return False


def bulges(units, link_ptr, links, canonical, max_kmers, max_diff=0, max_hops=None, max_visits=1024, ratio_q8=0):
    """units as ur.unitigs() returns them, the rows as lr.links() does -> (pop np.uint8[nS], visits np.uint32[nS], path_ptr
    np.int64[nS + 1], path np.uint32[n_path], (arms, popped, undecided)), the header's properties asserted"""
    max_hops = min(max_kmers + max_diff, MAX_HOPS) if max_hops is None else max_hops
    _check_args(max_kmers, max_diff, max_hops, max_visits, ratio_q8)
    nS = len(units)
    n, kc, circ = [u[2] for u in units], [u[1] for u in units], [bool(u[3]) for u in units]
    L = tr._oriented(link_ptr, links, nS, canonical)            # (asserts that these are real rows, mirrors and all)
    out = _out_rows(link_ptr, links, nS, canonical)
    assert {(a, b) for a, row in out.items() for b in row} == L and sum(len(r) for r in out.values()) == len(L)
    args = (max_kmers, max_diff, max_hops, max_visits, ratio_q8)
    arms, pop, visits, paths = _decide(n, kc, circ, out, canonical, *args)
    # the arms are the bubble rule's
    assert arms == {j: ends for (j, o), ends in br._arms(n, circ, L, max_kmers, canonical).items() if o == 0}
    undecided = {j for j in arms if visits[j] == max_visits + 1}
    assert all(visits[j] == 0 for j in range(nS) if j not in arms) and all(visits[j] <= max_visits + 1 for j in arms)
    assert set(paths) == {j for j in range(nS) if pop[j]} and not undecided & set(paths)
    # paths are real paths of eligible, distinct, non-excluded unitigs within the length window
    for j, path in paths.items():
        s, t = arms[j]
        assert 1 <= len(path) <= max_hops
        for a, b in zip([s] + path, path + [t]):
            assert (a, b) in L
        ws = [w for w, _ in path]
        assert len(set(ws)) == len(ws) and not {j, s[0], t[0]} & set(ws)
        assert all(_eligible(n, kc, w, j, ratio_q8) for w in ws)
        assert n[j] - max_diff <= sum(n[w] for w in ws) <= n[j] + max_diff
    # a popped unitig has no dead end, nor has an interior unitig of a path: disjoint from any tip[]
    cand, tip = tr._decide(n, kc, circ, L, 1 << 32, 0)
    assert not any(cand[j] for j in paths) and not any(cand[w] for p in paths.values() for w, _ in p)
    # with the bubble rule's pops and the tips of the same graph removed as well, s still reaches t
    bpop = br._decide(n, kc, circ, L, canonical, max_kmers, max_diff, ratio_q8)[1]
    gone = {j for j in range(nS) if pop[j] or bpop[j] or tip[j]}
    L_out = {}
    for a, b in L:
        L_out.setdefault(a, []).append(b)
    for j in paths:
        s, t = arms[j]
        assert _reaches(L_out, s, t, lambda w: w not in gone and w != j)
    # every unitig the bubble rule pops is popped here or undecided
    if max_hops >= 1:
        assert all(pop[j] or j in undecided for j in range(nS) if bpop[j])
    if max_kmers == 0 or max_hops == 0:
        assert not any(pop)
    if canonical:
        # every unitig replaced by its mirror image: the mirrored search decides the same unless one runs out of budget
        flipped = {(u, 1 - o): [(v, 1 - ov) for v, ov in row] for (u, o), row in out.items()}
        farms, fpop, fvisits, _ = _decide(n, kc, circ, flipped, canonical, *args)
        assert set(farms) == set(arms)
        assert all(pop[j] == fpop[j] for j in arms if j not in undecided and fvisits[j] != max_visits + 1)
    else:
        assert all(o == 0 for p in paths.values() for _, o in p)
    return _result(nS, arms, pop, visits, paths, max_visits)


def spell(units, path, k):
    """the sequence of a path of oriented unitigs (w << 1 | o), spelled with k - 1 overlaps"""
    seqs = [ur.rc(units[w >> 1][0]) if w & 1 else units[w >> 1][0] for w in path]
    assert all(a[len(a) - k + 1:] == b[:k - 1] for a, b in zip(seqs, seqs[1:]))
    return seqs[0] + "".join(s[k - 1:] for s in seqs[1:])


def simplify(table, k, canonical, min_count=1, tips=True, bubbles_=True, bulges_=True, rounds=4, tip_max_kmers=None, tip_ratio_q8=512,
             bubble_max_kmers=None, bubble_max_diff=0, bubble_ratio_q8=0, bulge_max_kmers=None, bulge_max_diff=0, bulge_max_hops=None,
             bulge_max_visits=1024, bulge_ratio_q8=0):
    """the loop: unitigs -> links -> each enabled rule on that same graph -> drop the k-mers of tip | pop | bulge, until a
    round finds none or `rounds` rounds are done -> (units of the simplified graph, [(unitigs, tips, bubbles, bulges, masked
    keys so far)], the reduced dictionary, the bubble rows of bubbles_ref, [(round, popped j, path, popped unit, the
    path's sequence)])"""
    tip_max_kmers = k if tip_max_kmers is None else tip_max_kmers
    bubble_max_kmers = k if bubble_max_kmers is None else bubble_max_kmers
    bulge_max_kmers = k if bulge_max_kmers is None else bulge_max_kmers
    report, rows, bulge_rows, masked = [], [], [], set()
    units, link_ptr, links = tr.graph(table, k, canonical, min_count)
    for rnd in range(1, rounds + 1):
        nS = len(units)
        tip = tr.tips(units, link_ptr, links, canonical, tip_max_kmers, tip_ratio_q8) if tips else np.zeros(nS, np.uint8)
        if bubbles_:
            pop, partner = br.bubbles(units, link_ptr, links, canonical, bubble_max_kmers, bubble_max_diff, bubble_ratio_q8)
        else:
            pop, partner = np.zeros(nS, np.uint8), np.full(nS, br.NONE, np.uint32)
        if bulges_:
            bulge, _, path_ptr, path, _ = bulges(units, link_ptr, links, canonical, bulge_max_kmers, bulge_max_diff, bulge_max_hops,
                                                 bulge_max_visits, bulge_ratio_q8)
        else:
            bulge, path_ptr, path = np.zeros(nS, np.uint8), np.zeros(nS + 1, np.int64), np.zeros(0, np.uint32)
        assert not (tip & (pop | bulge)).any()
        for j in np.flatnonzero(tip | pop | bulge):
            new = tr.unit_kmers(units[j][0], k, canonical)
            assert all(x in table and x not in masked for x in new)
            masked.update(new)
        for j in np.flatnonzero(pop).tolist():
            rows.append((rnd, j, int(partner[j]), units[j], units[int(partner[j]) >> 1]))
        for j in np.flatnonzero(bulge).tolist():
            p = path[path_ptr[j]:path_ptr[j + 1]].tolist()
            bulge_rows.append((rnd, j, p, units[j], spell(units, p, k)))
        report.append((nS, int(tip.sum()), int(pop.sum()), int(bulge.sum()), len(masked)))
        if not (tip.any() or pop.any() or bulge.any()):
            break
        table = tr.masked_table(table, masked)
        units, link_ptr, links = tr.graph(table, k, canonical, min_count)
    return units, report, table, rows, bulge_rows


def report_text(report):
    """what --tip-report writes with --unitigs-pop-bulges: six fields"""
    return "".join("%d\t%d\t%d\t%d\t%d\t%d\n" % ((i + 1,) + r) for i, r in enumerate(report)).encode()


def bulge_lines(rows, k):
    """what --bulge-report writes: round, popped name, LN, km, hops, the path's k-mers, the path in GAF segment notation,
    kind, the popped sequence, the path's sequence (spelled from s to t: oriented like the popped one)"""
    out = []
    for rnd, j, path, (seq, kc, n, _), spelled in rows:
        if len(seq) != len(spelled):
            kind = "indel"
        else:
            kind = "snp" if sum(a != b for a, b in zip(seq, spelled)) == 1 else "mnp"
        names = "".join(("<" if w & 1 else ">") + str(w >> 1) for w in path)
        out.append("%d\t%d\t%d\t%s\t%d\t%d\t%s\t%s\t%s\t%s\n" % (rnd, j, len(seq), br._km(kc, n), len(path), len(spelled) - k + 1, names, kind, seq,
                                                                 spelled))
    return "".join(out).encode()
