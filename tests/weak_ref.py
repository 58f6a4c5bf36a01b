"""Plain-Python statement of the weak rule and the simplify loop with it (include/cfrk_abi.h, "Weak unitigs"): sets and
Python integers over the unitig list of tests/unitig_ref.py and the link rows of tests/unitig_links_ref.py, nothing shared
with the product.  The four properties the header states are functions here, asserted on every real graph the reference
is asked about."""
import numpy as np

from . import bubbles_ref as br
from . import bulges_ref as gr
from . import tips_ref as tr
from . import unitig_links_ref as lr
from . import unitig_ref as ur

CONNECTION, ISOLATED = 1, 2
NAMES = {CONNECTION: "connection", ISOLATED: "isolated"}


def _ends(out, nS, canonical):
    """the rows as the header reads them -> (outs, ins): {oriented unitig: [oriented unitig, ...]}.  in() of a canonical job
    is read off the rows by the mirror convention, otherwise it is every link of every row that names the unitig"""
    ins = {}
    if canonical:
        for (u, o), row in out.items():
            ins[(u, 1 - o)] = [(v, 1 - ov) for v, ov in row]
    else:
        for a, row in out.items():
            for b in row:
                ins.setdefault(b, []).append(a)
    return out, ins


def above(n, kc, w, j):
    """w ranks above j"""
    a, b = kc[w] * n[j], kc[j] * n[w]
    return a > b or (a == b and w < j)


def beats(n, kc, w, j, ratio_q8):
    return 256 * kc[w] * n[j] >= ratio_q8 * kc[j] * n[w] and above(n, kc, w, j)


def _decide(n, kc, circ, out, canonical, max_kmers, ratio_q8, iso_max_kmers, iso_mean_q8):
    """-> (candidate[j], weak[j]) of the rows `out` ({oriented unitig: [targets in row order]})"""
    nS = len(n)
    outs, ins = _ends(out, nS, canonical)
    cand, weak = [False] * nS, [0] * nS
    for j in range(nS):
        right, left = outs.get((j, 0), ()), ins.get((j, 0), ())
        if circ[j]:
            continue
        if not left and not right:
            if n[j] <= iso_max_kmers and 256 * kc[j] < iso_mean_q8 * n[j]:
                weak[j] = ISOLATED
            continue
        row = list(outs.get((j, 0), ())) + list(outs.get((j, 1), ()))       # the whole of row j
        self_free = all(v != j for v, _ in row) and all(u != j for u, _ in left)
        if n[j] > max_kmers or not left or not right or not self_free:
            continue
        cand[j] = True
        ok = True
        for v in right:                                 # (j,+) -> v: the other sources of in(v)
            ok = ok and any(w != j and beats(n, kc, w, j, ratio_q8) for w, _ in ins.get(v, ()))
        for u in left:                                  # u -> (j,+): the other targets of out(u)
            ok = ok and any(w != j and beats(n, kc, w, j, ratio_q8) for w, _ in outs.get(u, ()))
        if ok:
            weak[j] = CONNECTION
    return cand, weak


def _check_args(max_kmers, ratio_q8, iso_max_kmers, iso_mean_q8):
    assert 0 <= ratio_q8 <= tr.RATIO_Q8_MAX and 0 <= max_kmers < 1 << 32 and 0 <= iso_max_kmers < 1 << 32 and 0 <= iso_mean_q8 < 1 << 32


def _result(cand, weak):
    nS = len(weak)
    stats = {"connections": weak.count(CONNECTION), "isolated": weak.count(ISOLATED), "candidates": sum(cand)}
    return np.array(weak, np.uint8).reshape(nS), stats


def weak_rows(rec, link_ptr, links, canonical, max_kmers, ratio_q8=1024, iso_max_kmers=0, iso_mean_q8=0):
    """the rule on records (kc, n_kmers, flags) and rows as given, real link set or not -> (weak, stats).  Only what makes
    the statement well defined is asked of the rows."""
    _check_args(max_kmers, ratio_q8, iso_max_kmers, iso_mean_q8)
    nS = len(rec)
    n, kc, circ = [int(x) for x in rec["n_kmers"]], [int(x) for x in rec["kc"]], [bool(x & 1) for x in rec["flags"]]
    assert len(link_ptr) == nS + 1 and link_ptr[0] == 0 and link_ptr[nS] == len(links) and (links["to"] < nS).all()
    out = gr._out_rows(link_ptr, links, nS, canonical)
    return _result(*_decide(n, kc, circ, out, canonical, max_kmers, ratio_q8, iso_max_kmers, iso_mean_q8))


# ---------------------------------------------------------------------------- the header's four properties

def holds_order_free(n, kc, circ, out, canonical, params, cand, weak):
    """every decision reads the input graph only: the rows in another order, and in a canonical job every unitig replaced
    by its mirror image, decide the same"""
    shuffled = {a: list(reversed(row)) for a, row in reversed(list(out.items()))}
    if _decide(n, kc, circ, shuffled, canonical, *params) != (cand, weak):
        return False
    if canonical:
        flipped = {(u, 1 - o): [(v, 1 - ov) for v, ov in row] for (u, o), row in out.items()}
        return _decide(n, kc, circ, flipped, canonical, *params) == (cand, weak)
    return True


def holds_best_neighbour_stays(n, kc, L, weak):
    """the best-ranked neighbour at any oriented end is no weak connection: an end that had a link keeps one"""
    out_, in_ = {}, {}
    for a, b in L:
        out_.setdefault(a, set()).add(b)
        in_.setdefault(b, set()).add(a)
    for side in (out_, in_):
        for a, others in side.items():
            ws = sorted({w for w, _ in others})
            top = ws[0]
            for w in ws:
                if above(n, kc, w, top):
                    top = w
            if weak[top] == CONNECTION:
                return False
    return True


def holds_disjoint_from_tips(n, kc, circ, L, weak):
    """a tip has exactly one dead end, a connection none, an isolated unitig two: no candidate of the tip rule, whatever its
    parameters, is weak"""
    cand, _ = tr._decide(n, kc, circ, L, 1 << 32, 0)
    return not any(w and c for w, c in zip(weak, cand))


def holds_contains_bubbles(n, kc, circ, L, canonical, max_kmers, ratio_q8, weak):
    """at equal max_kmers and ratio_q8 every unitig the bubble rule pops, whatever its max_diff, is a weak connection"""
    for max_diff in (0, 1, 1 << 32):
        pop = br._decide(n, kc, circ, L, canonical, max_kmers, max_diff, ratio_q8)[1]
        if any(p and w != CONNECTION for p, w in zip(pop, weak)):
            return False
    return True


def weak(units, link_ptr, links, canonical, max_kmers, ratio_q8=1024, iso_max_kmers=0, iso_mean_q8=0):
    """units as ur.unitigs() returns them, the rows as lr.links() does -> (weak np.uint8[nS], stats), the header's
    properties asserted"""
    params = (max_kmers, ratio_q8, iso_max_kmers, iso_mean_q8)
    _check_args(*params)
    nS = len(units)
    n, kc, circ = [u[2] for u in units], [u[1] for u in units], [bool(u[3]) for u in units]
    L = tr._oriented(link_ptr, links, nS, canonical)            # (asserts that these are real rows, mirrors and all)
    out = gr._out_rows(link_ptr, links, nS, canonical)
    assert {(a, b) for a, row in out.items() for b in row} == L and sum(len(r) for r in out.values()) == len(L)
    cand, wk = _decide(n, kc, circ, out, canonical, *params)
    # in() read off the rows is in() of the link set
    ins = _ends(out, nS, canonical)[1]
    assert {(a, b) for b, row in ins.items() for a in row} == L
    assert all(c or w != CONNECTION for c, w in zip(cand, wk))
    assert holds_order_free(n, kc, circ, out, canonical, params, cand, wk)
    assert holds_best_neighbour_stays(n, kc, L, wk)
    assert holds_disjoint_from_tips(n, kc, circ, L, wk)
    assert holds_contains_bubbles(n, kc, circ, L, canonical, max_kmers, ratio_q8, wk)
    if max_kmers == 0:
        assert CONNECTION not in wk
    if iso_max_kmers == 0 or iso_mean_q8 == 0:
        assert ISOLATED not in wk
    return _result(cand, wk)


def candidates(units, link_ptr, links, canonical, max_kmers):
    n, kc, circ = [u[2] for u in units], [u[1] for u in units], [bool(u[3]) for u in units]
    out = gr._out_rows(link_ptr, links, len(units), canonical)
    return _decide(n, kc, circ, out, canonical, max_kmers, 0, 0, 0)[0]


# ---------------------------------------------------------------------------- the loop

def simplify(table, k, canonical, min_count=1, tips=True, bubbles_=True, bulges_=False, weak_=True, rounds=4, tip_max_kmers=None,
             tip_ratio_q8=512, bubble_max_kmers=None, bubble_max_diff=0, bubble_ratio_q8=0, bulge_max_kmers=None, bulge_max_diff=0,
             bulge_max_hops=None, bulge_max_visits=1024, bulge_ratio_q8=0, weak_max_kmers=None, weak_ratio_q8=1024,
             weak_iso_max_kmers=None, weak_iso_mean_q8=512):
    """the loop of bulges_ref.simplify with the weak rule beside the three others: unitigs -> links -> each enabled rule on
    that same graph -> drop the k-mers of tip | pop | bulge | (weak != 0), until a round in which no enabled rule finds
    anything or `rounds` rounds are done -> (units of the simplified graph, [(unitigs, tips, bubbles, bulges, masked keys so
    far, connections, isolated)], the reduced dictionary, the bubble rows of bubbles_ref, the bulge rows of bulges_ref,
    [(round, j, kind, unit)] of the weak rule)"""
    tip_max_kmers = k if tip_max_kmers is None else tip_max_kmers
    bubble_max_kmers = k if bubble_max_kmers is None else bubble_max_kmers
    bulge_max_kmers = k if bulge_max_kmers is None else bulge_max_kmers
    weak_max_kmers = k if weak_max_kmers is None else weak_max_kmers
    weak_iso_max_kmers = 2 * k if weak_iso_max_kmers is None else weak_iso_max_kmers
    report, rows, bulge_rows, weak_rows_, masked = [], [], [], [], set()
    units, link_ptr, links = tr.graph(table, k, canonical, min_count)
    for rnd in range(1, rounds + 1):
        nS = len(units)
        tip = tr.tips(units, link_ptr, links, canonical, tip_max_kmers, tip_ratio_q8) if tips else np.zeros(nS, np.uint8)
        if bubbles_:
            pop, partner = br.bubbles(units, link_ptr, links, canonical, bubble_max_kmers, bubble_max_diff, bubble_ratio_q8)
        else:
            pop, partner = np.zeros(nS, np.uint8), np.full(nS, br.NONE, np.uint32)
        if bulges_:
            bulge, _, path_ptr, path, _ = gr.bulges(units, link_ptr, links, canonical, bulge_max_kmers, bulge_max_diff, bulge_max_hops,
                                                    bulge_max_visits, bulge_ratio_q8)
        else:
            bulge, path_ptr, path = np.zeros(nS, np.uint8), np.zeros(nS + 1, np.int64), np.zeros(0, np.uint32)
        if weak_:
            wk, stats = weak(units, link_ptr, links, canonical, weak_max_kmers, weak_ratio_q8, weak_iso_max_kmers, weak_iso_mean_q8)
        else:
            wk, stats = np.zeros(nS, np.uint8), {"connections": 0, "isolated": 0}
        assert not (tip & (pop | bulge | (wk != 0))).any()
        drop = tip | pop | bulge | (wk != 0).astype(np.uint8)
        for j in np.flatnonzero(drop):
            new = tr.unit_kmers(units[j][0], k, canonical)
            assert all(x in table and x not in masked for x in new)
            masked.update(new)
        for j in np.flatnonzero(pop).tolist():
            rows.append((rnd, j, int(partner[j]), units[j], units[int(partner[j]) >> 1]))
        for j in np.flatnonzero(bulge).tolist():
            p = path[path_ptr[j]:path_ptr[j + 1]].tolist()
            bulge_rows.append((rnd, j, p, units[j], gr.spell(units, p, k)))
        for j in np.flatnonzero(wk).tolist():
            weak_rows_.append((rnd, j, int(wk[j]), units[j]))
        report.append((nS, int(tip.sum()), int(pop.sum()), int(bulge.sum()), len(masked), stats["connections"], stats["isolated"]))
        if not drop.any():
            break
        table = tr.masked_table(table, masked)
        units, link_ptr, links = tr.graph(table, k, canonical, min_count)
    return units, report, table, rows, bulge_rows, weak_rows_


def report_rows(report, bubbles_=True, bulges_=False, weak_=True):
    """the loop's report in the shape GlobalCounter.simplify() and --tip-report give it: the bubble count only with the
    bubble rule (the CLI; simplify() always has it), the bulge count only with the bulge rule, the two weak counts at the end
    only with the weak rule"""
    out = []
    for nS, tips, pop, bulge, masked, conn, iso in report:
        out.append((nS, tips) + ((pop,) if bubbles_ else ()) + ((bulge,) if bulges_ else ()) + (masked,) + ((conn, iso) if weak_ else ()))
    return out


def report_text(report, bubbles_=True, bulges_=False, weak_=True):
    """what --tip-report writes: --unitigs-pop-bulges implies the bubble field"""
    rows = report_rows(report, bubbles_ or bulges_, bulges_, weak_)
    return "".join("\t".join(str(x) for x in (i + 1,) + r) + "\n" for i, r in enumerate(rows)).encode()


def weak_lines(rows):
    """what --weak-report writes: round, name, connection / isolated, LN, KC, km, the sequence"""
    return "".join("%d\t%d\t%s\t%d\t%d\t%s\t%s\n" % (rnd, j, NAMES[kind], len(seq), kc, br._km(kc, n), seq)
                   for rnd, j, kind, (seq, kc, n, _) in rows).encode()
