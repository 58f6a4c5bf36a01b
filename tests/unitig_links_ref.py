"""Plain-Python statement of the unitig-link contract (include/cfrk_abi.h, "Unitig links"): strings and dictionaries over
the unitig list of tests/unitig_ref.py, nothing shared with the product.  The facts the contract derives from the
definition are asserted on every input."""
import numpy as np

from . import unitig_ref as ur

FROM_MINUS, TO_MINUS = 1, 2
UNITIG_LINK_DTYPE = np.dtype([("to", "<u4"), ("flags", "<u4")])


def oriented_links(units, table, k, canonical, min_count=1):
    """units as ur.unitigs() returns them, of `table` at `min_count` -> one list per unitig of (o, b, v, ov): the link
    (j,o) -> (v,ov) by appending base b; o, ov are 0 for + and 1 for -.  In the row order of the contract."""
    t = max(1, min_count)
    solid = {x for x, c in table.items() if c >= t}
    oris = (0, 1) if canonical else (0,)
    in_O = (lambda a: min(a, ur.rc(a)) in solid) if canonical else (lambda a: a in solid)
    head = lambda j, o: units[j][0][:k] if o == 0 else ur.rc(units[j][0][-k:])
    tail = lambda j, o: units[j][0][-k:] if o == 0 else ur.rc(units[j][0][:k])
    heads = {}
    for j in range(len(units)):
        assert len(units[j][0]) >= k
        for o in oris:
            heads.setdefault(head(j, o), []).append((j, o))
    for h, who in heads.items():
        # two oriented unitigs begin with the same k-mer only when it is a palindromic single-node unitig
        assert len(who) == 1 or (len(who) == 2 and who[0][0] == who[1][0] and units[who[0][0]][0] == h == ur.rc(h)), h
    rows = []
    for j in range(len(units)):
        row = []
        for o in oris:
            a = tail(j, o)
            out = 0
            for b in ur.BASES:
                z = a[1:] + b
                if not in_O(z):
                    continue
                assert z in heads, (j, o, z)                    # a solid successor of a tail is the head of a unitig
                for v, ov in heads[z]:                          # (+ before -: the order they were entered in)
                    row.append((o, b, v, ov))
                    out += 1
            assert out <= 8
        rows.append(row)
    flat = {(j, o, v, ov) for j, row in enumerate(rows) for o, _, v, ov in row}
    assert len(flat) == sum(len(r) for r in rows)               # no link twice
    if canonical:
        assert all((v, 1 - ov, j, 1 - o) in flat for j, o, v, ov in flat)      # the mirror of every link is a link
    for j, (_, _, _, circ) in enumerate(units):
        if circ:
            assert (j, 0, j, 0) in flat and (not canonical or (j, 1, j, 1) in flat)
    assert len(flat) <= (16 if canonical else 4) * len(units)
    return rows


def links(units, table, k, canonical, min_count=1):
    """-> (link_ptr int64[nS + 1], links UNITIG_LINK_DTYPE[n_links]) in the ABI layout"""
    rows = oriented_links(units, table, k, canonical, min_count)
    link_ptr = np.zeros(len(units) + 1, np.int64)
    flat = []
    for j, row in enumerate(rows):
        flat += [(v, (FROM_MINUS if o else 0) | (TO_MINUS if ov else 0)) for o, _, v, ov in row]
        link_ptr[j + 1] = len(flat)
    return link_ptr, np.array(flat, UNITIG_LINK_DTYPE).reshape(len(flat))


def fasta_text_links(units, link_ptr, links):
    """what --unitigs-out writes with --unitigs-links: ur.fasta_text with the L tags at the end of every header"""
    plain = ur.fasta_text(units).decode().split("\n")
    out = []
    for j in range(len(units)):
        tags = "".join(" L:%s:%d:%s" % ("-" if f & FROM_MINUS else "+", to, "-" if f & TO_MINUS else "+")
                       for to, f in links[link_ptr[j]:link_ptr[j + 1]].tolist())
        out += [plain[2 * j] + tags, plain[2 * j + 1]]
    return "".join(x + "\n" for x in out).encode()


def gfa_text(units, k, link_ptr, links):
    """what --unitigs-gfa writes"""
    out = ["H\tVN:Z:1.0\n"]
    for j, (seq, kc, n, _) in enumerate(units):
        tenths = (kc * 10 + n // 2) // n
        out.append("S\t%d\t%s\tLN:i:%d\tKC:i:%d\tkm:f:%d.%d\n" % (j, seq, len(seq), kc, tenths // 10, tenths % 10))
    for j in range(len(units)):
        for to, f in links[link_ptr[j]:link_ptr[j + 1]].tolist():
            out.append("L\t%d\t%s\t%d\t%s\t%dM\n" % (j, "-" if f & FROM_MINUS else "+", to, "-" if f & TO_MINUS else "+", k - 1))
    return "".join(out).encode()
