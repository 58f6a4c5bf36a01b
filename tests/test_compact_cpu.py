"""CPU: the unitig-level compaction rule (tests/compact_ref.py, include/cfrk_abi.h "Unitig compaction") against the k-mer
rule on the reduced dictionary -- ur.unitigs(tr.masked_table(...)) -- on hand-made cases and on seeded random dictionaries;
the cases the GPU tests share; the ABI, the Python layer and the CLI option as far as they go without a GPU."""
import os
import subprocess

import numpy as np
import pytest

from . import compact_ref as cr
from . import tips_ref as tr
from . import unitig_ref as ur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ("cfrk_global_unitigs_compact", "cfrk_global_unitigs_compact_device")


def _rand(rng, n, letters=4):
    return "".join(ur.BASES[i] for i in rng.integers(0, letters, n))


def graph_case(seqs, k, canonical, drop_if):
    """-> (table, units, link_ptr, links, drop): the graph of the strings, drop[j] = drop_if(j, unit j)"""
    table = ur.count_kmers(seqs, k, canonical)
    units, link_ptr, links = tr.graph(table, k, canonical)
    drop = np.array([1 if drop_if(j, u) else 0 for j, u in enumerate(units)], np.uint8)
    return table, units, link_ptr, links, drop


def k_mer_rule(table, units, drop, k, canonical):
    """what the defining property asks for: the unitigs of the dictionary without the dropped unitigs' k-mers"""
    gone = [x for j in np.flatnonzero(drop) for x in tr.unit_kmers(units[j][0], k, canonical)]
    return ur.unitigs(tr.masked_table(table, gone, canonical), k, canonical)


def holds(case, k, canonical):
    """the reference against the k-mer rule -> (new units, into, stats)"""
    table, units, link_ptr, links, drop = case
    new, into, stats = cr.compact(units, link_ptr, links, drop, k, canonical)
    assert new == k_mer_rule(table, units, drop, k, canonical)
    cr.check_into(units, new, into, drop, k)
    return new, into, stats


# ------------------------------------------------------------------ hand-made cases

def _tips_dropped(k, main):
    """drop what lies on no string of `main`"""
    keep = {x for s in main for i in range(len(s) - k + 1) for x in (s[i:i + k], ur.rc(s[i:i + k]))}
    return lambda j, u: u[0][:k] not in keep


def hand_cases(canonical):
    """-> [(name, k, case)]; every case is checked for what its name says in test_hand_made_cases"""
    out = []
    # a backbone with two tips: dropping them joins three unitigs; seeds searched for a reversed middle member
    k = 5
    for seed in range(200):
        rng = np.random.default_rng(seed)
        g = _rand(rng, 40)
        t1, t2 = g[8:14] + _rand(rng, 5), g[20:26] + _rand(rng, 5)
        case = graph_case([g, t1, t2], k, canonical, _tips_dropped(k, [g]))
        if len(case[1]) < 5 or not case[4].any():
            continue
        _, into, stats = cr.compact(*case[1:], k, canonical)
        live = into[case[4] == 0]
        same = live[live["unitig"] == live["unitig"][0]]
        if stats["merged"] and len(same) >= 3 and (not canonical or 0 < (same["at"] & 1).sum() < len(same)):
            out.append(("a chain of three with a reversed middle member" if canonical else "a chain of three", k, case))
            break
    h = "ACCGTAG"
    out.append(("a hairpin", 5, graph_case([h + ur.rc(h), "TTGCA" + h[:6], h[:5] + "TTC"], 5, canonical, lambda j, u: "TTC" in u[0] or "GAA" in u[0])))
    out.append(("a homopolymer node", 4, graph_case(["CGTAAAAAGTC", "TAAAC"], 4, canonical, lambda j, u: u[0] in ("AAAC", "GTTT"))))
    out.append(("a palindromic node at even k", 4, graph_case(["GGCACGTCATT", "CACGA"], 4, canonical, lambda j, u: u[0] in ("ACGA", "TCGT", "CGA", "TCG"))))
    for seed in range(40):                              # a tip on a cycle: the cycle closes and is cut at its minimum
        rng = np.random.default_rng(100 + seed)
        c = _rand(rng, 9 + seed % 5)
        ring = c + c[:k - 1]
        tip = _rand(rng, 4) + c[3:3 + k - 1]
        case = graph_case([ring, tip], k, canonical, _tips_dropped(k, [ring]))
        # (a ring that repeats a (k - 1)-mer branches by itself and does not close: the reference says which seeds serve)
        if case[4].any() and not any(u[3] for u in case[1]) and cr.compact(*case[1:], k, canonical)[2]["closed"] == 1:
            out.append(("a tip on a cycle %d" % seed, k, case))
    c = "ACGGTCTATG"
    out.append(("an already circular unitig", 5, graph_case([c + c[:4], "TTCTCCTTAGC", "CTCCTA"], 5, canonical, lambda j, u: u[0].endswith("CCTA") or u[0].startswith("TAGG"))))
    g = "ACGGTCAATGCCTAGATTCA"
    out.append(("all dropped", 5, graph_case([g, g[5:10] + "G"], 5, canonical, lambda j, u: True)))
    out.append(("none dropped", 5, graph_case([g, g[5:10] + "G", c + c[:4]], 5, canonical, lambda j, u: False)))
    return out


@pytest.mark.parametrize("canonical", [False, True])
def test_hand_made_cases(canonical):
    names, closed, mirror = [], 0, 0
    for name, k, case in hand_cases(canonical):
        new, into, stats = holds(case, k, canonical)
        names.append(name)
        units, drop = case[1], case[4]
        if name.startswith("a chain of three"):
            assert stats["merged"] >= 1 and len(new) <= len(units) - int(drop.sum()) - 2
        if name == "a hairpin":
            rows = [(j, int(t), int(f)) for j in range(len(units)) for t, f in case[3][case[2][j]:case[2][j + 1]].tolist()]
            assert not canonical or any(t == j and f in (1, 2) for j, t, f in rows)       # (j,+) -> (j,-) or (j,-) -> (j,+)
        if name.startswith("a tip on a cycle"):
            assert stats["closed"] == 1 and any(u[3] for u in new)
            closed, mirror = closed + 1, mirror + stats["closed_mirror"]
        if name == "an already circular unitig":
            assert any(u[3] for u in units) and [u for u in new if u[3]] == [u for u in units if u[3]]
        if name == "all dropped":
            assert new == [] and (into["unitig"] == cr.POS_NONE).all()
        if name == "none dropped":
            assert new == units and into["unitig"].tolist() == list(range(len(units))) and not into["at"].any()
    assert any(n.startswith("a chain of three") for n in names) and closed >= 5
    assert not canonical or 0 < mirror < closed        # the minimum on the ring as first met, and on its mirror


# ------------------------------------------------------------------ seeded random dictionaries

def random_case(seed):
    """-> (k, canonical, case): a genome of at most 60 bases over 2 .. 4 letters, read twice over in pieces, random drops"""
    rng = np.random.default_rng(seed)
    k, canonical, letters = int(rng.integers(2, 8)), bool(rng.integers(2)), int(rng.integers(2, 5))
    g = _rand(rng, int(rng.integers(k + 1, 61)), letters)
    seqs = [g]
    if rng.random() < 0.3:
        seqs.append(g + g[:k - 1])                      # the genome as a circle
    for _ in range(int(rng.integers(0, 4))):
        seqs.append(_rand(rng, int(rng.integers(k, 2 * k + 3)), letters))
    how = rng.random()
    p = 0.0 if how < 0.05 else 1.0 if how < 0.08 else float(rng.choice([0.1, 0.2, 0.4]))
    table = ur.count_kmers(seqs, k, canonical)
    units, link_ptr, links = tr.graph(table, k, canonical)
    drop = (rng.random(len(units)) < p).astype(np.uint8)
    if how >= 0.5:                                      # short unitigs go first, as the rules drop them
        drop &= np.array([u[2] <= k for u in units], np.uint8)
    return k, canonical, (table, units, link_ptr, links, drop)


N_RANDOM = 2000


def pal_adjacent(case, k, canonical, into):
    """a surviving palindromic single node linked to a member of a merged component"""
    _, units, link_ptr, links, drop = case
    if not canonical:
        return False
    members = np.bincount(into["unitig"][drop == 0], minlength=1)
    merged = lambda u: not drop[u] and members[into[u]["unitig"]] >= 2
    for j, u in enumerate(units):
        if drop[j] or u[2] != 1 or u[0] != ur.rc(u[0]):
            continue
        if any(merged(int(t)) for t in links["to"][link_ptr[j]:link_ptr[j + 1]]):
            return True
    return False


def test_random_dictionaries():
    merged = closed = pal = 0
    for seed in range(N_RANDOM):
        k, canonical, case = random_case(seed)
        _, into, stats = holds(case, k, canonical)
        merged += stats["merged"] > 0
        closed += stats["closed"] > 0
        pal += stats["merged"] > 0 and pal_adjacent(case, k, canonical, into)
    # not vacuous, by the reference alone
    assert merged >= 100 and closed >= 20 and pal >= 1, (merged, closed, pal)


# ------------------------------------------------------------------ the layers that need no GPU

def test_abi_declares_the_compaction_calls():
    import cfrk_amd
    assert set(NEW_CALLS) <= set(cfrk_amd.abi_symbols())
    header = open(os.path.join(ROOT, "include", "cfrk_abi.h")).read()
    assert "Unitig compaction" in header and "CFRK_COMPACT_TILE_BYTES 4096" in header
    assert cfrk_amd.CFRK_COMPACT_TILE_BYTES == 4096
    for name in ("compact_unitigs", "compact_unitigs_device"):
        assert hasattr(cfrk_amd.GlobalCounter, name)
    import inspect
    for name in ("clip_tips", "simplify"):
        assert inspect.signature(getattr(cfrk_amd.GlobalCounter, name)).parameters["recompact"].default is False


def test_library_exports_the_compaction_calls():
    import cfrk_amd
    if not os.path.exists(cfrk_amd.library_path()):
        pytest.skip("libcfrk_hip.so is not built")
    L = cfrk_amd.load_library()
    assert all(hasattr(L, s) for s in NEW_CALLS)


def _cli():
    path = os.path.join(ROOT, "cfrk_amd", "cfrk")
    if not os.path.exists(path):
        pytest.skip("the cfrk command is not built")
    return path


def test_cli_refuses_recompact_without_a_rule(tmp_path):
    fa = tmp_path / "in.fa"
    fa.write_text(">r\nACGTACGTAGCTAGCTAGGATC\n")
    r = subprocess.run([_cli(), str(fa), str(tmp_path / "out"), "5", "--global", "--unitigs-out", str(tmp_path / "u.fa"), "--simplify-recompact"],
                       capture_output=True, timeout=60)
    assert r.returncode != 0 and b"--simplify-recompact needs" in r.stderr
    assert not (tmp_path / "out").exists() and not (tmp_path / "u.fa").exists()
