"""The planted inputs and parameter sets that tests/test_weak_cpu.py and tests/test_gpu_weak.py share, with their graphs
computed once by the references."""
import numpy as np

from . import tips_ref as tr
from .test_gpu_bubbles import _bubble_input
from .test_gpu_unitigs import _rand, _table

KS = [5, 12, 21, 31, 33]
# (max_kmers, ratio_q8, iso_max_kmers, iso_mean_q8): the default ratio, topology alone, mere rank, nothing at all, and the
# isolated thresholds on with the connections on and off
PARAMS = lambda k: [(k, 1024, 0, 0), (k, 0, 0, 0), (k, 256, 0, 0), (0, 1024, 0, 0), (k, 1024, 2 * k, 512), (0, 0, k + 3, 1 << 16)]

_INPUTS = {}


def weak_input(k):
    """[(string, times counted)]: the bubble input (a random genome counted 4 times with its tips, SNP arms, indels, a
    circle and a hairpin; at k = 5 the genome has 170 bases and repeats, which is what that point is for) and, planted on
    the same genome: chimeric reads that join two distant places by k - 1 junction k-mers, counted once (a connection at
    ratio 4), twice (at ratio 2 only) and 4 times (rank alone decides); two chimeras that leave the same k-mer; a chimera
    of 2k - 1 junction k-mers (longer than k); floating pieces of 4 k-mers counted once and twice, of k + 3 and of 2k + 1
    k-mers counted once"""
    if k in _INPUTS:
        return _INPUTS[k]
    seqs = list(_bubble_input(k, False))                            # (from k = 5 on one input serves both strand rules)
    G = seqs[0][0]
    L = len(G)
    rng = np.random.default_rng(11000 + 100 * k)
    third = max(1, (L - 2 * k) // 3)
    at = lambda i: k + (i * 37) % third                             # a place in the first third; + third, + 2 third: elsewhere
    join = lambda a, b: G[a - k + 1:a + 1] + G[b:b + k - 1]          # the k-mer ending at a, k - 1 junction k-mers, the k-mer from b
    for i, times in enumerate((1, 2, 4)):
        seqs.append((join(at(i), at(i) + third + i), times))
    a = at(5)                                                       # two chimeras out of one place
    seqs.append((join(a, a + third), 1))
    seqs.append((join(a, a + 2 * third), 2))
    a = at(7)                                                       # k random bases in the joint: 2k - 1 junction k-mers
    seqs.append((G[a - k + 1:a + 1] + _rand(rng, k) + G[a + third:a + third + k - 1], 1))
    seqs.append((_rand(rng, k + 3), 1))                             # floating pieces
    seqs.append((_rand(rng, k + 3), 2))
    seqs.append((_rand(rng, 2 * k + 2), 1))
    seqs.append((_rand(rng, 3 * k), 1))
    _INPUTS[k] = seqs
    return seqs


_REF = {}


def ref(k, canonical):
    """(table, units, link_ptr, links) of the planted input, computed once"""
    key = (k, canonical)
    if key not in _REF:
        table = _table(weak_input(k), k, canonical)
        _REF[key] = (table,) + tr.graph(table, k, canonical, 1)
    return _REF[key]
