"""
The exact strata under gate-level faults restated in NumPy / itertools, sharing nothing with the native library:

  sites            the site table of a gate list by a walk over the gates: one location per operand, in gate order
  enumerate_range  itertools.combinations x itertools.product over the kind masks, ranks from math.comb, the outcome words XOR-ed from
                   tests/gadget_enumerate_ref.effect_words (identity fault vectors through the restated gadget), the judgement
                   ec_ref.tally / ft_ref.tally
"""
import itertools
import math

import numpy as np

from tests.gadget_enumerate_ref import rank_of, subset_of_rank

CNOT = 1


def sites(gates):
    """(site_loc, n1, n2, site_gate): the one-operand gates first, then the CNOTs, each in gate order; site_loc is the first location."""
    one, two, loc = [], [], 0
    for g, (kind, _, _) in enumerate(np.asarray(gates).tolist()):
        (two if kind == CNOT else one).append((loc, g))
        loc += 2 if kind == CNOT else 1
    both = one + two
    return [l for l, _ in both], len(one), len(two), [g for _, g in both]


def mask_words(eff, first_locations, nbits):
    """(sites, 2^nbits, ldr): the outcome words of every kind mask (index = mask, 0 unused) at the given first locations."""
    locs = np.asarray(first_locations, dtype=np.int64)
    out = np.zeros((len(locs), 1 << nbits, eff.shape[2]), dtype=np.uint64)
    for mask in range(1, 1 << nbits):
        for bit in range(nbits):
            if (mask >> bit) & 1:
                out[:, mask] ^= eff[locs + (bit >> 1), bit & 1]
    return out


def _part(n, k, first, count, whole):
    """The subsets of ranks [first, first + count) of the k-subsets of [0, n), ascending rank."""
    if whole:
        return sorted(itertools.combinations(range(n), k), key=rank_of)[first:first + count]
    return [subset_of_rank(n, k, r) for r in range(first, first + count)]


def subsets_of_range(n1, n2, a, b, first_rank, count):
    """[(one-operand picks, CNOT picks)] of ranks [first_rank, first_rank + count): rank = r_s + C(n1, a) r_c."""
    c1 = math.comb(n1, a)
    total = c1 * math.comb(n2, b)
    assert 0 <= first_rank and first_rank + count <= total
    if count * 8 > total:                                              # most of the stratum: the product of the two sorted lists
        ones, twos = _part(n1, a, 0, c1, True), _part(n2, b, 0, math.comb(n2, b), True)
        return [(s, c) for c in twos for s in ones][first_rank:first_rank + count]
    return [(subset_of_rank(n1, a, r % c1), subset_of_rank(n2, b, r // c1)) for r in range(first_rank, first_rank + count)]


def enumerate_range(gadget, eff, w, b, first_rank, count):
    """counts[(b + 1)][F] as a NumPy object array of Python ints over the site subsets of ranks [first_rank, first_rank + count) of
    (w, b): every kind assignment from itertools.product, the words of one c judged together."""
    fields = len(gadget.tally(np.zeros((0, gadget.ldr), dtype=np.uint64))[0])
    counts = np.zeros((b + 1, fields), dtype=object)
    counts[...] = 0
    if count == 0:
        return counts
    site_loc, n1, n2, _ = sites(gadget.gates)
    a = w - b
    subsets = subsets_of_range(n1, n2, a, b, first_rank, count)
    assert len(subsets) == count
    for s, c in (subsets[0], subsets[-1]):
        assert all(0 <= v < n1 for v in s) and all(0 <= v < n2 for v in c)
    assert rank_of(subsets[0][0]) + math.comb(n1, a) * rank_of(subsets[0][1]) == first_rank
    assert rank_of(subsets[-1][0]) + math.comb(n1, a) * rank_of(subsets[-1][1]) == first_rank + count - 1
    one = mask_words(eff, site_loc[:n1], 2)
    two = mask_words(eff, site_loc[n1:], 4)
    picks_s = np.array([s for s, _ in subsets], dtype=np.int64).reshape(count, a)
    picks_c = np.array([c for _, c in subsets], dtype=np.int64).reshape(count, b)
    by_c = [[] for _ in range(b + 1)]
    for kinds in itertools.product(*([range(1, 4)] * a + [range(1, 16)] * b)):
        words = np.zeros((count, gadget.ldr), dtype=np.uint64)
        for k in range(a):
            words ^= one[picks_s[:, k], kinds[k]]
        for k in range(b):
            words ^= two[picks_c[:, k], kinds[a + k]]
        by_c[sum(1 for kappa in kinds[a:] if kappa & 3 and kappa >> 2)].append(words)
    for c, parts in enumerate(by_c):
        if parts:
            got, _ = gadget.tally(np.concatenate(parts))
            for f in range(fields):
                counts[c, f] += int(got[f])
    return counts
