"""
The exact strata of the two post-selected gadgets restated in NumPy / itertools (DESIGN.md sections 5b "Exact strata of the cycle"
and 5c "Exact strata of the measurement"), sharing nothing with the native library:

  effect_words    the outcome words of every single X and Z fault: identity fault vectors run through the restated gadget's
                  outcome_words (forward frame propagation, tests/ec_ref.py), not through gf2_circuit_effects_timed's table
  enumerate       itertools.combinations x itertools.product over the kinds, ranks from math.comb, the judgement ec_ref.tally /
                  ft_ref.tally (quil_classical_correct on vectors of known errors, with the code's own table dicts)
  pairs           the whole weight-2 stratum vectorised: all C(L, 2) x 9 outcome words at once, unique rows classified once
"""
import itertools
import math

import numpy as np

KINDS = (1, 3, 2)                                                      # X, Y, Z as the sampler's kind bits (1 = X, 2 = Z)


def effect_words(gadget):
    """(L, 2, ldr) uint64: the outcome words of an X fault ([l, 0]) and of a Z fault ([l, 1]) at every location of an ec_ref.Cycle or an
    ft_ref.Rewritten."""
    L = gadget.locations
    eye, zero = np.identity(L, dtype=np.uint8), np.zeros((L, L), dtype=np.uint8)
    return np.stack((gadget.outcome_words(eye, zero), gadget.outcome_words(zero, eye)), axis=1)


def rank_of(subset):
    return sum(math.comb(s, k + 1) for k, s in enumerate(subset))


def subset_of_rank(L, w, rank):
    """The inverse of rank_of by a linear scan from the top pick down."""
    out, hi = [], L
    for k in range(w, 0, -1):
        s = k - 1
        while s + 1 < hi and math.comb(s + 1, k) <= rank:
            s += 1
        out.append(s)
        rank -= math.comb(s, k)
        hi = s
    return tuple(reversed(out))


def successor(subset, w):
    subset = list(subset)
    j = 0
    while j < w - 1 and subset[j] + 1 == subset[j + 1]:
        subset[j] = j
        j += 1
    subset[j] += 1
    return tuple(subset)


def enumerate_range(gadget, eff, w, first_rank, count):
    """counts[(w + 1)][(w + 1)][F] as a NumPy object array of Python ints over the subsets of ranks [first_rank, first_rank + count):
    every configuration's words XOR-ed from `eff`, all of them judged by one call of the gadget's tally per composition."""
    fields = len(gadget.tally(np.zeros((0, gadget.ldr), dtype=np.uint64))[0])
    counts = np.zeros((w + 1, w + 1, fields), dtype=object)
    counts[...] = 0
    if count == 0:
        return counts
    L = gadget.locations
    total = math.comb(L, w)
    assert 0 <= first_rank and first_rank + count <= total
    subsets = []
    if count * 8 > total:                                              # most of the stratum: walk it all in colexicographic order
        ordered = sorted(itertools.combinations(range(L), w), key=rank_of) if w else [()]
        subsets = ordered[first_rank:first_rank + count]
    else:
        subset = subset_of_rank(L, w, first_rank)
        for i in range(count):
            if i:
                subset = successor(subset, w)
            subsets.append(subset)
    assert [rank_of(s) for s in (subsets[0], subsets[-1])] == [first_rank, first_rank + count - 1]
    picks = np.array(subsets, dtype=np.int64).reshape(len(subsets), w)
    for kinds in itertools.product(KINDS, repeat=w):
        words = np.zeros((len(subsets), gadget.ldr), dtype=np.uint64)
        for k, kind in enumerate(kinds):
            if kind & 1:
                words ^= eff[picks[:, k], 0]
            if kind & 2:
                words ^= eff[picks[:, k], 1]
        got, _ = gadget.tally(words)
        n_x, n_y = kinds.count(1), kinds.count(3)
        for f in range(fields):
            counts[n_x, n_y, f] += int(got[f])
    return counts


def pairs(gadget, eff, chunk=1 << 20):
    """The whole weight-2 stratum, counts[3][3][F] as Python ints: the C(L, 2) pairs from np.triu_indices (the order does not matter
    for a whole stratum), nine kind assignments each."""
    fields = len(gadget.tally(np.zeros((0, gadget.ldr), dtype=np.uint64))[0])
    counts = np.zeros((3, 3, fields), dtype=object)
    counts[...] = 0
    a, b = np.triu_indices(gadget.locations, k=1)
    single = {1: eff[:, 0], 3: eff[:, 0] ^ eff[:, 1], 2: eff[:, 1]}
    for k_a, k_b in itertools.product(KINDS, repeat=2):
        n_x, n_y = (k_a, k_b).count(1), (k_a, k_b).count(3)
        for at in range(0, len(a), chunk):
            words = single[k_a][a[at:at + chunk]] ^ single[k_b][b[at:at + chunk]]
            words = words[~words[:, _first_flag_word(gadget):].any(axis=1)]          # (a rejected word adds nothing to any field)
            got, _ = gadget.tally(words)
            for f in range(fields):
                counts[n_x, n_y, f] += int(got[f])
    return counts


def _first_flag_word(gadget):
    return gadget.nsteps if hasattr(gadget, "nsteps") else gadget.rounds + 1
