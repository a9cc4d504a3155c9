"""
The malignant fault sets of the two post-selected gadgets restated in NumPy / itertools (DESIGN.md sections 5b "Malignant fault sets
of the cycle" and 5c "Malignant fault sets of the measurement"), sharing nothing with the native library: the subsets and ranks of
tests/gadget_enumerate_ref.py, every configuration's words XOR-ed from the restated gadget's effect words, the class byte from
ec_ref.tally / ft_ref.tally (quil_classical_correct on vectors of known errors).

  list_range      the (rank, kinds code, class) triples of a rank range, sorted by (rank, kinds code)
  records         the same as the (found, 2) uint64 words of include/gf2hip.h "malignant fault sets"
"""
import itertools

import numpy as np

from tests import gadget_enumerate_ref as ger

KIND_BITS = (1, 3, 2)                                                  # kind 0 X, 1 Y, 2 Z as the sampler's kind bits (1 = X, 2 = Z)


def subsets_of_range(L, w, first_rank, count):
    out = []
    subset = ger.subset_of_rank(L, w, first_rank) if count else ()
    for i in range(count):
        if i:
            subset = ger.successor(subset, w)
        out.append(subset)
    assert not out or [ger.rank_of(s) for s in (out[0], out[-1])] == [first_rank, first_rank + count - 1]
    return out


def list_range(gadget, eff, w, first_rank, count, select):
    """[(rank, kinds code, class byte)] of the accepted configurations of ranks [first_rank, first_rank + count) whose class byte has
    a bit of `select`: kinds code = sum_j kind_j 3^j over the picks in ascending location order."""
    subsets = subsets_of_range(gadget.locations, w, first_rank, count)
    picks = np.array(subsets, dtype=np.int64).reshape(len(subsets), w)
    out = []
    for kinds in itertools.product(range(3), repeat=w):                # kinds[j]: of pick j
        words = np.zeros((len(subsets), gadget.ldr), dtype=np.uint64)
        for j, kind in enumerate(kinds):
            if KIND_BITS[kind] & 1:
                words ^= eff[picks[:, j], 0]
            if KIND_BITS[kind] & 2:
                words ^= eff[picks[:, j], 1]
        _, classes = gadget.tally(words)
        code = sum(kind * 3**j for j, kind in enumerate(kinds))
        for i in np.flatnonzero((classes & 1 != 0) & (classes & select != 0)).tolist():
            out.append((first_rank + i, code, int(classes[i])))
    return sorted(out)


def records(gadget, eff, w, first_rank, count, select):
    triples = list_range(gadget, eff, w, first_rank, count, select)
    out = np.zeros((len(triples), 2), dtype=np.uint64)
    for k, (rank, code, cls) in enumerate(triples):
        out[k] = (rank, code | cls << 32)
    return out
