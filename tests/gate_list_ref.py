"""
The malignant fault sets under gate-level faults restated in NumPy / itertools (DESIGN.md section 5e "Malignant fault sets under
gate-level faults"), sharing nothing with the native library: tests/gate_enumerate_ref.py's walk (sites, subsets_of_range, mask_words),
the judgement ec_ref.tally / ft_ref.tally, whose class byte per configuration is kept here instead of its counts.

  list_range   the records of a rank range: (found, 2) uint64, sorted by (rank, kind masks)
"""
import itertools

import numpy as np

from tests import gate_enumerate_ref as gate_ref


def list_range(gadget, eff, w, b, first_rank, count, select):
    """The records of the accepted configurations with a class bit of `select` over the site subsets of ranks [first_rank,
    first_rank + count) of (w, b): word 0 the rank, word 1 the kind masks (a nibble per pick, the one-operand picks first) and, from
    bit 32, the class byte."""
    if count == 0:
        return np.zeros((0, 2), dtype=np.uint64)
    site_loc, n1, n2, _ = gate_ref.sites(gadget.gates)
    a = w - b
    subsets = gate_ref.subsets_of_range(n1, n2, a, b, first_rank, count)
    assert len(subsets) == count
    one = gate_ref.mask_words(eff, site_loc[:n1], 2)
    two = gate_ref.mask_words(eff, site_loc[n1:], 4)
    picks_s = np.array([s for s, _ in subsets], dtype=np.int64).reshape(count, a)
    picks_c = np.array([c for _, c in subsets], dtype=np.int64).reshape(count, b)
    ranks = np.arange(first_rank, first_rank + count, dtype=np.uint64)
    found = []
    for kinds in itertools.product(*([range(1, 4)] * a + [range(1, 16)] * b)):
        words = np.zeros((count, gadget.ldr), dtype=np.uint64)
        for k in range(a):
            words ^= one[picks_s[:, k], kinds[k]]
        for k in range(b):
            words ^= two[picks_c[:, k], kinds[a + k]]
        _, classes = gadget.tally(words)
        hit = ((classes & 1) != 0) & ((classes & select) != 0)
        masks = sum(kappa << (4 * k) for k, kappa in enumerate(kinds))
        tail = np.uint64(masks) | (classes[hit].astype(np.uint64) << np.uint64(32))
        found.append(np.stack((ranks[hit], tail), axis=1))
    records = np.concatenate(found) if found else np.zeros((0, 2), dtype=np.uint64)
    order = np.lexsort((records[:, 1] & np.uint64(0xFFFF), records[:, 0]))
    return np.ascontiguousarray(records[order])
