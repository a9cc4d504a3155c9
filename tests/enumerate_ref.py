"""
NumPy restatement of the exact strata (DESIGN.md section 5 "Exact strata"), for tests/test_enumerate.py and
tests/test_gpu_enumerate.py.  Written from the definition alone: configurations from itertools.combinations and
itertools.product, ranks from math.comb, outcomes XOR-ed from FaultCircuit.effects, the decode through the table dicts of an
oracle.cpu_ref code.  It shares no code with gf2_circuit_enumerate_host (csrc/gf2_host.cpp) or the kernel.

    rank(S) = sum_k C(s_k, k + 1);  kinds 1 = X, 2 = Z, 3 = Y;  outcome = XOR_k [kind_k & 1] eff[s_k][0] ^ [kind_k & 2] eff[s_k][1]
    words: [key_x: kw(r_2)] [key_z: kw(r_1)] [parity],  kw(r) = 1 for r <= 63 else 2, low word first
"""
import itertools
import math

import numpy as np

FIELDS = ('logical_x', 'logical_z', 'logical_any', 'uncorrectable_x', 'uncorrectable_z')


def rank_of(subset):
    return sum(math.comb(int(s), k + 1) for k, s in enumerate(sorted(subset)))


def unrank(nb, w, rank):
    """Python-integer inverse of rank_of: from the top pick down, the largest s with C(s, k) <= what is left."""
    out, hi = [], nb
    for k in range(w, 0, -1):
        lo = k - 1
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if math.comb(mid, k) <= rank else (lo, mid)
        out.append(lo)
        rank -= math.comb(lo, k)
        hi = lo
    return out[::-1]


def subsets(nb, w, first_rank=0, count=None):
    """The w-subsets of range(nb) with ranks [first_rank, first_rank + count), in rank order."""
    total = math.comb(nb, w)
    count = total - first_rank if count is None else count
    if 4 * count < total:                                                    # a window: by the Python-integer inverse
        return [tuple(unrank(nb, w, r)) for r in range(first_rank, first_rank + count)]
    picked = sorted((rank_of(s), s) for s in itertools.combinations(range(nb), w))
    assert [r for r, _ in picked] == list(range(total))                      # rank is a bijection onto [0, C(nb, w))
    return [s for _, s in picked[first_rank:first_rank + count]]


def tables_of(code):
    """[(table: key -> flip of the correction, key words)] for side 0 (key_x: parity_check_c2, z operator) and side 1."""
    out = []
    for table, op, r in ((code._c2_syndromes, code.z_operator_matrix()[0], code.r_2), (code._c1_syndromes, code.x_operator_matrix()[0], code.r_1)):
        op = np.asarray(op).astype(np.int64) & 1
        out.append(({int(key): int(np.dot(op, np.asarray(corr).astype(np.int64))) & 1 for key, corr in table.items()}, 1 if r <= 63 else 2))
    return out


def counts(code, effects, w, first_rank=0, count=None):
    """(w + 1, w + 1, 5) uint64 counts [n_x][n_y][field] over the subsets of the rank range with all 3^w kind assignments."""
    effects = np.asarray(effects)
    nb, ldr = effects.shape[0], effects.shape[2]
    eff = [[[int(v) for v in effects[l, c]] for c in range(2)] for l in range(nb)]
    (tab_x, kwx), (tab_z, kwz) = tables_of(code)
    assert ldr == kwx + kwz + 1
    out = np.zeros((w + 1, w + 1, 5), dtype=np.uint64)
    for subset in subsets(nb, w, first_rank, count):
        for kinds in itertools.product((1, 2, 3), repeat=w):
            words = [0] * ldr
            for s, kind in zip(subset, kinds):
                for q in range(ldr):
                    words[q] ^= (eff[s][0][q] if kind & 1 else 0) ^ (eff[s][1][q] if kind & 2 else 0)
            key_x = words[0] | (words[1] << 64 if kwx == 2 else 0)
            key_z = words[kwx] | (words[kwx + 1] << 64 if kwz == 2 else 0)
            found_x, found_z = tab_x.get(key_x), tab_z.get(key_z)
            flip_x, flip_z = (words[-1] & 1) ^ (found_x or 0), ((words[-1] >> 1) & 1) ^ (found_z or 0)
            out[kinds.count(1), kinds.count(3)] += np.array([flip_x, flip_z, flip_x | flip_z, found_x is None, found_z is None], dtype=np.uint64)
    return out
