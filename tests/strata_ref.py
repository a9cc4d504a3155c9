"""
NumPy restatement of the stratified sampler (DESIGN.md section 5 "Strata") and of the table decode that follows it, for
tests/test_strata.py and tests/test_gpu_strata.py.  Written from the definition alone: it shares no code with the HIP kernels,
with gf2_stratum_errors (csrc/gf2_host.cpp) or with the package.

    ks = mix64(seed + G (i + 1)),  d = mix64(ks + M (w + 1))                  the segment slot carries the weight
    k = 0 .. w - 1:  v = mix64(d + G (k + 1)),  j = nb - w + k,  t = ((v >> 32) (j + 1)) >> 32,  position = j if t is taken else t
                     c = v & (2^32 - 1):  X component iff c < t_2,  Z component iff c >= t_1
    t_1 = quantise(k_x / s),  t_2 = quantise((k_x + k_y) / s),  s = k_x + k_y + k_z
"""
import math

import numpy as np

GOLDEN = 0x9E3779B97F4A7C15
STREAM_MULT = 0xD1B54A32D192ED03
FIELDS = ('logical_x', 'logical_z', 'logical_any', 'uncorrectable_x', 'uncorrectable_z')


def mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def quantise(x):
    return min(1 << 32, max(0, int(math.floor(x * 4294967296.0 + 0.5))))


def thresholds(kinds):
    k_x, k_y, k_z = (float(k) for k in kinds)
    s = k_x + k_y + k_z
    return quantise(k_x / s), quantise((k_x + k_y) / s)


def kind_probabilities(kinds):
    """Exact probabilities of X, Y, Z under the quantised thresholds."""
    t_1, t_2 = thresholds(kinds)
    return np.array([t_1, t_2 - t_1, (1 << 32) - t_2], dtype=np.float64) / 4294967296.0


def stratum_draws(seed, first, count, nb, w, kinds=(1, 1, 1), floyd_plus=1):
    """Positions (count, w) int64 and kinds (count, w) uint8 (bit 0: X component, bit 1: Z component) of samples
    [first, first + count).  floyd_plus = 0 is the mutant that draws Floyd's t over j instead of j + 1."""
    t_1, t_2 = thresholds(kinds)
    with np.errstate(over="ignore"):
        i = np.arange(count, dtype=np.uint64) + np.uint64(first)
        ks = mix64(np.uint64(seed) + np.uint64(GOLDEN) * (i + np.uint64(1)))
        d = mix64(ks + np.uint64(STREAM_MULT) * np.uint64(w + 1))
        pos = np.zeros((count, w), dtype=np.int64)
        kind = np.zeros((count, w), dtype=np.uint8)
        for k in range(w):
            v = mix64(d + np.uint64(GOLDEN) * np.uint64(k + 1))
            j = nb - w + k
            t = (((v >> np.uint64(32)) * np.uint64(j + floyd_plus)) >> np.uint64(32)).astype(np.int64)
            taken = (pos[:, :k] == t[:, None]).any(axis=1)
            pos[:, k] = np.where(taken, j, t)
            c = v & np.uint64(0xFFFFFFFF)
            kind[:, k] = (c < np.uint64(t_2)).astype(np.uint8) | ((c >= np.uint64(t_1)).astype(np.uint8) << 1)
    return pos, kind


def stratum_bits(seed, first, count, nb, w, kinds=(1, 1, 1)):
    """Dense (e_x, e_z), count x nb uint8 each."""
    pos, kind = stratum_draws(seed, first, count, nb, w, kinds)
    e_x = np.zeros((count, nb), dtype=np.uint8)
    e_z = np.zeros_like(e_x)
    rows = np.arange(count)
    for k in range(w):
        e_x[rows, pos[:, k]] |= kind[:, k] & 1
        e_z[rows, pos[:, k]] |= kind[:, k] >> 1
    return e_x, e_z


def pack(bits):
    """Rows of 0/1 as packed little-endian uint64 words (bit j of a row = bit j & 63 of word j >> 6)."""
    m, n = bits.shape
    ld = max(1, (n + 63) // 64)
    wide = np.zeros((m, ld * 64), dtype=np.uint8)
    wide[:, :n] = bits
    return np.ascontiguousarray(np.packbits(wide, axis=1, bitorder="little").view("<u8").reshape(m, ld))


def unpack(words, n):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=-1, bitorder="little")[..., :n]


def keys_of(check, errors):
    """vec_to_int(check . e) of every row of `errors` (row 0 of the check = most significant bit) as Python ints."""
    synd = (errors.astype(np.int64) @ (np.asarray(check).T.astype(np.int64) & 1)) & 1
    r = synd.shape[1]
    lo_rows, hi_rows = synd[:, max(0, r - 64):], synd[:, :max(0, r - 64)]
    word = lambda part: (part.astype(np.uint64) << np.arange(part.shape[1] - 1, -1, -1, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
    lo = word(lo_rows).tolist()
    if hi_rows.shape[1] == 0:
        return lo
    return [(h << 64) | l for h, l in zip(word(hi_rows).tolist(), lo)]


def decode_counts(code, e_x, e_z):
    """The five counts of the table decode (css_code.py:649-685 and :640-646) of dense errors: a syndrome found in the code's
    table dict gets its correction, one not found leaves the error and counts as uncorrectable; X errors go through
    parity_check_c2 and the z operator, Z errors through parity_check_c1 and the x operator."""
    flips, misses = [], []
    for err, check, table, op in ((e_x, code.parity_check_c2, code._c2_syndromes, code.z_operator_matrix()[0]),
                                  (e_z, code.parity_check_c1, code._c1_syndromes, code.x_operator_matrix()[0])):
        op = np.asarray(op).astype(np.int64) & 1
        of_entry = {int(key): int(np.dot(op, np.asarray(corr).astype(np.int64))) & 1 for key, corr in table.items()}
        own = (err.astype(np.int64) @ op) & 1
        found = [of_entry.get(key) for key in keys_of(check, err)]
        misses.append(np.array([f is None for f in found]))
        flips.append(own ^ np.array([f or 0 for f in found], dtype=np.int64))
    return np.array([flips[0].sum(), flips[1].sum(), (flips[0] | flips[1]).sum(), misses[0].sum(), misses[1].sum()], dtype=np.uint64)


def strata_counts(code, weights, samples, kinds=(1, 1, 1), seed=0, first=0, chunk=1 << 16):
    """(nstrata, 5) counts of the code-capacity strata by this module alone; samples and first: one number or one per stratum."""
    samples = np.broadcast_to(np.asarray(samples, dtype=np.int64), (len(weights),))
    firsts = np.broadcast_to(np.asarray(first, dtype=np.int64), (len(weights),))
    n = np.asarray(code.parity_check_c1).shape[1]
    out = np.zeros((len(weights), 5), dtype=np.uint64)
    for s, w in enumerate(weights):
        for done in range(0, int(samples[s]), chunk):
            now = min(chunk, int(samples[s]) - done)
            out[s] += decode_counts(code, *stratum_bits(seed, int(firsts[s]) + done, now, n, int(w), kinds))
    return out


def steane_failures(code):
    """(#X, #Y, #Z) of every one of the 4^7 Pauli errors of a 7-qubit code that ends in a logical flip of either kind, as
    test_quantisation_floor_of_the_steane_logical_error_rate enumerates them -- and the same split by side: [any, x, z]."""
    n = 7
    e = np.arange(4 ** n)
    kinds = np.stack([(e >> (2 * j)) & 3 for j in range(n)], axis=1)
    e_x = np.isin(kinds, (1, 2)).astype(np.uint8)
    e_z = np.isin(kinds, (2, 3)).astype(np.uint8)
    flips = []
    for err, check, table, op in ((e_x, code.parity_check_c2, code._c2_syndromes, code.z_operator_matrix()[0]),
                                  (e_z, code.parity_check_c1, code._c1_syndromes, code.x_operator_matrix()[0])):
        op = np.asarray(op).astype(np.int64) & 1
        corr = np.array([np.asarray(table[key]) if key in table else np.zeros(n, dtype=np.int64) for key in keys_of(check, err)])
        flips.append((((err + corr) & 1) @ op) & 1)
    triples = np.stack([(kinds == 1).sum(axis=1), (kinds == 2).sum(axis=1), (kinds == 3).sum(axis=1)], axis=1)
    pick = lambda mask: [tuple(int(v) for v in row) for row in triples[mask.astype(bool)]]
    return pick(flips[0] | flips[1]), pick(flips[0]), pick(flips[1])
