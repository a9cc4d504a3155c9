"""
NumPy restatement of the stratified sampler over gates (DESIGN.md section 5e "Sampled strata under gate-level faults"), for
tests/test_gate_strata.py and tests/test_gpu_gate_strata.py.  Written from the definition alone: it shares no code with the HIP
kernel, with gf2_gate_stratum_outcomes_host (csrc/gf2_host.cpp) or with the package; only mix64 and the two constants come from
tests/strata_ref.py, itself such a restatement.

    ks = mix64(seed + G (i + 1)),  d = mix64(ks + M (64 + 17 b + a + 1))          the segment slot carries the stratum (a, b)
    k = 0 .. a + b - 1:  v = mix64(d + G (k + 1)),  hi = v >> 32,  lo = v & (2^32 - 1)
      k < a:   j = n1 - a + k,        t = (hi (j + 1)) >> 32,  site = j if t is an earlier pick else t,       kappa = 1 + ((lo 3) >> 32)
      k >= a:  j = n2 - b + (k - a),  t = (hi (j + 1)) >> 32,  site = n1 + (j if t is an earlier CNOT pick else t),  kappa = 1 + ((lo 15) >> 32)
    words = XOR over the picks and the set bits t of kappa of eff[site_loc[site] + (t >> 1)][t & 1]
    c     = the number of CNOT picks with (kappa & 3) and (kappa >> 2) both non-zero
"""
import numpy as np

from tests.strata_ref import GOLDEN, STREAM_MULT, mix64

MAX_WEIGHT = 16


def gate_stratum_draws(seed, first, count, n1, n2, a, b, floyd_plus=1):
    """Sites (count, a + b) int64 in the unified numbering (one-operand sites [0, n1), CNOT sites [n1, n1 + n2)) and kind masks
    (count, a + b) uint8 of samples [first, first + count).  floyd_plus = 0 is the mutant that draws Floyd's t over j instead of
    j + 1."""
    with np.errstate(over="ignore"):
        i = np.arange(count, dtype=np.uint64) + np.uint64(first)
        ks = mix64(np.uint64(seed) + np.uint64(GOLDEN) * (i + np.uint64(1)))
        d = mix64(ks + np.uint64(STREAM_MULT) * np.uint64(64 + 17 * b + a + 1))
        site = np.zeros((count, a + b), dtype=np.int64)
        kappa = np.zeros((count, a + b), dtype=np.uint8)
        for k in range(a + b):
            v = mix64(d + np.uint64(GOLDEN) * np.uint64(k + 1))
            hi, lo = v >> np.uint64(32), v & np.uint64(0xFFFFFFFF)
            if k < a:
                base, j, nkinds, earlier = 0, n1 - a + k, 3, site[:, :k]
            else:
                base, j, nkinds, earlier = n1, n2 - b + (k - a), 15, site[:, a:k]
            t = ((hi * np.uint64(j + floyd_plus)) >> np.uint64(32)).astype(np.int64) + base
            taken = (earlier == t[:, None]).any(axis=1)
            site[:, k] = np.where(taken, base + j, t)
            kappa[:, k] = (1 + ((lo * np.uint64(nkinds)) >> np.uint64(32))).astype(np.uint8)
    return site, kappa


def two_operand(kappa, a):
    """c per sample: the CNOT picks (columns a and up) whose mask has both halves non-zero."""
    cnot = kappa[:, a:]
    return (((cnot & 3) != 0) & ((cnot >> 2) != 0)).sum(axis=1).astype(np.uint8)


def gate_stratum_words(eff, site_loc, n1, n2, seed, first, count, a, b):
    """(words (count, ldr) uint64, c (count,) uint8) of those samples over the effect words eff (L, 2, ldr)."""
    site_loc = np.asarray(site_loc, dtype=np.int64)
    site, kappa = gate_stratum_draws(seed, first, count, n1, n2, a, b)
    words = np.zeros((count, eff.shape[2]), dtype=np.uint64)
    for k in range(a + b):
        loc = site_loc[site[:, k]]
        for bit in range(4):
            has = ((kappa[:, k] >> bit) & 1).astype(bool)
            words[has] ^= eff[loc[has] + (bit >> 1), bit & 1]
    return words, two_operand(kappa, a)


def gate_stratum_counts(gadget, eff, site_loc, n1, n2, seed, first, count, a, b, chunk=1 << 16):
    """The (17, F) tally [c][field] of those samples by the restated gadget's rule (gadget.tally)."""
    nfields = len(gadget.tally(np.zeros((0, gadget.ldr), dtype=np.uint64))[0])
    out = np.zeros((MAX_WEIGHT + 1, nfields), dtype=np.uint64)
    for done in range(0, count, chunk):
        words, c = gate_stratum_words(eff, site_loc, n1, n2, seed, first + done, min(chunk, count - done), a, b)
        for value in np.unique(c).tolist():
            out[value] += np.array([int(v) for v in gadget.tally(words[c == value])[0]], dtype=np.uint64)
    return out


def synthetic_sites(n1, n2, rng):
    """A shuffled site table: site_loc (n1 + n2) int32 over L = n1 + 2 n2 locations, the one-operand sites first."""
    order = rng.permutation(n1 + n2)                                          # the order in which the sites take their locations
    width = np.where(order < n1, 1, 2)
    start = np.concatenate(([0], np.cumsum(width)[:-1]))
    site_loc = np.zeros(n1 + n2, dtype=np.int32)
    site_loc[order] = start
    return site_loc
