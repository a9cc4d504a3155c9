"""
The sampled strata of the two post-selected gadgets restated in NumPy (DESIGN.md sections 5b "Sampled strata of the cycle" and 5c
"Sampled strata of the measurement"), sharing nothing with the native library: positions and kinds from strata_ref.stratum_draws,
the XOR over gadget_enumerate_ref.effect_words (identity fault vectors through the restated gadget), the judgement ec_ref.tally /
ft_ref.tally.
"""
import numpy as np

from tests import strata_ref


def stratum_words(eff, seed, first, count, w, kinds=(1, 1, 1)):
    """(count, ldr) uint64: the outcome words of stratified samples [first, first + count) of weight w over the L = len(eff) locations
    of the effect words eff (L, 2, ldr)."""
    pos, kind = strata_ref.stratum_draws(seed, first, count, len(eff), w, kinds)
    words = np.zeros((count, eff.shape[2]), dtype=np.uint64)
    for k in range(w):
        has_x, has_z = (kind[:, k] & 1).astype(bool), (kind[:, k] >> 1).astype(bool)
        words[has_x] ^= eff[pos[has_x, k], 0]
        words[has_z] ^= eff[pos[has_z, k], 1]
    return words


def stratum_counts(gadget, eff, seed, first, count, w, kinds=(1, 1, 1), chunk=1 << 16):
    """The gadget's tally (a list of Python ints) of those samples."""
    total = None
    for done in range(0, count, chunk):
        got, _ = gadget.tally(stratum_words(eff, seed, first + done, min(chunk, count - done), w, kinds))
        got = [int(v) for v in got]
        total = got if total is None else [a + b for a, b in zip(total, got)]
    if total is None:
        total = [int(v) for v in gadget.tally(np.zeros((0, gadget.ldr), dtype=np.uint64))[0]]
    return total
