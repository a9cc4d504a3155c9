"""
The tally rules of the two post-selected gadgets restated on plain tables (DESIGN.md sections 5b "Error-correction cycle" and 5c
"Logical measurement"), in Python and NumPy, sharing nothing with quantum_css_codes_amd, csrc/gf2_host.cpp or the kernels.  Where
tests/ec_ref.py and tests/ft_ref.py need a code (check matrices, vectors of known errors, the code's own table dicts), these take what
the native entry points take: outcome words, the key widths r_1 and r_2, and two tables of keys with one flip bit each -- so they
also judge synthetic effect tables that belong to no code.

  ec_tally        the eight counts of the cycle's rule, in the order of ec_noise.EC_FIELDS
  ft_tally        the seven counts of the measurement's rule, in the order of ft_noise.FT_FIELDS
  sampled_words   the outcome words of an effect table under the oracle's sampler run over its L locations

A table is a dict key -> flip bit.  Side 0 is key_x (the low half of a word, r_2 bits, table 2), side 1 is key_z (the high half, r_1
bits, table 1).  Each side keeps a record of what its earlier lookups matched: K, the XOR of the matched keys, and P, the XOR of their
flip bits.  A key is looked up relative to K; a hit joins the record, a miss is counted and leaves the record alone.
"""
import numpy as np

from tests import stream_ref

EC_FIELDS = ('accepted', 'logical_x', 'logical_z', 'logical_any', 'uncorrectable_x', 'uncorrectable_z', 'round_unmatched_x',
             'round_unmatched_z')
FT_FIELDS = ('accepted', 'wrong', 'trial_wrong', 'first_trial_wrong', 'split_vote', 'unmatched_x', 'unmatched_z')


def _sides(r1, keys1, flips1, r2, keys2, flips2):
    """[(shift, key mask, table)] of side 0 and side 1."""
    sides = []
    for shift, r, keys, flips in ((0, r2, keys2, flips2), (32, r1, keys1, flips1)):
        keys = [int(k) for k in np.asarray(keys).reshape(-1)]
        flips = [int(f) & 1 for f in np.asarray(flips).reshape(-1)]
        assert len(keys) == len(flips) == len(set(keys))
        sides.append((shift, (1 << int(r)) - 1, dict(zip(keys, flips))))
    return sides


def ec_tally(words, rounds, r1, keys1, flips1, r2, keys2, flips2):
    """The eight counts over outcome words (samples, ldr) laid out as [final frame] [round 1 .. rounds] [flag words]."""
    sides = _sides(r1, keys1, flips1, r2, keys2, flips2)
    counts = [0] * 8
    for row in np.asarray(words, dtype=np.uint64).tolist():
        if any(row[rounds + 1:]):
            continue                                                   # a verification fired: rejected
        counts[0] += 1
        flip = [0, 0]
        for side, (shift, mask, table) in enumerate(sides):
            known, parity = 0, 0
            for t in range(1, rounds + 1):
                key = ((row[t] >> shift) & mask) ^ known
                if key in table:
                    known ^= key
                    parity ^= table[key]
                else:
                    counts[6 + side] += 1
            key = ((row[0] >> shift) & mask) ^ known
            flip[side] = ((row[0] >> (shift + 31)) & 1) ^ parity
            if key in table:
                flip[side] ^= table[key]
            else:
                counts[4 + side] += 1
        counts[1] += flip[0]
        counts[2] += flip[1]
        counts[3] += flip[0] | flip[1]
    return counts


def ft_tally(words, nsteps, measure_mask, r1, keys1, flips1, r2, keys2, flips2):
    """The seven counts over outcome words (samples, ldr) laid out as [step 0 .. nsteps - 1] [flag words]; bit s of measure_mask
    makes step s a MEASURE step."""
    sides = _sides(r1, keys1, flips1, r2, keys2, flips2)
    measures = [s for s in range(nsteps) if (measure_mask >> s) & 1]
    trials = len(measures)
    counts = [0] * 7
    for row in np.asarray(words, dtype=np.uint64).tolist():
        if any(row[nsteps:]):
            continue
        counts[0] += 1
        known, parity = [0, 0], [0, 0]
        wrong = first_wrong = 0
        for s in range(nsteps):
            measure = s in measures
            for side, (shift, mask, table) in enumerate(sides):
                if measure and side == 1:
                    continue                                           # a MEASURE step carries no key_z
                key = ((row[s] >> shift) & mask) ^ known[side]
                if key in table:
                    known[side] ^= key
                    parity[side] ^= table[key]
                else:
                    counts[5 + side] += 1
            if measure:
                bad = ((row[s] >> 31) & 1) ^ parity[0]
                wrong += bad
                if s == measures[0]:
                    first_wrong = bad
        counts[1] += 2 * wrong > trials
        counts[2] += wrong
        counts[3] += first_wrong
        counts[4] += 0 < wrong < trials
    return counts


def sampled_words(eff, seed, first, count, p):
    """(count, ldr) uint64: for every sample of [first, first + count) the XOR of eff[l, 0] over its faults with an X component and of
    eff[l, 1] over those with a Z component (Y has both), the faults being tests/stream_ref.sampled_faults' (the C oracle's sampler
    with n := L)."""
    eff = np.asarray(eff, dtype=np.uint64)
    locations, _, ldr = eff.shape
    fault_first, location, kind = stream_ref.sampled_faults(locations, seed, first, count, p)
    sample = np.repeat(np.arange(count), np.diff(fault_first))
    out = np.zeros((count, ldr), dtype=np.uint64)
    for component in (0, 1):
        has = ((kind >> component) & 1) == 1
        np.bitwise_xor.at(out, sample[has], eff[location[has], component])
    return out
