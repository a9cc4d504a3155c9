"""
The tally rules of the two post-selected gadgets and of the streamed routes restated on plain tables (DESIGN.md sections 5b
"Error-correction cycle", 5c "Logical measurement" and 5d), in Python and NumPy, sharing nothing with quantum_css_codes_amd,
csrc/gf2_host.cpp or the kernels.  Where tests/ec_ref.py and tests/ft_ref.py need a code (check matrices, vectors of known errors,
the code's own table dicts), these take what the native entry points take: outcome words, the key widths r_1 and r_2, and two tables
of keys with one flip bit each -- so they also judge synthetic effect tables that belong to no code.

  ec_tally        the eight counts of the cycle's rule, in the order of ec_noise.EC_FIELDS
  ft_tally        the seven counts of the measurement's rule, in the order of ft_noise.FT_FIELDS
  stream_tally    the twelve counts of the streamed rule (DESIGN.md section 5d "Streamed gadgets") over stream-layout words, the steps'
                  kinds read from the block kinds -- what gf2_stream_tally_host states, and with the exhausted samples and the attempts
                  the tally of the four retried routes
  mstream_tally   the twenty counts of the multi-block rule (section 5d "Multi-block programs"), one record per side and frame kept as a
                  (K, P) pair, under both settings of `records`
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


STREAM_FIELDS = ('accepted', 'logical_x', 'logical_z', 'logical_any', 'uncorrectable_x', 'uncorrectable_z', 'unmatched_x', 'unmatched_z',
                 'wrong', 'trial_wrong', 'first_trial_wrong', 'split_vote')
NONE, EC, MEASURE, FINAL, CNOT = 0, 1, 2, 3, 4                         # block kinds of the streamed routes


def _lookup(side, word, record, counts, miss_field):
    """One lookup of a step word's key on `side` relative to the record [K, P]: a hit joins the record, a miss is counted."""
    shift, mask, table = side
    key = ((word >> shift) & mask) ^ record[0]
    if key in table:
        record[0] ^= key
        record[1] ^= table[key]
    else:
        counts[miss_field] += 1


def stream_tally(words, kinds, flag_words, r1, keys1, flips1, r2, keys2, flips2):
    """The twelve counts of the streamed rule (STREAM_FIELDS) over words (samples, ldw) laid out as [steps] [flag words]; kinds: the
    block kinds, a NONE block has no step.  An EC step looks up both sides, a MEASURE step side 0 only and reads its trial against the
    updated record, the FINAL step judges its word against the records without joining them."""
    sides = _sides(r1, keys1, flips1, r2, keys2, flips2)
    steps = [int(k) for k in kinds if int(k) != NONE]
    nsteps, trials = len(steps), sum(k == MEASURE for k in steps)
    counts = [0] * 12
    for row in np.asarray(words, dtype=np.uint64).tolist():
        if any(row[nsteps:nsteps + flag_words]):
            continue
        counts[0] += 1
        records = [[0, 0], [0, 0]]
        outcomes = []
        for s, kind in enumerate(steps):
            if kind == FINAL:
                flip = [0, 0]
                for side, (shift, mask, table) in enumerate(sides):
                    key = ((row[s] >> shift) & mask) ^ records[side][0]
                    flip[side] = ((row[s] >> (shift + 31)) & 1) ^ records[side][1]
                    if key in table:
                        flip[side] ^= table[key]
                    else:
                        counts[4 + side] += 1
                counts[1] += flip[0]
                counts[2] += flip[1]
                counts[3] += flip[0] | flip[1]
                continue
            _lookup(sides[0], row[s], records[0], counts, 6)
            if kind == EC:
                _lookup(sides[1], row[s], records[1], counts, 7)
            else:
                outcomes.append(((row[s] >> 31) & 1) ^ records[0][1])
        wrong = sum(outcomes)
        counts[8] += 2 * wrong > trials
        counts[9] += wrong
        counts[10] += outcomes[0] if outcomes else 0
        counts[11] += 0 < wrong < trials
    return counts


def mstream_tally(words, kinds, frame_a, frame_b, nframes, flag_words, records, r1, keys1, flips1, r2, keys2, flips2):
    """The twenty counts of the multi-block rule over words (samples, ldw) laid out as [the EC and MEASURE steps] [flag words]: accepted,
    wrong_any, unmatched_x, unmatched_z, then wrong, trial_wrong, first_trial_wrong, split_vote of up to four measurements in program
    order.  One record [K, P] per side and per frame; with records = 1 (propagated) a CNOT block a -> b adds side 0's record of a to
    b's and side 1's record of b to a's, with records = 0 it leaves them alone."""
    sides = _sides(r1, keys1, flips1, r2, keys2, flips2)
    blocks = [(int(k), int(a), int(b)) for k, a, b in zip(kinds, frame_a, frame_b)]
    nsteps = sum(k in (EC, MEASURE) for k, _, _ in blocks)
    measured = []                                                      # the frames in the order they are measured
    for kind, a, _ in blocks:
        if kind == MEASURE and a not in measured:
            measured.append(a)
    trials = sum(k == MEASURE for k, _, _ in blocks) // len(measured)
    counts = [0] * 20
    for row in np.asarray(words, dtype=np.uint64).tolist():
        if any(row[nsteps:nsteps + flag_words]):
            continue
        counts[0] += 1
        record = [[[0, 0], [0, 0]] for _ in range(nframes)]           # [frame][side] -> [K, P]
        outcomes = {frame: [] for frame in measured}
        s = 0
        for kind, a, b in blocks:
            if kind == CNOT:
                if records:
                    record[b][0] = [record[b][0][0] ^ record[a][0][0], record[b][0][1] ^ record[a][0][1]]
                    record[a][1] = [record[a][1][0] ^ record[b][1][0], record[a][1][1] ^ record[b][1][1]]
                continue
            if kind == NONE:
                continue
            _lookup(sides[0], row[s], record[a][0], counts, 2)
            if kind == EC:
                _lookup(sides[1], row[s], record[a][1], counts, 3)
            else:
                outcomes[a].append(((row[s] >> 31) & 1) ^ record[a][0][1])
            s += 1
        any_wrong = 0
        for m, frame in enumerate(measured):
            wrong = sum(outcomes[frame])
            any_wrong |= 2 * wrong > trials
            counts[4 + 4 * m] += 2 * wrong > trials
            counts[5 + 4 * m] += wrong
            counts[6 + 4 * m] += outcomes[frame][0]
            counts[7 + 4 * m] += 0 < wrong < trials
        counts[1] += any_wrong
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
