"""
The fault-tolerant logical measurement restated in NumPy (DESIGN.md section 5c "Logical measurement"), sharing nothing with
quantum_css_codes_amd/ft_noise.py or the native library, and nothing with tests/ec_ref.py but its primitives (the encoders, forward
frame propagation, word packing):

  program         the gate list and the measurements of what ftqc.rewrite_program emits for `ops; MEASURE` on one logical qubit,
                  written from the reference's line numbers (ftqc.py:76-95; css_code.py:314-366, 386-409, 436-533, 542-646)
  layout          those measurements as timed outcome rows in the outcome-word layout
  Rewritten       gates, rows and the outcome words of fault vectors
  tally           the classical side of the rewritten program on VECTORS of known errors: quil_classical_correct
                  (css_code.py:649-685) with the code's own table dicts after every measured word, the outcome of every trial from
                  the corrected word (:642-646), the majority vote (:582); unique outcome rows are classified once
"""
import numpy as np

from oracle import cpu_ref
from tests.ec_ref import CNOT, H, IDLE, RESET, encoder, num_locations, pack_words, propagate_rows

UNUSED, STEP, FLAG = 0, 2, 3
FIELDS = ('accepted', 'wrong', 'trial_wrong', 'first_trial_wrong', 'split_vote', 'unmatched_x', 'unmatched_z')
EC, MEASURE = 'ec', 'measure'


def pauli_qubits(code, op):
    """css_code.py:386-407: apply_gate's physical Paulis are the factors of x_operators()[0] / z_operators()[0] / y_operators()[0], in
    the order of the term: qubits ascending for X and Z (pauli_term_for_row, :787-807); Y is the product of the two (:163-172), which
    keeps the X operator's qubits in place (Y where the Z operator acts too) and appends the qubits of the Z operator alone."""
    if op == 'I':
        return []
    x_row = code.x_operator_matrix()[0] if op in 'XY' else np.zeros(code.n, dtype=int)
    z_row = code.z_operator_matrix()[0] if op in 'ZY' else np.zeros(code.n, dtype=int)
    first = [q for q in range(code.n) if x_row[q] == 1]
    return first + [q for q in range(code.n) if z_row[q] == 1 and x_row[q] == 0]


def program(code, ops):
    """(gates, measurements, steps): gates (g, 3) int32; a measurement is (time, kind, step, part, qubits, matrix): the Z-basis readout
    of `qubits` just before gate `time`, multiplied by `matrix`; part is 'x', 'z' (the two keys of an EC step), 'm' (a trial's key
    and raw parity) or None (a flag); steps is the list of EC / MEASURE in program order."""
    n = code.n
    data, a_1, a_2 = list(range(0, n)), list(range(n, 2 * n)), list(range(2 * n, 3 * n))
    h_1, h_2 = np.asarray(code.parity_check_c1), np.asarray(code.parity_check_c2)
    gates, measurements, steps = [], [], []

    def reset(block):                                                  # qecc.py:35-49
        gates.extend((RESET, q, 0) for q in block)

    def measure(block, matrix, kind, step, part):
        gates.extend((IDLE, q, 0) for q in block)
        measurements.append((len(gates), kind, step, part, list(block), np.asarray(matrix) & 1))

    def error_detect_x(block, ancilla, step, include_operators):       # css_code.py:472-501
        reset(ancilla)
        gates.extend(encoder(code, 'zero' if include_operators else 'plus', ancilla))
        gates.extend((CNOT, block[i], ancilla[i]) for i in range(n))
        check = np.concatenate([h_2, code.z_operator_matrix()], axis=0) if include_operators else h_2
        measure(ancilla, check, FLAG, step, None)

    def error_detect_z(block, ancilla, step, include_operators):       # css_code.py:503-533
        reset(ancilla)
        gates.extend(encoder(code, 'plus' if include_operators else 'zero', ancilla))
        gates.extend((CNOT, ancilla[i], block[i]) for i in range(n))
        gates.extend((H, ancilla[i], 0) for i in range(n))
        check = np.concatenate([h_1, code.x_operator_matrix()], axis=0) if include_operators else h_1
        measure(ancilla, check, FLAG, step, None)

    def encode(block, ancilla, state, step):                           # css_code.py:314-366, the loop body once
        reset(block)
        gates.extend(encoder(code, state, block))
        error_detect_x(block, ancilla, step, include_operators=(state == 'zero'))
        error_detect_z(block, ancilla, step, include_operators=(state == 'plus'))

    def error_correct():                                               # css_code.py:436-470 on the data block
        step = len(steps)
        steps.append(EC)
        encode(a_1, a_2, 'plus', step)                                 # :458
        gates.extend((CNOT, data[i], a_1[i]) for i in range(n))        # :459
        measure(a_1, h_2, STEP, step, 'x')                             # :460-462
        encode(a_1, a_2, 'zero', step)                                 # :465
        gates.extend((CNOT, a_1[i], data[i]) for i in range(n))        # :466
        gates.extend((H, a_1[i], 0) for i in range(n))                 # :467
        measure(a_1, h_1, STEP, step, 'z')                             # :468-470

    encode(data, a_1, 'zero', -1)                                      # ftqc.py:77-78: ancilla_1 verifies the logical qubit
    for op in ops:                                                     # ftqc.py:80-86
        if op not in ('I', 'X', 'Y', 'Z'):
            raise ValueError("not a logical Pauli: %r" % (op,))
        gates.extend((IDLE, data[q], 0) for q in pauli_qubits(code, op))   # css_code.py:386-409: a Pauli acts trivially on the frame
        error_correct()                                                # ftqc.py:86
    for _ in range(2 * code.t + 1):                                    # ftqc.py:87-95, css_code.py:570, :576-579
        step = len(steps)
        steps.append(MEASURE)
        encode(a_1, a_2, 'zero', step)                                 # css_code.py:623
        gates.extend((CNOT, data[i], a_1[i]) for i in range(n))        # :634
        measure(a_1, np.concatenate([h_2, code.z_operator_matrix()[0:1]], axis=0), STEP, step, 'm')   # :635, :638, :642
        error_correct()                                                # ftqc.py:95, after every yield (css_code.py:579)
    return np.array(gates, dtype=np.int32).reshape(-1, 3), measurements, steps


def layout(code, gates, measurements, steps):
    """The outcome rows: (rows_x, rows_z, row_time, row_kind, ldr), row r = bit r & 63 of word r >> 6.  Everything is read in the Z
    basis (the H gates before an X-basis readout are in the gate list), so rows_z stays zero."""
    n, r_1, r_2 = code.n, code.r_1, code.r_2
    nsteps = len(steps)
    flags = sum(len(m[5]) for m in measurements if m[1] == FLAG)
    ldr = nsteps + max(1, (flags + 63) // 64)
    rows_x = np.zeros((64 * ldr, 3 * n), dtype=np.uint8)
    rows_z = np.zeros_like(rows_x)
    row_time = np.full(64 * ldr, len(gates), dtype=np.int64)
    row_kind = np.zeros(64 * ldr, dtype=np.int8)
    flag = 0
    for time, kind, step, part, qubits, matrix in measurements:
        if part == 'x':
            bits = [64 * step + r_2 - 1 - i for i in range(r_2)]
        elif part == 'z':
            bits = [64 * step + 32 + r_1 - 1 - i for i in range(r_1)]
        elif part == 'm':
            bits = [64 * step + r_2 - 1 - i for i in range(r_2)] + [64 * step + 31]
        else:
            bits = list(range(64 * nsteps + flag, 64 * nsteps + flag + len(matrix)))
            flag += len(matrix)
        for bit, row in zip(bits, matrix):
            rows_x[bit, qubits] = row
            row_time[bit], row_kind[bit] = time, kind
    return rows_x, rows_z, row_time, row_kind, ldr


class Rewritten(object):
    """The restated program of a code: gates, rows, and the outcome words of fault vectors."""

    def __init__(self, code, ops):
        self.code, self.ops = code, tuple(ops)
        self.gates, self.measurements, self.steps = program(code, self.ops)
        self.rows_x, self.rows_z, self.row_time, self.row_kind, self.ldr = layout(code, self.gates, self.measurements, self.steps)
        self.nsteps = len(self.steps)
        self.measure_mask = sum(1 << s for s, kind in enumerate(self.steps) if kind == MEASURE)
        self.locations = num_locations(self.gates)

    def outcome_words(self, f_x, f_z, chunk=16384):
        parts = [pack_words(propagate_rows(self.gates, 3 * self.code.n, f_x[:, s:s + chunk], f_z[:, s:s + chunk], self.rows_x, self.rows_z,
                                           self.row_time)) for s in range(0, f_x.shape[1], chunk)]
        return np.concatenate(parts) if parts else np.zeros((0, self.ldr), dtype=np.uint64)

    def tally(self, words):
        return tally(self.code, self.steps, words)


def correct(check, table, syndrome_of_word, errors):
    """quil_classical_correct (css_code.py:649-685) on a vector of known errors, given check . word: the syndrome of word ^ errors
    (:667-671; the product is linear) is looked up, a match XORs its correction into errors (:677-682), no match leaves them
    (:655-657).  Returns (errors, matched)."""
    key = cpu_ref.vec_to_int((syndrome_of_word + check @ errors) % 2)
    if key in table:
        return (errors + np.asarray(table[key])) % 2, True
    return errors, False


def classify(code, steps, word):
    """One sample's outcome words (Python ints) -> None if rejected, else (wrong, wrong trials, first trial wrong, split, unmatched_x,
    unmatched_z)."""
    nsteps = len(steps)
    if any(word[nsteps:]):
        return None                                                    # a verification fired (css_code.py:336-341): not this attempt
    r_1, r_2 = code.r_1, code.r_2
    z_operator = code.z_operator_matrix()[0]
    x_errors = np.zeros(code.n, dtype=np.int64)                        # data.x_errors, data.z_errors (qecc.py:14-33)
    z_errors = np.zeros(code.n, dtype=np.int64)
    unmatched_x = unmatched_z = 0
    outcomes = []
    for s, kind in enumerate(steps):
        measured_x = cpu_ref.int_to_vec(word[s] & ((1 << r_2) - 1), r_2)
        x_errors, found = correct(code.parity_check_c2, code._c2_syndromes, measured_x, x_errors)      # css_code.py:462 / :638
        unmatched_x += not found
        if kind == EC:
            measured_z = cpu_ref.int_to_vec((word[s] >> 32) & ((1 << r_1) - 1), r_1)
            z_errors, found = correct(code.parity_check_c1, code._c1_syndromes, measured_z, z_errors)  # css_code.py:470
            unmatched_z += not found
        else:                                                          # :685 leaves mem = measured ^ x_errors; :642-646 reads z_operator . mem
            outcomes.append(((word[s] >> 31) & 1) ^ (int(z_operator @ x_errors) & 1))
    ones = sum(outcomes)                                               # the frame's bits: 1 = differs from the noiseless trial
    return int(2 * ones > len(outcomes)), ones, outcomes[0], int(0 < ones < len(outcomes)), unmatched_x, unmatched_z


def tally(code, steps, words):
    """(counts[7] as Python ints, class byte per sample: bit 0 accepted, 1 wrong, 2 first trial wrong, 3 split vote, 4 an unmatched
    x key, 5 an unmatched z key)."""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    counts = [0] * 7
    classes = np.zeros(len(words), dtype=np.uint8)
    if len(words) == 0:
        return counts, classes
    unique, inverse, freq = np.unique(words, axis=0, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    byte = np.zeros(len(unique), dtype=np.uint8)
    for u, (row, times) in enumerate(zip(unique.tolist(), freq.tolist())):
        got = classify(code, steps, row)
        if got is None:
            continue
        wrong, ones, first, split, mx, mz = got
        byte[u] = 1 | wrong << 1 | first << 2 | split << 3 | (mx != 0) << 4 | (mz != 0) << 5
        for k, v in enumerate((1, wrong, ones, first, split, mx, mz)):
            counts[k] += v * times
    return counts, byte[inverse]
