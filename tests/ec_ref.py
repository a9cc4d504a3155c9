"""
The error-correction cycle restated in NumPy (DESIGN.md section 5b "Error-correction cycle"), sharing nothing with
quantum_css_codes_amd/ec_noise.py or the native library:

  gadget          the gate list and the measurements of `rounds` rounds of CSSCode.error_correct, written from the reference's
                  line numbers (css_code.py:314-366, 436-533), encoders from oracle.cpu_ref
  layout          those measurements as timed outcome rows in the outcome-word layout
  propagate_rows  forward Pauli-frame propagation with RESET and timed rows: every gate acts, then its locations' faults are
                  XOR-ed in; a row is read just before the gate of its time acts
  outcome_words   the packed outcome words of a batch of fault vectors
  tally           quil_classical_correct (css_code.py:649-685) round by round on a vector of known errors, with the code's own
                  table dicts and vec_to_int, then the judgement of the final frame; unique outcome rows are classified once
"""
import numpy as np

from oracle import cpu_ref

H, CNOT, IDLE, RESET = 0, 1, 2, 3
UNUSED, FINAL, ROUND, FLAG = 0, 1, 2, 3
FIELDS = ('accepted', 'logical_x', 'logical_z', 'logical_any', 'uncorrectable_x', 'uncorrectable_z', 'round_unmatched_x',
          'round_unmatched_z')


def encoder(code, state, qubits):
    make = cpu_ref.encode_zero_gates if state == 'zero' else cpu_ref.encode_plus_gates
    return [tuple(int(v) for v in g) for g in np.asarray(make(code, qubits)).reshape(-1, 3)]


def gadget(code, rounds=1, idle_data=False):
    """(gates, measurements): gates (g, 3) int32; a measurement is (time, kind, round, qubits, matrix): the Z-basis readout of
    `qubits` just before gate `time`, multiplied by `matrix`."""
    n = code.n
    data, a_1, a_2 = list(range(0, n)), list(range(n, 2 * n)), list(range(2 * n, 3 * n))
    h_1, h_2 = np.asarray(code.parity_check_c1), np.asarray(code.parity_check_c2)
    gates, measurements = [], []

    def reset(block):
        gates.extend((RESET, q, 0) for q in block)

    def measure(block, matrix, kind, rnd):
        gates.extend((IDLE, q, 0) for q in block)
        measurements.append((len(gates), kind, rnd, list(block), np.asarray(matrix) & 1))

    def error_detect_x(block, rnd, include_operators):                 # css_code.py:472-501
        reset(a_2)                                                     # :487
        gates.extend(encoder(code, 'zero' if include_operators else 'plus', a_2))   # :488-491
        gates.extend((CNOT, block[i], a_2[i]) for i in range(n))       # :494
        check = h_2                                                    # :498-500
        if include_operators:
            check = np.concatenate([check, code.z_operator_matrix()], axis=0)
        measure(a_2, check, FLAG, rnd)                                 # :495, :501

    def error_detect_z(block, rnd, include_operators):                 # css_code.py:503-533
        reset(a_2)                                                     # :518
        gates.extend(encoder(code, 'plus' if include_operators else 'zero', a_2))   # :519-522
        gates.extend((CNOT, a_2[i], block[i]) for i in range(n))       # :525
        gates.extend((H, a_2[i], 0) for i in range(n))                 # :526
        check = h_1                                                    # :530-532
        if include_operators:
            check = np.concatenate([check, code.x_operator_matrix()], axis=0)
        measure(a_2, check, FLAG, rnd)                                 # :527, :533

    def encode(block, state, rnd):                                     # css_code.py:314-366, the loop body once
        reset(block)                                                   # :332 / :356
        gates.extend(encoder(code, state, block))                      # :333 / :357
        error_detect_x(block, rnd, include_operators=(state == 'zero'))  # :335 / :359
        error_detect_z(block, rnd, include_operators=(state == 'plus'))  # :338 / :362

    for rnd in range(1, rounds + 1):
        if idle_data:
            gates.extend((IDLE, q, 0) for q in data)
        encode(a_1, 'plus', rnd)                                       # css_code.py:458
        gates.extend((CNOT, data[i], a_1[i]) for i in range(n))        # :459
        measure(a_1, h_2, ROUND, rnd)                                  # :460-462
        encode(a_1, 'zero', rnd)                                       # :465
        gates.extend((CNOT, a_1[i], data[i]) for i in range(n))        # :466
        gates.extend((H, a_1[i], 0) for i in range(n))                 # :467
        measure(a_1, h_1, ROUND, rnd)                                  # :468-470
    return np.array(gates, dtype=np.int32).reshape(-1, 3), measurements


def num_locations(gates):
    return int(len(gates) + np.count_nonzero(gates[:, 0] == CNOT))


def layout(code, gates, measurements, rounds):
    """The outcome rows: (rows_x, rows_z, row_time, row_kind, row_round, ldr), row r = bit r & 63 of word r >> 6."""
    n, r_1, r_2 = code.n, code.r_1, code.r_2
    flags = sum(len(m[4]) for m in measurements if m[1] == FLAG)
    ldr = 1 + rounds + (flags + 63) // 64
    rows_x = np.zeros((64 * ldr, 3 * n), dtype=np.uint8)
    rows_z = np.zeros_like(rows_x)
    row_time = np.full(64 * ldr, len(gates), dtype=np.int64)
    row_kind = np.zeros(64 * ldr, dtype=np.int8)
    row_round = np.zeros(64 * ldr, dtype=np.int8)
    flag = 0
    seen = {}
    for time, kind, rnd, qubits, matrix in measurements:
        if kind == ROUND:                                              # each round: first the Z-basis half (key_x), then the X-basis half
            half = seen.get(rnd, 0)
            seen[rnd] = half + 1
            r = r_1 if half else r_2
            bits = [64 * rnd + 32 * half + r - 1 - i for i in range(r)]
        else:
            bits = list(range(64 * (1 + rounds) + flag, 64 * (1 + rounds) + flag + len(matrix)))
            flag += len(matrix)
        for bit, row in zip(bits, matrix):
            rows_x[bit, qubits] = row
            row_time[bit], row_kind[bit], row_round[bit] = time, kind, rnd
    for i in range(r_2):
        rows_x[r_2 - 1 - i, :n] = code.parity_check_c2[i]
    rows_x[31, :n] = code.z_operator_matrix()[0]
    for i in range(r_1):
        rows_z[32 + r_1 - 1 - i, :n] = code.parity_check_c1[i]
    rows_z[63, :n] = code.x_operator_matrix()[0]
    row_kind[[r_2 - 1 - i for i in range(r_2)] + [31] + [32 + r_1 - 1 - i for i in range(r_1)] + [63]] = FINAL
    return rows_x, rows_z, row_time, row_kind, row_round, ldr


def propagate_rows(gates, n, f_x, f_z, rows_x, rows_z, row_time):
    """Row values (count, nrows) of fault vectors f_x, f_z (L, count): the frame starts at zero; RESET clears its qubit, H swaps,
    CNOT copies, then the gate's locations' faults are XOR-ed in; row r is read on the frame just before gate row_time[r]."""
    count = f_x.shape[1]
    e_x = np.zeros((n, count), dtype=np.uint8)
    e_z = np.zeros((n, count), dtype=np.uint8)
    out = np.zeros((count, len(row_time)), dtype=np.uint8)
    by_time = {}
    for r, t in enumerate(np.asarray(row_time).tolist()):
        if rows_x[r].any() or rows_z[r].any():
            by_time.setdefault(t, []).append(r)

    def read(t):
        rows = by_time.get(t)
        if rows:
            # (float32 products of 0/1 entries over at most a few hundred qubits are exact)
            value = rows_x[rows].astype(np.float32) @ e_x.astype(np.float32) + rows_z[rows].astype(np.float32) @ e_z.astype(np.float32)
            out[:, rows] = (value.astype(np.int64) & 1).T

    loc = 0
    for g, (kind, a, b) in enumerate(np.asarray(gates).tolist()):
        read(g)
        if kind == H:
            e_x[a], e_z[a] = e_z[a].copy(), e_x[a].copy()
        elif kind == CNOT:
            e_x[b] ^= e_x[a]
            e_z[a] ^= e_z[b]
        elif kind == RESET:
            e_x[a] = 0
            e_z[a] = 0
        for q in ((a, b) if kind == CNOT else (a,)):
            e_x[q] ^= f_x[loc]
            e_z[q] ^= f_z[loc]
            loc += 1
    read(len(gates))
    assert loc == f_x.shape[0]
    return out


def pack_words(bits):
    """(count, 64 * ldr) row values as (count, ldr) uint64 words."""
    count, nrows = bits.shape
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view("<u8").reshape(count, nrows // 64)


class Cycle(object):
    """The restated cycle of a code: gates, rows, and the outcome words of fault vectors."""

    def __init__(self, code, rounds=1, idle_data=False):
        self.code, self.rounds = code, rounds
        self.gates, self.measurements = gadget(code, rounds, idle_data)
        self.rows_x, self.rows_z, self.row_time, self.row_kind, self.row_round, self.ldr = layout(code, self.gates, self.measurements, rounds)
        self.locations = num_locations(self.gates)

    def outcome_words(self, f_x, f_z, chunk=16384):
        parts = [pack_words(propagate_rows(self.gates, 3 * self.code.n, f_x[:, s:s + chunk], f_z[:, s:s + chunk], self.rows_x, self.rows_z,
                                           self.row_time)) for s in range(0, f_x.shape[1], chunk)]
        return np.concatenate(parts) if parts else np.zeros((0, self.ldr), dtype=np.uint64)

    def tally(self, words):
        return tally(self.code, self.rounds, words)


def classify(code, rounds, word):
    """One sample's outcome words (Python ints) -> None if rejected, else (flip_x, flip_z, unc_x, unc_z, unmatched_x, unmatched_z)."""
    if any(word[rounds + 1:]):
        return None
    result = []
    sides = ((code.parity_check_c2, code._c2_syndromes, code.z_operator_matrix()[0], code.r_2, 0),
             (code.parity_check_c1, code._c1_syndromes, code.x_operator_matrix()[0], code.r_1, 32))
    for check, table, operator, r, shift in sides:
        known = np.zeros(code.n, dtype=np.int64)                       # CodeBlock.x_errors / z_errors
        unmatched = 0
        for t in range(1, rounds + 1):                                 # quil_classical_correct, css_code.py:649-685
            measured = cpu_ref.int_to_vec((word[t] >> shift) & ((1 << r) - 1), r)
            syndrome = (measured + check @ known) % 2                  # :667-671 (the syndrome is linear in the codeword)
            key = cpu_ref.vec_to_int(syndrome)
            if key in table:
                known = (known + np.asarray(table[key])) % 2           # :677-682
            else:
                unmatched += 1                                         # :655-657
        final = cpu_ref.int_to_vec((word[0] >> shift) & ((1 << r) - 1), r)
        key = cpu_ref.vec_to_int((final + check @ known) % 2)
        flip = ((word[0] >> (shift + 31)) & 1) ^ (int(operator @ known) & 1)
        if key in table:
            flip ^= int(operator @ np.asarray(table[key])) & 1
        result.append((flip, int(key not in table), unmatched))
    (fx, ux, mx), (fz, uz, mz) = result
    return fx, fz, ux, uz, mx, mz


def tally(code, rounds, words):
    """(counts[8] as Python ints, class byte per sample)."""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    counts = [0] * 8
    classes = np.zeros(len(words), dtype=np.uint8)
    if len(words) == 0:
        return counts, classes
    unique, inverse, freq = np.unique(words, axis=0, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    byte = np.zeros(len(unique), dtype=np.uint8)
    for u, (row, times) in enumerate(zip(unique.tolist(), freq.tolist())):
        got = classify(code, rounds, row)
        if got is None:
            continue
        fx, fz, ux, uz, mx, mz = got
        byte[u] = 1 | fx << 1 | fz << 2 | ux << 3 | uz << 4
        for k, v in enumerate((1, fx, fz, fx | fz, ux, uz, mx, mz)):
            counts[k] += v * times
    return counts, byte[inverse]
