"""
Fault Monte-Carlo of the error-correction cycle [build-defined; DESIGN.md "Error-correction cycle"].

The encoders circuit_noise.py studies are a sub-circuit of what the reference builds them for: CSSCode.error_correct
(css_code.py:436-470), Steane's error-correction gadget.  This module says how often that gadget fails: the logical error rate
per cycle of `rounds` rounds at physical fault rates (p_x, p_y, p_z) per location.

Registers: three blocks of n qubits, data D = 0 .. n-1, A1 = n .. 2n-1, A2 = 2n .. 3n-1.  A round is, as css_code.py:458-470,
    prep(A1, plus); CNOT D[i] -> A1[i]; measure A1 against parity_check_c2 (this round's key_x);
    prep(A1, zero); CNOT A1[i] -> D[i]; H on A1; measure A1 against parity_check_c1 (key_z)
and prep(B, s) is ONE attempt of encode_plus / encode_zero (css_code.py:314-366): RESET B, the noisy encoder, _error_detect_x and
_error_detect_z against a freshly reset and encoded A2 (css_code.py:472-533).  Every row of those detections is a flag row.
A measurement is no gate: it is a set of outcome rows read at its moment (a time per row), and its error is one IDLE gate on
every measured qubit immediately before.  RESET clears the frame of its qubit and has one fault location (a preparation fault).

Repeat-until-success is post-selection.  One sample is one draw of the Monte-Carlo sampler over all L locations -- one attempt
per preparation -- and a sample with any flag bit set is rejected.  Attempts are independent, and the model puts no fault on the
data block while it waits, so the accepted samples have exactly the distribution of the reference's while_do loop;
samples / accepted is the expected number of whole-cycle attempts per accepted one under this model.

Corrections are recorded (CodeBlock.x_errors, quil_classical_correct, css_code.py:649-685), never applied to the qubits, so
everything but the table lookups is linear over GF(2) and one effect table carries the whole gadget.  The tally rule -- round
t's syndrome decoded relative to what earlier rounds recorded, the final data frame judged against the record -- is stated in
DESIGN.md and include/gf2hip.h; gf2_ec_tally_host is its serial form and gf2_mc_ec_decode the device kernel.
"""
import contextlib
import math

import numpy as np

from . import _native
from . import circuit_noise

GATE_H, GATE_CNOT, GATE_IDLE, GATE_RESET = _native.GATE_H, _native.GATE_CNOT, _native.GATE_IDLE, _native.GATE_RESET
MAX_ROUNDS = _native.EC_MAX_ROUNDS
EC_FIELDS = ('accepted', 'logical_x', 'logical_z', 'logical_any', 'uncorrectable_x', 'uncorrectable_z', 'round_unmatched_x',
             'round_unmatched_z')
ROW_UNUSED, ROW_FINAL, ROW_ROUND, ROW_FLAG = 0, 1, 2, 3
KINDS = ('X', 'Y', 'Z')                             # the columns of single_faults' class bytes
CLASS_ACCEPTED, CLASS_FLIP_X, CLASS_FLIP_Z, CLASS_UNCORRECTABLE_X, CLASS_UNCORRECTABLE_Z = 1, 2, 4, 8, 16
CLASS_NAMES = ('accepted', 'flip_x', 'flip_z', 'uncorrectable_x', 'uncorrectable_z')      # the class byte's bits, from bit 0


class ECGates(object):
    """What error_correct_gates returns: `gates` (g, 3) int32 rows (kind, a, b) on `qubits` = 3n qubits; the outcome rows `rows_x`,
    `rows_z` (64 * ldr, 3n) uint8, row r being bit r & 63 of outcome word r >> 6, with their times `row_time`; `row_kind` (ROW_UNUSED,
    ROW_FINAL, ROW_ROUND, ROW_FLAG) and `row_round` (1 .. rounds for round and flag rows, else 0); `flag_rows`, the rows of the
    verifications in measurement order; `spans`, the parts of the gadget as (first gate, end gate, path) with path a tuple of names
    from the outermost part in (GadgetBuilder.span)."""

    def __init__(self, gates, qubits, rounds, ldr, rows_x, rows_z, row_time, row_kind, row_round, flag_rows, spans=()):
        self.gates, self.qubits, self.rounds, self.ldr = gates, qubits, rounds, ldr
        self.rows_x, self.rows_z, self.row_time, self.row_kind, self.row_round = rows_x, rows_z, row_time, row_kind, row_round
        self.flag_rows = flag_rows
        self.spans = tuple(spans)

    def gate_paths(self):
        """Per gate, the path of the innermost part it belongs to (() for a gate in none): what a fault list is grouped by."""
        paths = [()] * len(self.gates)
        for first, end, path in sorted(self.spans, key=lambda span: len(span[2])):     # inner parts overwrite the parts around them
            paths[first:end] = [path] * (end - first)
        return paths

    @property
    def num_rows(self):
        return int(np.count_nonzero(self.row_kind))


def _encoder(code, state, qubits):
    from .css_code import CSSCode                   # (any object with n, r_1, r_2 and the two checks will do)
    make = CSSCode.encode_zero_gates if state == 'zero' else CSSCode.encode_plus_gates
    return make(code, qubits).tolist()


class GadgetBuilder(object):
    """The gate list and the timed outcome rows of a sequence of gadgets on the three blocks, as they are emitted: `gates`, rows
    (kind, a, b), and `rows`, tuples (bit or None for a flag row, kind, round, time, block, side, vector).  error_correct_gates
    and ft_noise.program_gates are written with it."""

    def __init__(self, code):
        self.code, self.n, self.r_1, self.r_2 = code, int(code.n), int(code.r_1), int(code.r_2)
        if min(self.r_1, self.r_2) < 1 or max(self.r_1, self.r_2) > 31:
            raise ValueError("the error-correction cycle needs 1 <= r_1, r_2 <= 31 (both keys of a frame share an outcome word)")
        self.h_1, self.h_2 = np.asarray(code.parity_check_c1), np.asarray(code.parity_check_c2)
        self.z_op, self.x_op = np.asarray(code.z_operator_matrix()), np.asarray(code.x_operator_matrix())
        self.data, self.anc_1, self.anc_2 = (list(range(b * self.n, (b + 1) * self.n)) for b in range(3))
        self.gates = []
        self.rows = []
        self.spans, self._path = [], []

    @contextlib.contextmanager
    def span(self, name):
        """The gates emitted inside are the part `name` of the part around them (ECGates.spans)."""
        self._path.append(name)
        first = len(self.gates)
        try:
            yield
        finally:
            self.spans.append((first, len(self.gates), tuple(self._path)))
            self._path.pop()

    def measure(self, block, matrix, kind, rnd, bits):
        with self.span("measure (idle)"):
            self.gates.extend((GATE_IDLE, q, 0) for q in block)     # measurement error
        for row, bit in zip(matrix, bits):
            self.rows.append((bit, kind, rnd, len(self.gates), block, 0, row))

    def detect_x(self, block, verifier, rnd, include_operators):    # css_code.py:472-501
        state = 'zero' if include_operators else 'plus'
        with self.span("detect_x"):
            with self.span("verifier reset"):
                self.gates.extend((GATE_RESET, q, 0) for q in verifier)
            with self.span("verifier encode_%s" % state):
                self.gates.extend(_encoder(self.code, state, verifier))
            with self.span("CNOT block -> verifier"):
                self.gates.extend((GATE_CNOT, b, a) for b, a in zip(block, verifier))
            matrix = np.concatenate([self.h_2, self.z_op]) if include_operators else self.h_2
            self.measure(verifier, matrix, ROW_FLAG, rnd, [None] * len(matrix))

    def detect_z(self, block, verifier, rnd, include_operators):    # css_code.py:503-533
        state = 'plus' if include_operators else 'zero'
        with self.span("detect_z"):
            with self.span("verifier reset"):
                self.gates.extend((GATE_RESET, q, 0) for q in verifier)
            with self.span("verifier encode_%s" % state):
                self.gates.extend(_encoder(self.code, state, verifier))
            with self.span("CNOT verifier -> block"):
                self.gates.extend((GATE_CNOT, a, b) for b, a in zip(block, verifier))
            with self.span("H verifier"):
                self.gates.extend((GATE_H, a, 0) for a in verifier)
            matrix = np.concatenate([self.h_1, self.x_op]) if include_operators else self.h_1
            self.measure(verifier, matrix, ROW_FLAG, rnd, [None] * len(matrix))

    def prep(self, block, state, rnd, verifier=None):               # css_code.py:314-366, one attempt
        verifier = self.anc_2 if verifier is None else verifier
        with self.span("prep %s" % state):
            with self.span("reset"):
                self.gates.extend((GATE_RESET, q, 0) for q in block)
            with self.span("encode_%s" % state):
                self.gates.extend(_encoder(self.code, state, block))
            self.detect_x(block, verifier, rnd, include_operators=state == 'zero')
            self.detect_z(block, verifier, rnd, include_operators=state == 'plus')

    def error_correct(self, rnd, word):                             # css_code.py:458-470; the keys go to outcome word `word`
        r_1, r_2 = self.r_1, self.r_2
        with self.span("x half"):
            self.prep(self.anc_1, 'plus', rnd)
            with self.span("CNOT data -> ancilla"):
                self.gates.extend((GATE_CNOT, d, a) for d, a in zip(self.data, self.anc_1))
            self.measure(self.anc_1, self.h_2, ROW_ROUND, rnd, [64 * word + r_2 - 1 - i for i in range(r_2)])
        with self.span("z half"):
            self.prep(self.anc_1, 'zero', rnd)
            with self.span("CNOT ancilla -> data"):
                self.gates.extend((GATE_CNOT, a, d) for d, a in zip(self.data, self.anc_1))
            with self.span("H ancilla"):
                self.gates.extend((GATE_H, a, 0) for a in self.anc_1)
            self.measure(self.anc_1, self.h_1, ROW_ROUND, rnd, [64 * word + 32 + r_1 - 1 - i for i in range(r_1)])

    @property
    def num_flags(self):
        return sum(1 for row in self.rows if row[0] is None)

    def arrays(self, ldr, first_flag_word):
        """(gates, rows_x, rows_z, row_time, row_kind, row_round, flag_rows) for ldr outcome words, the flag rows from word
        first_flag_word on in measurement order."""
        end = len(self.gates)
        rows_x = np.zeros((64 * ldr, 3 * self.n), dtype=np.uint8)
        rows_z = np.zeros_like(rows_x)
        row_time = np.full(64 * ldr, end, dtype=np.int64)
        row_kind = np.zeros(64 * ldr, dtype=np.int8)
        row_round = np.zeros(64 * ldr, dtype=np.int8)
        flag_rows = []
        for bit, kind, rnd, time, block, side, vector in self.rows:
            if bit is None:
                bit = 64 * first_flag_word + len(flag_rows)
                flag_rows.append(bit)
            (rows_z if side else rows_x)[bit, block] = np.asarray(vector) & 1
            row_time[bit], row_kind[bit], row_round[bit] = time, kind, rnd
        return (np.array(self.gates, dtype=np.int32).reshape(-1, 3), rows_x, rows_z, row_time, row_kind, row_round,
                np.array(flag_rows, dtype=np.int64))


def error_correct_gates(code, rounds=1, idle_data=False):
    """The gate list and timed outcome rows of `rounds` rounds of CSSCode.error_correct (the module docstring has the order), one
    attempt per preparation; idle_data adds one IDLE per data qubit at the start of each round.  Returns an ECGates."""
    rounds = int(rounds)
    build = GadgetBuilder(code)
    if not 1 <= rounds <= MAX_ROUNDS:
        raise ValueError("the error-correction cycle needs 1 <= rounds <= %d" % MAX_ROUNDS)
    r_1, r_2, data = build.r_1, build.r_2, build.data
    for t in range(1, rounds + 1):                                  # css_code.py:458-470
        with build.span("round %d" % t):
            if idle_data:
                with build.span("data idle"):
                    build.gates.extend((GATE_IDLE, q, 0) for q in data)
            build.error_correct(t, t)
    end = len(build.gates)
    for i in range(r_2):                                            # vec_to_int: row 0 is the most significant bit
        build.rows.append((r_2 - 1 - i, ROW_FINAL, 0, end, data, 0, build.h_2[i]))
    build.rows.append((31, ROW_FINAL, 0, end, data, 0, build.z_op[0]))
    for i in range(r_1):
        build.rows.append((32 + r_1 - 1 - i, ROW_FINAL, 0, end, data, 1, build.h_1[i]))
    build.rows.append((63, ROW_FINAL, 0, end, data, 1, build.x_op[0]))

    flags = build.num_flags
    ldr = 1 + rounds + (flags + 63) // 64
    if ldr > _native.CIRCUIT_MAX_LDR:
        raise ValueError("%d rounds with %d flag rows need %d outcome words per sample, more than %d"
                         % (rounds, flags, ldr, _native.CIRCUIT_MAX_LDR))
    gates, rows_x, rows_z, row_time, row_kind, row_round, flag_rows = build.arrays(ldr, 1 + rounds)
    return ECGates(gates, 3 * build.n, rounds, ldr, rows_x, rows_z, row_time, row_kind, row_round, flag_rows, build.spans)


class ECCircuit(object):
    """The error-correction cycle of a code prepared for the Monte-Carlo: the gadget (error_correct_gates), its effect table
    (gf2_circuit_effects_timed, host code) and, on first use, the device copy."""

    def __init__(self, code, rounds=1, idle_data=False):
        self.code = code
        self.rounds = int(rounds)
        self.gadget = error_correct_gates(code, rounds, idle_data)
        self.ldr = self.gadget.ldr
        self.effects, self.locations = _native.circuit_effects_timed(
            self.gadget.gates, self.gadget.qubits, _native.pack_rows(self.gadget.rows_x), _native.pack_rows(self.gadget.rows_z),
            self.gadget.row_time, ldr=self.ldr)
        self._device = None
        self._sites = None

    @property
    def num_locations(self):
        return len(self.locations)

    def device(self):
        if self._device is None:
            if not 1 <= self.num_locations <= circuit_noise.MAX_LOCATIONS:
                raise ValueError("the Monte-Carlo needs 1 <= L <= %d (2^20) fault locations, the cycle has %d"
                                 % (circuit_noise.MAX_LOCATIONS, self.num_locations))
            self._device = _native.default_context().circuit_create(self.effects)
        return self._device

    def _tables(self):
        keys1, flips1, keys2, flips2 = circuit_noise.code_tables(self.code)
        return self.code.r_1, keys1, flips1, self.code.r_2, keys2, flips2

    def outcomes(self, num_samples, p_x, p_y, p_z, seed=0, first_sample=0):
        """The outcome words of samples [first_sample, first_sample + num_samples), rejected ones included: a (num_samples, ldr)
        uint64 array (gf2_circuit_outcomes_dev)."""
        ctx = _native.default_context()
        circ = self.device()
        count = int(num_samples)
        buf = ctx.alloc(max(1, count) * self.ldr * 8)
        ctx.circuit_outcomes_dev(circ, int(seed), int(first_sample), count, float(p_x), float(p_y), float(p_z), buf, self.ldr)
        out = buf.download((count, self.ldr), np.uint64)
        buf.free()
        return out

    def logical_error_rates(self, num_samples, p_x, p_y, p_z, seed=0, first_sample=0):
        """The tally of samples [first_sample, first_sample + num_samples) on the device: a dict of EC_FIELDS plus 'samples'.
        Every field after 'accepted' counts among accepted samples; the counts of sample ranges add."""
        counts = _native.default_context().mc_ec_decode(self.device(), self.rounds, *self._tables(), int(seed), int(first_sample),
                                                        int(num_samples), float(p_x), float(p_y), float(p_z))
        out = {name: int(v) for name, v in zip(EC_FIELDS, counts)}
        out['samples'] = int(num_samples)
        return out

    def tally_host(self, words, classes=False):
        """The tally rule over outcome words (samples, ldr) on the host (gf2_ec_tally_host, no GPU): the dict of EC_FIELDS plus
        'samples'; classes=True returns (dict, class byte per sample) instead."""
        words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, self.ldr)
        got = _native.ec_tally_host(words, self.rounds, *self._tables(), classes=classes)
        counts = got[0] if classes else got
        out = {name: int(v) for name, v in zip(EC_FIELDS, counts)}
        out['samples'] = len(words)
        return (out, got[1]) if classes else out

    def enumerate_strata(self, weights, first_rank=None, count=None, max_configurations=None, host=False):
        """Exact strata of the cycle (DESIGN.md "Exact strata of the cycle"): every configuration of exactly weights[s] <= 8 faults
        -- each subset of the L locations with every assignment of X, Y, Z to its picks -- judged by logical_error_rates' tally
        rule, post-selection included, and counted per kind composition.  Arguments as FaultCircuit.enumerate_strata's: ranks
        [first_rank, first_rank + count) per weight (default: everything), more than `max_configurations` (default
        circuit_noise.ENUMERATE_BUDGET) configurations in all is a ValueError, host=True runs the serial host statement
        (gf2_ec_enumerate_host) and needs no GPU.  Returns a montecarlo.PostSelectedStrata over nb = L."""
        from . import montecarlo
        weights, firsts, counts = circuit_noise.gadget_enumerate_request(self.num_locations, weights, first_rank, count, max_configurations,
                                                                         "cycle")
        if host:
            run = lambda w, f, n: _native.ec_enumerate_host(self.effects, self.rounds, *self._tables(), w, f, n)
        else:
            ctx, circ = _native.default_context(), self.device()
            run = lambda w, f, n: ctx.ec_enumerate(circ, self.rounds, *self._tables(), w, f, n)
        return montecarlo.PostSelectedStrata(self.num_locations, weights, [run(w, f, n) for w, f, n in zip(weights, firsts, counts)],
                                             EC_FIELDS)

    def malignant_faults(self, weight, select=CLASS_FLIP_X | CLASS_FLIP_Z, first_rank=None, count=None, max_configurations=None, host=False):
        """The malignant fault sets of the cycle (DESIGN.md "Malignant fault sets of the cycle"): enumerate_strata's walk of the
        configurations of exactly `weight` <= 8 faults over ranks [first_rank, first_rank + count) (default: everything), but the
        accepted ones whose class byte has a bit of `select` (CLASS_* bits; CLASS_ACCEPTED lists every accepted one) are listed,
        not counted (gf2_ec_enumerate_list; host=True: gf2_ec_enumerate_list_host, no GPU).  Budget as enumerate_strata's; more
        than 2^26 records is a ValueError.  Returns a montecarlo.FaultList over nb = L, which describe() puts into words."""
        from . import montecarlo
        if host:
            run = lambda w, f, n, select, capacity: _native.ec_enumerate_list_host(self.effects, self.rounds, *self._tables(), w, f, n, select, capacity)
        else:
            ctx, circ = _native.default_context(), self.device()
            run = lambda w, f, n, select, capacity: ctx.ec_enumerate_list(circ, self.rounds, *self._tables(), w, f, n, select, capacity)
        return montecarlo.malignant_faults(self.num_locations, weight, CLASS_NAMES, select, first_rank, count, max_configurations, "cycle", run)

    def describe(self, fault_list):
        """Every record of a FaultList of this cycle as a tuple over its picks of (gate index, gate (kind, a, b), qubit, 'X' / 'Y' /
        'Z'): single_faults' format, so the weight-1 list of the default select reads as single_faults()[1]."""
        return describe_faults(self, fault_list)

    def strata(self, weights, samples, kinds=(1, 1, 1), seed=0, first_sample=0, host=False):
        """Sampled strata of the cycle (DESIGN.md "Sampled strata of the cycle"): stratum s draws samples [first_sample, first_sample +
        samples[s]) of exactly weights[s] <= 16 faults among the L locations, kinds X : Y : Z = kinds, and judges them by
        logical_error_rates' tally rule, post-selection included (gf2_mc_ec_decode_strata).  `samples` and `first_sample` are one
        number for all strata or one per stratum.  host=True draws the outcome words with gf2_stratum_outcomes_host and tallies them
        with gf2_ec_tally_host: no GPU.  Returns a montecarlo.SampledPostSelectedStrata over nb = L."""
        from . import montecarlo
        tables = self._tables()
        if host:
            run = montecarlo.host_strata_run(self.effects, lambda words: _native.ec_tally_host(words, self.rounds, *tables), len(EC_FIELDS), seed)
        else:
            ctx, circ = _native.default_context(), self.device()
            run = lambda first, ws, ns, ks: ctx.mc_ec_decode_strata(circ, self.rounds, *tables, int(seed), int(first), ws, ns, *ks)
        return montecarlo.gadget_strata_local(self.num_locations, EC_FIELDS, weights, samples, kinds, first_sample, run)

    def gate_sites(self):
        """(site_loc, n1, n2, site_gate) of the cycle's gates (circuit_noise.gate_sites), made once."""
        if self._sites is None:
            self._sites = circuit_noise.gate_sites(self.gadget.gates, self.locations)
        return self._sites

    def enumerate_gate_range(self, w, b, first_rank, count, host=False):
        """One call of the gate-fault enumeration: the (b + 1, 8) uint64 counts [c][field] over the site
        subsets of ranks [first_rank, first_rank + count) of weight w with b CNOT picks, c the number of two-operand kinds
        (gf2_ec_gate_enumerate; host=True: gf2_ec_gate_enumerate_host, no GPU).  Counts of disjoint ranges add."""
        sites = self.gate_sites()[:3]
        if host:
            return _native.ec_gate_enumerate_host(self.effects, self.rounds, *self._tables(), *sites, w, b, first_rank, count)
        return _native.default_context().ec_gate_enumerate(self.device(), self.rounds, *self._tables(), *sites, w, b, first_rank, count)

    def enumerate_gate_strata(self, weights, max_configurations=None, host=False):
        """Exact strata of the cycle under gate-level faults: every configuration of exactly weights[s] <= 4
        faulty gates -- a one-operand gate with X, Y or Z, a CNOT with one of the 15 two-qubit Paulis -- judged by
        logical_error_rates' tally rule, post-selection included, whole strata, every CNOT count b.  More than `max_configurations`
        (default circuit_noise.ENUMERATE_BUDGET) configurations in all is a ValueError.  Returns a montecarlo.GateStrata."""
        return gate_strata(self, EC_FIELDS, weights, max_configurations, host, "cycle")

    def gate_strata(self, strata, samples, seed=0, first_sample=0, host=False):
        """Sampled strata of the cycle under gate-level faults (DESIGN.md section 5e "Sampled strata under gate-level faults"):
        stratum s = (a, b) draws samples [first_sample, first_sample + samples[s]) of exactly a faulty one-operand gates and b faulty
        CNOTs, a + b <= 16, kinds uniform over the 3 and the 15, and judges them by logical_error_rates' tally rule, post-selection
        included, tallied by the number c of two-operand kinds (gf2_mc_ec_decode_gate_strata).  `samples` and `first_sample` are one
        number for all strata or one per stratum.  host=True draws with gf2_gate_stratum_outcomes_host and tallies with
        gf2_ec_tally_host: no GPU.  Returns a montecarlo.SampledGateStrata."""
        from . import montecarlo
        tables, sites = self._tables(), self.gate_sites()[:3]
        if host:
            run = montecarlo.host_gate_strata_run(self.effects, sites, lambda words: _native.ec_tally_host(words, self.rounds, *tables),
                                                  len(EC_FIELDS), seed)
        else:
            ctx, circ = _native.default_context(), self.device()
            run = lambda first, strata, ns: ctx.mc_ec_decode_gate_strata(circ, self.rounds, *tables, *sites, int(seed), int(first), strata, ns)
        return montecarlo.gate_strata_local(sites[1], sites[2], EC_FIELDS, strata, samples, first_sample, run)

    def gate_error_rates(self, num_samples, p1, p2, seed=0, first_sample=0, host=False):
        """The direct Monte-Carlo of the cycle under gate-level faults (DESIGN.md section 5e "Direct Monte-Carlo under gate-level
        faults"): in samples [first_sample, first_sample + num_samples) every one-operand gate fails with probability p1 and one of
        its 3 kinds, every CNOT as one event with probability p2 and one of its 15, and logical_error_rates' tally rule judges them,
        post-selection included (gf2_mc_ec_decode_gate).  host=True draws with gf2_gate_outcomes_host and tallies with
        gf2_ec_tally_host: no GPU.  Returns a dict of EC_FIELDS plus 'samples'; the counts of sample ranges add."""
        tables, sites = self._tables(), self.gate_sites()[:3]
        if host:
            from . import montecarlo
            counts = montecarlo.host_gate_counts(self.effects, sites, lambda words: _native.ec_tally_host(words, self.rounds, *tables),
                                                 len(EC_FIELDS), num_samples, p1, p2, seed, first_sample)
        else:
            counts = _native.default_context().mc_ec_decode_gate(self.device(), self.rounds, *tables, *sites, int(seed), int(first_sample),
                                                                 int(num_samples), float(p1), float(p2))
        out = {name: int(v) for name, v in zip(EC_FIELDS, counts)}
        out['samples'] = int(num_samples)
        return out

    def gate_single_faults(self):
        """The census of every single gate fault, no GPU: (classes, flipping) -- classes (G, 15) uint8, the class byte (CLASS_* bits)
        of kind mask kappa (column kappa - 1; a one-operand gate uses columns 0 .. 2, the others stay 0) at every gate of the list;
        flipping, the accepted faults with a logical flip as (gate index, gate (kind, a, b), Paulis) with Paulis one letter for a
        one-operand gate and control then target, e.g. 'XI' or 'ZY', for a CNOT."""
        return gate_single_faults(self, CLASS_FLIP_X | CLASS_FLIP_Z)

    def single_faults(self):
        """The census of all 3 L single faults, no GPU: (classes, flipping) -- classes (L, 3) uint8, the class byte (CLASS_* bits)
        of an X, Y, Z fault (the columns, KINDS) at every location; flipping, the accepted faults with a logical flip as
        (gate index, gate (kind, a, b), qubit, 'X' / 'Y' / 'Z')."""
        eff = self.effects
        words = np.stack((eff[:, 0], eff[:, 0] ^ eff[:, 1], eff[:, 1]), axis=1)              # X, Y, Z
        _, classes = self.tally_host(words.reshape(-1, self.ldr), classes=True)
        classes = classes.reshape(-1, 3)
        flipping = []
        for l, k in zip(*np.nonzero((classes & CLASS_ACCEPTED != 0) & (classes & (CLASS_FLIP_X | CLASS_FLIP_Z) != 0))):
            g, q = (int(v) for v in self.locations[l])
            flipping.append((g, tuple(int(v) for v in self.gadget.gates[g]), q, KINDS[k]))
        return classes, flipping


def describe_faults(gadget, fault_list):
    """ECCircuit.describe and FTProgram.describe: `gadget` has num_locations, locations (location -> gate, qubit) and gadget.gates."""
    if fault_list.nb != gadget.num_locations:
        raise ValueError("the list is over %d locations, the gadget has %d" % (fault_list.nb, gadget.num_locations))
    out = []
    for picks, kinds in zip(fault_list.locations().tolist(), fault_list.kinds().tolist()):
        row = []
        for l, k in zip(picks, kinds):
            g, q = (int(v) for v in gadget.locations[l])
            row.append((g, tuple(int(v) for v in gadget.gadget.gates[g]), q, KINDS[k]))
        out.append(tuple(row))
    return out


def gate_strata(gadget, fields, weights, max_configurations, host, what):
    """ECCircuit / FTProgram.enumerate_gate_strata: whole strata through gadget.enumerate_gate_range, stacked per weight into
    (w + 1, w + 1, F) counts [b][c]."""
    from . import montecarlo
    _, n1, n2, _ = gadget.gate_sites()
    weights = circuit_noise.gate_enumerate_request(n1, n2, weights, max_configurations, what)
    if not host:
        gadget.device()
    counts = []
    for w in weights:
        stack = np.zeros((w + 1, w + 1, len(fields)), dtype=np.uint64)
        for b in range(w + 1):
            stack[b, :b + 1] = gadget.enumerate_gate_range(w, b, 0, math.comb(n1, w - b) * math.comb(n2, b), host=host)
        counts.append(stack)
    return montecarlo.GateStrata(n1, n2, weights, counts, fields)


PAULI_OF_MASK = ('I', 'X', 'Z', 'Y')                # the two bits of a kind mask: 1 = X, 2 = Z, 3 = Y


def gate_single_faults(gadget, flip_mask):
    """ECCircuit / FTProgram.gate_single_faults: `flip_mask` the class bits that make an accepted fault one to list."""
    site_loc, n1, n2, site_gate = gadget.gate_sites()
    eff = gadget.effects
    gates = gadget.gadget.gates
    classes = np.zeros((len(gates), 15), dtype=np.uint8)
    for sites, nbits in ((slice(0, n1), 2), (slice(n1, n1 + n2), 4)):
        locs = site_loc[sites].astype(np.int64)
        if not len(locs):
            continue
        words = np.zeros((len(locs), (1 << nbits) - 1, gadget.ldr), dtype=np.uint64)
        for kappa in range(1, 1 << nbits):
            for bit in range(nbits):
                if (kappa >> bit) & 1:
                    words[:, kappa - 1] ^= eff[locs + (bit >> 1), bit & 1]
        _, cls = gadget.tally_host(words.reshape(-1, gadget.ldr), classes=True)
        classes[site_gate[sites], :(1 << nbits) - 1] = cls.reshape(len(locs), -1)
    flipping = []
    for g, k in zip(*np.nonzero((classes & CLASS_ACCEPTED != 0) & (classes & flip_mask != 0))):
        kappa = int(k) + 1
        gate = tuple(int(v) for v in gates[g])
        paulis = PAULI_OF_MASK[kappa & 3] + (PAULI_OF_MASK[kappa >> 2] if gate[0] == GATE_CNOT else '')
        flipping.append((int(g), gate, paulis))
    return classes, flipping


def circuit_for(code, rounds=1, idle_data=False):
    """ECCircuit(code, rounds, idle_data), cached on the code object."""
    cache = code.__dict__.setdefault("_ec_circuits", {})
    key = (int(rounds), bool(idle_data))
    if key not in cache:
        cache[key] = ECCircuit(code, rounds, idle_data)
    return cache[key]
