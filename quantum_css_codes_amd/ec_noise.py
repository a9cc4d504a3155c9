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
samples / accepted is the expected number of whole-cycle attempts per accepted one under this model.  (The model that does put
faults on the waiting data block, on every attempt of every preparation, is stream_noise.py's retry_wait_* route: DESIGN.md section
5d "Repeat-until-success with waiting faults".)

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


PAULI_OF_MASK = ('I', 'X', 'Z', 'Y')                # the two bits of a kind mask: 1 = X, 2 = Z, 3 = Y


class Gadget(object):
    """A post-selected gadget prepared for the Monte-Carlo, what ECCircuit and ft_noise.FTProgram are: the gate list `gadget` (an
    ECGates), its effect table (gf2_circuit_effects_timed, host code) and, on first use, the device copy, judged by one of _native's
    tally rules.  A subclass states
        rule, fields, class_names    the rule (_native.EC_RULE / FT_RULE), the names of its counts and of its class byte's bits
        flip_mask, noun              the class bits that make an accepted fault one to list; the gadget's name in error messages
        _create, _outcomes_dev       the Context methods that make the device copy and draw its outcome words
    and _head(), the rule's own arguments.  {ec,ft} below stands for the rule's prefix in the names of entry points."""

    def __init__(self, code, gadget):
        self.code, self.gadget, self.ldr = code, gadget, gadget.ldr
        self.effects, self.locations = _native.circuit_effects_timed(
            gadget.gates, gadget.qubits, _native.pack_rows(gadget.rows_x), _native.pack_rows(gadget.rows_z), gadget.row_time, ldr=self.ldr)
        self._device = None
        self._sites = None

    @property
    def num_locations(self):
        return len(self.locations)

    def device(self):
        if self._device is None:
            if not 1 <= self.num_locations <= circuit_noise.MAX_LOCATIONS:
                raise ValueError("the Monte-Carlo needs 1 <= L <= %d (2^20) fault locations, the %s has %d"
                                 % (circuit_noise.MAX_LOCATIONS, self.noun, self.num_locations))
            self._device = getattr(_native.default_context(), self._create)(self.effects)
        return self._device

    def _tables(self):
        keys1, flips1, keys2, flips2 = circuit_noise.code_tables(self.code)
        return self.code.r_1, keys1, flips1, self.code.r_2, keys2, flips2

    def _entry(self, name, host=False):
        """The rule's wrapper `name` (%s: the rule's prefix) with this gadget's leading arguments filled in: the default context's
        method on the device copy or, host=True, _native's host statement `name`_host on the effect table (no GPU)."""
        if host:
            fn, table = getattr(_native, (name + "_host") % self.rule.name), self.effects
        else:
            fn, table = getattr(_native.default_context(), name % self.rule.name), self.device()
        lead = (table,) + self._head() + self._tables()
        return lambda *rest: fn(*lead, *rest)

    def _tally(self, words, classes=False):
        return getattr(_native, "%s_tally_host" % self.rule.name)(words, *self._head(), *self._tables(), classes=classes)

    def _dict(self, counts, samples):
        out = {name: int(v) for name, v in zip(self.fields, counts)}
        out['samples'] = int(samples)
        return out

    def outcomes(self, num_samples, p_x, p_y, p_z, seed=0, first_sample=0):
        """The outcome words of samples [first_sample, first_sample + num_samples), rejected ones included: a (num_samples, ldr)
        uint64 array (gf2_circuit_outcomes_dev; a program: gf2_ft_outcomes_dev)."""
        ctx = _native.default_context()
        return ctx.outcomes(getattr(ctx, self._outcomes_dev), self.device(), seed, first_sample, num_samples, p_x, p_y, p_z, self.ldr)

    def _error_rates(self, num_samples, p_x, p_y, p_z, seed, first_sample):
        counts = self._entry("mc_%s_decode")(int(seed), int(first_sample), int(num_samples), float(p_x), float(p_y), float(p_z))
        return self._dict(counts, num_samples)

    def tally_host(self, words, classes=False):
        """The tally rule over outcome words (samples, ldr) on the host (gf2_{ec,ft}_tally_host, no GPU): the dict of `fields` plus
        'samples'; classes=True returns (dict, class byte per sample) instead."""
        words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, self.ldr)
        got = self._tally(words, classes)
        out = self._dict(got[0] if classes else got, len(words))
        return (out, got[1]) if classes else out

    def enumerate_strata(self, weights, first_rank=None, count=None, max_configurations=None, host=False):
        """Exact strata (DESIGN.md "Exact strata of the cycle", "Exact strata of the measurement"): every configuration of exactly
        weights[s] <= 8 faults -- each subset of the L locations with every assignment of X, Y, Z to its picks -- judged by the tally
        rule, post-selection included, and counted per kind composition.  Arguments as FaultCircuit.enumerate_strata's: ranks
        [first_rank, first_rank + count) per weight (default: everything), more than `max_configurations` (default
        circuit_noise.ENUMERATE_BUDGET) configurations in all is a ValueError, host=True runs the serial host statement
        (gf2_{ec,ft}_enumerate_host) and needs no GPU.  Returns a montecarlo.PostSelectedStrata over nb = L."""
        from . import montecarlo
        weights, firsts, counts = circuit_noise.gadget_enumerate_request(self.num_locations, weights, first_rank, count, max_configurations,
                                                                         self.noun)
        run = self._entry("%s_enumerate", host)
        return montecarlo.PostSelectedStrata(self.num_locations, weights, [run(w, f, n) for w, f, n in zip(weights, firsts, counts)],
                                             self.fields)

    def malignant_faults(self, weight, select=None, first_rank=None, count=None, max_configurations=None, host=False):
        """The malignant fault sets (DESIGN.md "Malignant fault sets of the cycle", "... of the measurement"): enumerate_strata's walk
        of the configurations of exactly `weight` <= 8 faults over ranks [first_rank, first_rank + count) (default: everything), but
        the accepted ones whose class byte has a bit of `select` (CLASS_* bits, default `flip_mask`: CLASS_FLIP_X | CLASS_FLIP_Z for a
        cycle, CLASS_WRONG for a program; CLASS_ACCEPTED lists every accepted one) are listed, not counted (gf2_{ec,ft}_enumerate_list;
        host=True: gf2_{ec,ft}_enumerate_list_host, no GPU).  Budget as enumerate_strata's; more than 2^26 records is a ValueError.
        Returns a montecarlo.FaultList over nb = L, which describe() puts into words."""
        from . import montecarlo
        return montecarlo.malignant_faults(self.num_locations, weight, self.class_names, self.flip_mask if select is None else select,
                                           first_rank, count, max_configurations, self.noun, self._entry("%s_enumerate_list", host))

    def _fault(self, location, kind):
        g, q = (int(v) for v in self.locations[location])
        return g, tuple(int(v) for v in self.gadget.gates[g]), q, KINDS[kind]

    def describe(self, fault_list):
        """Every record of a FaultList of this gadget as a tuple over its picks of (gate index, gate (kind, a, b), qubit, 'X' / 'Y' /
        'Z'): single_faults' format, so the weight-1 list of the default select reads as single_faults()[1]."""
        if fault_list.nb != self.num_locations:
            raise ValueError("the list is over %d locations, the gadget has %d" % (fault_list.nb, self.num_locations))
        return [tuple(self._fault(l, k) for l, k in zip(picks, kinds))
                for picks, kinds in zip(fault_list.locations().tolist(), fault_list.kinds().tolist())]

    def strata(self, weights, samples, kinds=(1, 1, 1), seed=0, first_sample=0, host=False):
        """Sampled strata (DESIGN.md "Sampled strata of the cycle", "Sampled strata of the measurement"): stratum s draws samples
        [first_sample, first_sample + samples[s]) of exactly weights[s] <= 16 faults among the L locations, kinds X : Y : Z = kinds,
        and judges them by the tally rule, post-selection included (gf2_mc_{ec,ft}_decode_strata).  `samples` and `first_sample` are
        one number for all strata or one per stratum.  host=True draws the outcome words with gf2_stratum_outcomes_host and tallies
        them with gf2_{ec,ft}_tally_host: no GPU.  Returns a montecarlo.SampledPostSelectedStrata over nb = L."""
        from . import montecarlo
        if host:
            run = montecarlo.host_strata_run(self.effects, self._tally, len(self.fields), seed)
        else:
            decode = self._entry("mc_%s_decode_strata")
            run = lambda first, ws, ns, ks: decode(int(seed), int(first), ws, ns, *ks)
        return montecarlo.gadget_strata_local(self.num_locations, self.fields, weights, samples, kinds, first_sample, run)

    def gate_sites(self):
        """(site_loc, n1, n2, site_gate) of the gadget's gates (circuit_noise.gate_sites), made once."""
        if self._sites is None:
            self._sites = circuit_noise.gate_sites(self.gadget.gates, self.locations)
        return self._sites

    def enumerate_gate_range(self, w, b, first_rank, count, host=False):
        """One call of the gate-fault enumeration: the (b + 1, F) uint64 counts [c][field] over the site
        subsets of ranks [first_rank, first_rank + count) of weight w with b CNOT picks, c the number of two-operand kinds
        (gf2_{ec,ft}_gate_enumerate; host=True: gf2_{ec,ft}_gate_enumerate_host, no GPU).  Counts of disjoint ranges add."""
        sites = self.gate_sites()[:3]
        return self._entry("%s_gate_enumerate", host)(*sites, w, b, first_rank, count)

    def enumerate_gate_strata(self, weights, max_configurations=None, host=False):
        """Exact strata under gate-level faults: every configuration of exactly weights[s] <= 4 faulty gates
        -- a one-operand gate with X, Y or Z, a CNOT with one of the 15 two-qubit Paulis -- judged by the tally rule, post-selection
        included, whole strata, every CNOT count b, through enumerate_gate_range.  More than `max_configurations` (default
        circuit_noise.ENUMERATE_BUDGET) configurations in all is a ValueError.  Returns a montecarlo.GateStrata, the counts of a
        weight stacked into (w + 1, w + 1, F) [b][c]."""
        from . import montecarlo
        _, n1, n2, _ = self.gate_sites()
        weights = circuit_noise.gate_enumerate_request(n1, n2, weights, max_configurations, self.noun)
        if not host:
            self.device()
        counts = []
        for w in weights:
            stack = np.zeros((w + 1, w + 1, len(self.fields)), dtype=np.uint64)
            for b in range(w + 1):
                stack[b, :b + 1] = self.enumerate_gate_range(w, b, 0, math.comb(n1, w - b) * math.comb(n2, b), host=host)
            counts.append(stack)
        return montecarlo.GateStrata(n1, n2, weights, counts, self.fields)

    def malignant_gate_faults(self, weight, b=None, select=None, first_rank=0, count=None, max_configurations=None, host=False):
        """The malignant fault sets under gate-level faults (DESIGN.md section 5e "Malignant fault sets under gate-level faults"):
        enumerate_gate_range's walk of the configurations of exactly `weight` <= 4 faulty gates, b of them CNOTs, over ranks
        [first_rank, first_rank + count) (default: everything), but the accepted ones whose class byte has a bit of `select`
        (default `flip_mask`, as malignant_faults) are listed, not counted (gf2_{ec,ft}_gate_enumerate_list; host=True:
        gf2_{ec,ft}_gate_enumerate_list_host, no GPU).  b=None lists the whole stratum of every b and takes no rank range.  Budget
        as enumerate_gate_strata's; more than 2^26 records is a ValueError.  Returns a montecarlo.GateFaultList -- a
        montecarlo.GateFaultLists over b for b=None -- which describe_gate_faults() puts into words."""
        from . import montecarlo
        site_loc, n1, n2, _ = self.gate_sites()
        entry = self._entry("%s_gate_enumerate_list", host)
        run = lambda w, k, first, n, sel, capacity: entry(site_loc, n1, n2, w, k, first, n, sel, capacity)
        return montecarlo.malignant_gate_faults(n1, n2, weight, b, self.class_names, self.flip_mask if select is None else select,
                                                first_rank, count, max_configurations, self.noun, run)

    def describe_gate_faults(self, fault_list):
        """Every record of a GateFaultList of this gadget (or of every list of a GateFaultLists, b ascending) as a tuple over its
        picks of (gate index, gate (kind, a, b), qubits, Paulis): qubits the gate's operands -- one, or control then target -- and
        Paulis one letter per operand, gate_single_faults' format ('XI', 'ZY', ...)."""
        from . import montecarlo
        if isinstance(fault_list, montecarlo.GateFaultLists):
            return [record for part in fault_list for record in self.describe_gate_faults(part)]
        _, n1, n2, site_gate = self.gate_sites()
        if (fault_list.n1, fault_list.n2) != (n1, n2):
            raise ValueError("the list is over %d + %d sites, the gadget has %d + %d" % (fault_list.n1, fault_list.n2, n1, n2))

        def pick(g, kappa):
            gate = tuple(int(v) for v in self.gadget.gates[g])
            two = gate[0] == GATE_CNOT
            return (g, gate, (gate[1], gate[2]) if two else (gate[1],), PAULI_OF_MASK[kappa & 3] + (PAULI_OF_MASK[kappa >> 2] if two else ''))

        return [tuple(pick(g, k) for g, k in zip(gates, kinds))
                for gates, kinds in zip(fault_list.gates(site_gate).tolist(), fault_list.kinds().tolist())]

    def gate_strata(self, strata, samples, seed=0, first_sample=0, host=False):
        """Sampled strata under gate-level faults (DESIGN.md section 5e "Sampled strata under gate-level faults"): stratum s = (a, b)
        draws samples [first_sample, first_sample + samples[s]) of exactly a faulty one-operand gates and b faulty CNOTs, a + b <= 16,
        kinds uniform over the 3 and the 15, and judges them by the tally rule, post-selection included, tallied by the number c of
        two-operand kinds (gf2_mc_{ec,ft}_decode_gate_strata).  `samples` and `first_sample` are one number for all strata or one per
        stratum.  host=True draws with gf2_gate_stratum_outcomes_host and tallies with gf2_{ec,ft}_tally_host: no GPU.  Returns a
        montecarlo.SampledGateStrata."""
        from . import montecarlo
        sites = self.gate_sites()[:3]
        if host:
            run = montecarlo.host_gate_strata_run(self.effects, sites, self._tally, len(self.fields), seed)
        else:
            decode = self._entry("mc_%s_decode_gate_strata")
            run = lambda first, strata, ns: decode(*sites, int(seed), int(first), strata, ns)
        return montecarlo.gate_strata_local(sites[1], sites[2], self.fields, strata, samples, first_sample, run)

    def gate_error_rates(self, num_samples, p1, p2, seed=0, first_sample=0, host=False):
        """The direct Monte-Carlo under gate-level faults (DESIGN.md section 5e "Direct Monte-Carlo under gate-level faults"): in
        samples [first_sample, first_sample + num_samples) every one-operand gate fails with probability p1 and one of its 3 kinds,
        every CNOT as one event with probability p2 and one of its 15, and the tally rule judges them, post-selection included
        (gf2_mc_{ec,ft}_decode_gate).  host=True draws with gf2_gate_outcomes_host and tallies with gf2_{ec,ft}_tally_host: no GPU.
        Returns a dict of `fields` plus 'samples'; the counts of sample ranges add."""
        sites = self.gate_sites()[:3]
        if host:
            from . import montecarlo
            counts = montecarlo.host_gate_counts(self.effects, sites, self._tally, len(self.fields), num_samples, p1, p2, seed, first_sample)
        else:
            counts = self._entry("mc_%s_decode_gate")(*sites, int(seed), int(first_sample), int(num_samples), float(p1), float(p2))
        return self._dict(counts, num_samples)

    def _listed(self, classes):
        """The (row, column) pairs of a census' class bytes that are accepted and have a bit of flip_mask."""
        return zip(*np.nonzero((classes & CLASS_ACCEPTED != 0) & (classes & self.flip_mask != 0)))

    def gate_single_faults(self):
        """The census of every single gate fault, no GPU: (classes, listed) -- classes (G, 15) uint8, the class byte (CLASS_* bits)
        of kind mask kappa (column kappa - 1; a one-operand gate uses columns 0 .. 2, the others stay 0) at every gate of the list;
        listed, the accepted faults with a bit of flip_mask (a logical flip of the cycle, a wrong measured bit of the program) as
        (gate index, gate (kind, a, b), Paulis) with Paulis one letter for a one-operand gate and control then target, e.g. 'XI' or
        'ZY', for a CNOT."""
        site_loc, n1, n2, site_gate = self.gate_sites()
        eff = self.effects
        gates = self.gadget.gates
        classes = np.zeros((len(gates), 15), dtype=np.uint8)
        for sites, nbits in ((slice(0, n1), 2), (slice(n1, n1 + n2), 4)):
            locs = site_loc[sites].astype(np.int64)
            if not len(locs):
                continue
            words = np.zeros((len(locs), (1 << nbits) - 1, self.ldr), dtype=np.uint64)
            for kappa in range(1, 1 << nbits):
                for bit in range(nbits):
                    if (kappa >> bit) & 1:
                        words[:, kappa - 1] ^= eff[locs + (bit >> 1), bit & 1]
            _, cls = self.tally_host(words.reshape(-1, self.ldr), classes=True)
            classes[site_gate[sites], :(1 << nbits) - 1] = cls.reshape(len(locs), -1)
        listed = []
        for g, k in self._listed(classes):
            kappa = int(k) + 1
            gate = tuple(int(v) for v in gates[g])
            paulis = PAULI_OF_MASK[kappa & 3] + (PAULI_OF_MASK[kappa >> 2] if gate[0] == GATE_CNOT else '')
            listed.append((int(g), gate, paulis))
        return classes, listed

    def single_faults(self):
        """The census of all 3 L single faults, no GPU: (classes, listed) -- classes (L, 3) uint8, the class byte (CLASS_* bits)
        of an X, Y, Z fault (the columns, KINDS) at every location; listed, the accepted faults with a bit of flip_mask as
        (gate index, gate (kind, a, b), qubit, 'X' / 'Y' / 'Z')."""
        eff = self.effects
        words = np.stack((eff[:, 0], eff[:, 0] ^ eff[:, 1], eff[:, 1]), axis=1)              # X, Y, Z
        _, classes = self.tally_host(words.reshape(-1, self.ldr), classes=True)
        classes = classes.reshape(-1, 3)
        return classes, [self._fault(l, k) for l, k in self._listed(classes)]


class ECCircuit(Gadget):
    """The error-correction cycle of a code prepared for the Monte-Carlo: the gadget (error_correct_gates), its effect table
    (gf2_circuit_effects_timed, host code) and, on first use, the device copy.  The methods are Gadget's, with the cycle's tally
    rule (gf2_ec_tally_host, gf2_mc_ec_decode, ...), EC_FIELDS and this module's CLASS_* bits."""
    rule, fields, class_names, flip_mask, noun = _native.EC_RULE, EC_FIELDS, CLASS_NAMES, CLASS_FLIP_X | CLASS_FLIP_Z, "cycle"
    _create, _outcomes_dev = "circuit_create", "circuit_outcomes_dev"

    def __init__(self, code, rounds=1, idle_data=False):
        self.rounds = int(rounds)
        Gadget.__init__(self, code, error_correct_gates(code, rounds, idle_data))

    def _head(self):
        return (self.rounds,)

    def logical_error_rates(self, num_samples, p_x, p_y, p_z, seed=0, first_sample=0):
        """The tally of samples [first_sample, first_sample + num_samples) on the device (gf2_mc_ec_decode): a dict of EC_FIELDS plus
        'samples'.  Every field after 'accepted' counts among accepted samples; the counts of sample ranges add."""
        return self._error_rates(num_samples, p_x, p_y, p_z, seed, first_sample)


def circuit_for(code, rounds=1, idle_data=False):
    """ECCircuit(code, rounds, idle_data), cached on the code object."""
    cache = code.__dict__.setdefault("_ec_circuits", {})
    key = (int(rounds), bool(idle_data))
    if key not in cache:
        cache[key] = ECCircuit(code, rounds, idle_data)
    return cache[key]
