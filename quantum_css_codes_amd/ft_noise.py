"""
Fault Monte-Carlo of the fault-tolerant logical measurement [build-defined; DESIGN.md "Logical measurement"].

ec_noise.py says how often one error-correction gadget fails.  This module asks the question the reference's top-level workload
asks (test/test_fidelity.py): a one-qubit program -- logical Paulis, then MEASURE -- is rewritten by ftqc.rewrite_program
(ftqc.py:76-95) for a CSS code; how often is the measured bit wrong when every fault location of the rewritten program fails
independently with (p_x, p_y, p_z)?  And how often is the bare program's?

The gate list mirrors rewrite_program step for step, on ec_noise's registers (D = 0 .. n-1, A1 = n .. 2n-1, A2 = 2n .. 3n-1):
    prep(D, zero) verified by A1                                                      ftqc.py:78
    for each logical gate: its physical Paulis (one IDLE location each; I has none), then error_correct(D)   -- an EC step
    2t + 1 times (CSSCode.measure, css_code.py:542-589):
        prep(A1, zero) verified by A2; CNOT D[i] -> A1[i]; measure A1: parity_check_c2 (the key) and z_operator (the raw parity)
                                                                                       -- a MEASURE step (noisy_measure, :599-646)
        error_correct(D), after the last trial as well (measure yields after every trial)   -- an EC step
Every verification row of every prep is a flag row; a sample with a flag bit set is rejected (ec_noise's docstring: one attempt per
preparation and post-selection have the accepted attempts' distribution).

Outcome words: word s < nsteps is step s's (an EC step: key_x in bits 0 .. r_2-1, key_z in bits 32 .. 32+r_1-1; a MEASURE step:
key_x, and z_operator . e_x[A1] in bit 31), then F >= 1 flag words; ldr = nsteps + F <= 16.  The tally rule is
quil_classical_correct's (css_code.py:649-685) record of known errors run through the steps -- corrections and measurements share
data.x_errors -- and a majority vote over the trials; gf2_ft_tally_host is its serial form and gf2_mc_ft_decode the device kernel.

Only the Paulis are accepted.  A Clifford gate that moves the known-error registers (a logical H swaps the roles of x_errors and
z_errors, which the reference itself does not do) is a different model.
"""
import numpy as np

from . import _native
from . import circuit_noise
from . import ec_noise
from .ec_noise import GATE_IDLE, GATE_CNOT, ROW_FLAG, ROW_ROUND, KINDS
from .errors import UnsupportedProgramError

MAX_LDR = _native.FT_MAX_LDR
FT_FIELDS = ('accepted', 'wrong', 'trial_wrong', 'first_trial_wrong', 'split_vote', 'unmatched_x', 'unmatched_z')
CLASS_ACCEPTED, CLASS_WRONG, CLASS_FIRST_TRIAL_WRONG, CLASS_SPLIT_VOTE, CLASS_UNMATCHED_X, CLASS_UNMATCHED_Z = 1, 2, 4, 8, 16, 32
CLASS_NAMES = ('accepted', 'wrong', 'first_trial_wrong', 'split_vote', 'unmatched_x', 'unmatched_z')   # the class byte's bits, from bit 0
PAULIS = ('I', 'X', 'Y', 'Z')


class FTGates(ec_noise.ECGates):
    """What program_gates returns: an ECGates (rounds = the number of EC steps; row_round = 1 + the step of a row, 0 for the rows of
    the first preparation) plus `ops`, `nsteps`, `measure_mask` (bit s set: step s is a MEASURE step), `trials` and `pauli_gates`,
    the indices of the IDLE gates that stand for the physical Paulis of the logical gates."""


def check_ops(ops):
    """The logical gates as a tuple of 'I', 'X', 'Y', 'Z'; UnsupportedProgramError, naming the gate, for anything else."""
    ops = tuple(ops)
    for op in ops:
        if op not in PAULIS:
            raise UnsupportedProgramError("unsupported instruction: %r (the fault model takes the logical gates I, X, Y, Z on one "
                                          "qubit, then MEASURE)" % (op,))
    return ops


def logical_pauli_qubits(code, op):
    """The block qubits of the physical Paulis CSSCode.apply_gate emits for logical `op`, in emission order (css_code.py:386-409:
    the qubits of x_operators()[0], Y where z_operators()[0] acts too, then the qubits only the Z operator acts on)."""
    x_row = np.asarray(code.x_operator_matrix())[0] if op in ('X', 'Y') else np.zeros(code.n, dtype=int)
    z_row = np.asarray(code.z_operator_matrix())[0] if op in ('Z', 'Y') else np.zeros(code.n, dtype=int)
    return [q for q in range(code.n) if x_row[q]] + [q for q in range(code.n) if z_row[q] and not x_row[q]]


def program_gates(code, ops):
    """The gate list and timed outcome rows of the rewritten program `ops; MEASURE` (the module docstring has the order), one
    attempt per preparation.  Returns an FTGates."""
    ops = check_ops(ops)
    build = ec_noise.GadgetBuilder(code)
    trials = 2 * int(code.t) + 1
    nsteps = len(ops) + 2 * trials
    r_2, data, anc_1 = build.r_2, build.data, build.anc_1
    with build.span("prepare data"):
        build.prep(data, 'zero', 0, verifier=anc_1)                 # ftqc.py:78
    step, measure_mask, pauli_gates = 0, 0, []
    for op in ops:                                                  # ftqc.py:80-83
        with build.span("step %d: logical %s, EC" % (step, op)):
            with build.span("logical Pauli"):
                for q in logical_pauli_qubits(code, op):
                    pauli_gates.append(len(build.gates))
                    build.gates.append((GATE_IDLE, data[q], 0))
            build.error_correct(step + 1, step)
        step += 1
    for trial in range(trials):                                     # ftqc.py:84-89, css_code.py:576-579
        with build.span("step %d: MEASURE trial %d" % (step, trial)):
            build.prep(anc_1, 'zero', step + 1)                     # css_code.py:629
            with build.span("CNOT data -> ancilla"):
                build.gates.extend((GATE_CNOT, d, a) for d, a in zip(data, anc_1))
            build.measure(anc_1, np.concatenate([build.h_2, build.z_op[:1]]), ROW_ROUND, step + 1,
                          [64 * step + r_2 - 1 - i for i in range(r_2)] + [64 * step + 31])
        measure_mask |= 1 << step
        step += 1
        with build.span("step %d: EC after trial %d" % (step, trial)):
            build.error_correct(step + 1, step)
        step += 1
    assert step == nsteps
    flags = build.num_flags
    ldr = nsteps + max(1, (flags + 63) // 64)
    if ldr > MAX_LDR:
        raise ValueError("%d logical gates give %d steps and %d flag rows: %d outcome words per sample (ldr %d), more than %d"
                         % (len(ops), nsteps, flags, ldr, ldr, MAX_LDR))
    gates, rows_x, rows_z, row_time, row_kind, row_round, flag_rows = build.arrays(ldr, nsteps)
    out = FTGates(gates, 3 * build.n, nsteps - trials, ldr, rows_x, rows_z, row_time, row_kind, row_round, flag_rows, build.spans)
    out.ops, out.nsteps, out.measure_mask, out.trials, out.pauli_gates = ops, nsteps, measure_mask, trials, pauli_gates
    return out


def ops_of_quil(raw_prog):
    """The logical gates of a quil.Program of the accepted shape (DECLAREs; I, X, Y, Z on one qubit; one final MEASURE) as a tuple;
    UnsupportedProgramError, naming the instruction, for anything else."""
    ops, qubits, measured = [], set(), False
    for inst in raw_prog.instructions:
        if inst[0] == "DECLARE":
            continue
        if measured:
            raise UnsupportedProgramError("unsupported instruction after the final MEASURE: {}".format(inst))
        if inst[0] == "GATE" and inst[1] in PAULIS and len(inst[2]) == 1:
            qubits.add(inst[2][0])
            ops.append(inst[1])
        elif inst[0] == "MEASURE":
            qubits.add(inst[1])
            measured = True
        else:
            raise UnsupportedProgramError("unsupported instruction: {}".format(inst))
        if len(qubits) > 1:
            raise UnsupportedProgramError("unsupported instruction: {} (the fault model takes one logical qubit)".format(inst))
    if not measured:
        raise UnsupportedProgramError("unsupported program: it must end with a MEASURE")
    return tuple(ops)


class FTProgram(object):
    """The rewritten program `ops; MEASURE` of a code prepared for the Monte-Carlo: the gate list (program_gates), its effect table
    (gf2_circuit_effects_timed, host code) and, on first use, the device copy."""

    def __init__(self, code, ops):
        self.code = code
        self.gadget = program_gates(code, ops)
        self.ops, self.ldr, self.nsteps, self.measure_mask = self.gadget.ops, self.gadget.ldr, self.gadget.nsteps, self.gadget.measure_mask
        self.effects, self.locations = _native.circuit_effects_timed(
            self.gadget.gates, self.gadget.qubits, _native.pack_rows(self.gadget.rows_x), _native.pack_rows(self.gadget.rows_z),
            self.gadget.row_time, ldr=self.ldr)
        self._device = None
        self._sites = None

    @classmethod
    def from_quil(cls, raw_prog, code):
        """The model of ftqc.rewrite_program(raw_prog, code) for a quil.Program of the accepted shape (ops_of_quil)."""
        return cls(code, ops_of_quil(raw_prog))

    @property
    def num_locations(self):
        return len(self.locations)

    def device(self):
        if self._device is None:
            if not 1 <= self.num_locations <= circuit_noise.MAX_LOCATIONS:
                raise ValueError("the Monte-Carlo needs 1 <= L <= %d (2^20) fault locations, the program has %d"
                                 % (circuit_noise.MAX_LOCATIONS, self.num_locations))
            self._device = _native.default_context().ft_circuit_create(self.effects)
        return self._device

    def _tables(self):
        keys1, flips1, keys2, flips2 = circuit_noise.code_tables(self.code)
        return self.code.r_1, keys1, flips1, self.code.r_2, keys2, flips2

    def outcomes(self, num_samples, p_x, p_y, p_z, seed=0, first_sample=0):
        """The outcome words of samples [first_sample, first_sample + num_samples), rejected ones included: a (num_samples, ldr)
        uint64 array (gf2_ft_outcomes_dev)."""
        ctx = _native.default_context()
        circ = self.device()
        count = int(num_samples)
        buf = ctx.alloc(max(1, count) * self.ldr * 8)
        ctx.ft_outcomes_dev(circ, int(seed), int(first_sample), count, float(p_x), float(p_y), float(p_z), buf, self.ldr)
        out = buf.download((count, self.ldr), np.uint64)
        buf.free()
        return out

    def _dict(self, counts, samples):
        out = {name: int(v) for name, v in zip(FT_FIELDS, counts)}
        out['samples'] = int(samples)
        return out

    def measurement_error_rates(self, num_samples, p_x, p_y, p_z, seed=0, first_sample=0):
        """The tally of samples [first_sample, first_sample + num_samples) on the device (gf2_mc_ft_decode): a dict of FT_FIELDS
        plus 'samples'.  wrong / accepted estimates the probability that the rewritten program's measured bit is wrong.  Every
        field after 'accepted' counts among accepted samples; the counts of sample ranges add."""
        counts = _native.default_context().mc_ft_decode(self.device(), self.nsteps, self.measure_mask, *self._tables(), int(seed),
                                                        int(first_sample), int(num_samples), float(p_x), float(p_y), float(p_z))
        return self._dict(counts, num_samples)

    def tally_host(self, words, classes=False):
        """The tally rule over outcome words (samples, ldr) on the host (gf2_ft_tally_host, no GPU): the dict of FT_FIELDS plus
        'samples'; classes=True returns (dict, class byte per sample) instead."""
        words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, self.ldr)
        got = _native.ft_tally_host(words, self.nsteps, self.measure_mask, *self._tables(), classes=classes)
        out = self._dict(got[0] if classes else got, len(words))
        return (out, got[1]) if classes else out

    def enumerate_strata(self, weights, first_rank=None, count=None, max_configurations=None, host=False):
        """Exact strata of the measurement (DESIGN.md "Exact strata of the measurement"): every configuration of exactly
        weights[s] <= 8 faults of the rewritten program judged by measurement_error_rates' tally rule, post-selection included, and
        counted per kind composition.  Arguments as FaultCircuit.enumerate_strata's (ECCircuit.enumerate_strata has them in
        full); host=True runs gf2_ft_enumerate_host and needs no GPU.  Returns a montecarlo.PostSelectedStrata over nb = L."""
        from . import montecarlo
        weights, firsts, counts = circuit_noise.gadget_enumerate_request(self.num_locations, weights, first_rank, count, max_configurations,
                                                                         "program")
        if host:
            run = lambda w, f, n: _native.ft_enumerate_host(self.effects, self.nsteps, self.measure_mask, *self._tables(), w, f, n)
        else:
            ctx, circ = _native.default_context(), self.device()
            run = lambda w, f, n: ctx.ft_enumerate(circ, self.nsteps, self.measure_mask, *self._tables(), w, f, n)
        return montecarlo.PostSelectedStrata(self.num_locations, weights, [run(w, f, n) for w, f, n in zip(weights, firsts, counts)],
                                             FT_FIELDS)

    def malignant_faults(self, weight, select=CLASS_WRONG, first_rank=None, count=None, max_configurations=None, host=False):
        """The malignant fault sets of the measurement (DESIGN.md "Malignant fault sets of the measurement"): the accepted
        configurations of exactly `weight` <= 8 faults of the rewritten program whose class byte has a bit of `select` (CLASS_*
        bits), listed (gf2_ft_enumerate_list; host=True: gf2_ft_enumerate_list_host, no GPU).  Arguments and result as
        ECCircuit.malignant_faults': a montecarlo.FaultList over nb = L."""
        from . import montecarlo
        if host:
            run = lambda w, f, n, select, capacity: _native.ft_enumerate_list_host(self.effects, self.nsteps, self.measure_mask, *self._tables(),
                                                                                   w, f, n, select, capacity)
        else:
            ctx, circ = _native.default_context(), self.device()
            run = lambda w, f, n, select, capacity: ctx.ft_enumerate_list(circ, self.nsteps, self.measure_mask, *self._tables(), w, f, n,
                                                                          select, capacity)
        return montecarlo.malignant_faults(self.num_locations, weight, CLASS_NAMES, select, first_rank, count, max_configurations, "program", run)

    def describe(self, fault_list):
        """Every record of a FaultList of this program as a tuple over its picks of (gate index, gate (kind, a, b), qubit, 'X' / 'Y' /
        'Z'): single_faults' format, so the weight-1 list of the default select reads as single_faults()[1]."""
        return ec_noise.describe_faults(self, fault_list)

    def strata(self, weights, samples, kinds=(1, 1, 1), seed=0, first_sample=0, host=False):
        """Sampled strata of the measurement (DESIGN.md "Sampled strata of the measurement"): stratum s draws samples [first_sample,
        first_sample + samples[s]) of exactly weights[s] <= 16 faults among the L locations of the rewritten program, kinds X : Y : Z
        = kinds, judged by measurement_error_rates' tally rule, post-selection included (gf2_mc_ft_decode_strata).  Arguments as
        ECCircuit.strata's; host=True goes through gf2_stratum_outcomes_host and gf2_ft_tally_host and needs no GPU.  Returns a
        montecarlo.SampledPostSelectedStrata over nb = L."""
        from . import montecarlo
        tables = self._tables()
        if host:
            run = montecarlo.host_strata_run(self.effects, lambda words: _native.ft_tally_host(words, self.nsteps, self.measure_mask, *tables),
                                             len(FT_FIELDS), seed)
        else:
            ctx, circ = _native.default_context(), self.device()
            run = lambda first, ws, ns, ks: ctx.mc_ft_decode_strata(circ, self.nsteps, self.measure_mask, *tables, int(seed), int(first), ws, ns, *ks)
        return montecarlo.gadget_strata_local(self.num_locations, FT_FIELDS, weights, samples, kinds, first_sample, run)

    def gate_sites(self):
        """(site_loc, n1, n2, site_gate) of the program's gates (circuit_noise.gate_sites), made once."""
        if self._sites is None:
            self._sites = circuit_noise.gate_sites(self.gadget.gates, self.locations)
        return self._sites

    def enumerate_gate_range(self, w, b, first_rank, count, host=False):
        """One call of the gate-fault enumeration: the (b + 1, 7) uint64 counts [c][field] over the site
        subsets of ranks [first_rank, first_rank + count) of weight w with b CNOT picks, c the number of two-operand kinds
        (gf2_ft_gate_enumerate; host=True: gf2_ft_gate_enumerate_host, no GPU).  Counts of disjoint ranges add."""
        sites = self.gate_sites()[:3]
        if host:
            return _native.ft_gate_enumerate_host(self.effects, self.nsteps, self.measure_mask, *self._tables(), *sites, w, b, first_rank, count)
        return _native.default_context().ft_gate_enumerate(self.device(), self.nsteps, self.measure_mask, *self._tables(), *sites, w, b,
                                                           first_rank, count)

    def enumerate_gate_strata(self, weights, max_configurations=None, host=False):
        """Exact strata of the measurement under gate-level faults: every configuration of exactly
        weights[s] <= 4 faulty gates of the rewritten program judged by measurement_error_rates' tally rule, post-selection
        included, whole strata, every CNOT count b.  Arguments as ECCircuit.enumerate_gate_strata's.  Returns a montecarlo.GateStrata."""
        return ec_noise.gate_strata(self, FT_FIELDS, weights, max_configurations, host, "program")

    def gate_strata(self, strata, samples, seed=0, first_sample=0, host=False):
        """Sampled strata of the measurement under gate-level faults (DESIGN.md section 5e "Sampled strata under gate-level faults"):
        stratum s = (a, b) draws samples of exactly a faulty one-operand gates and b faulty CNOTs of the rewritten program, a + b <= 16,
        judged by measurement_error_rates' tally rule, post-selection included, tallied by the number c of two-operand kinds
        (gf2_mc_ft_decode_gate_strata).  Arguments as ECCircuit.gate_strata's; host=True goes through gf2_gate_stratum_outcomes_host
        and gf2_ft_tally_host and needs no GPU.  Returns a montecarlo.SampledGateStrata."""
        from . import montecarlo
        tables, sites = self._tables(), self.gate_sites()[:3]
        if host:
            run = montecarlo.host_gate_strata_run(self.effects, sites,
                                                  lambda words: _native.ft_tally_host(words, self.nsteps, self.measure_mask, *tables),
                                                  len(FT_FIELDS), seed)
        else:
            ctx, circ = _native.default_context(), self.device()
            run = lambda first, strata, ns: ctx.mc_ft_decode_gate_strata(circ, self.nsteps, self.measure_mask, *tables, *sites, int(seed),
                                                                         int(first), strata, ns)
        return montecarlo.gate_strata_local(sites[1], sites[2], FT_FIELDS, strata, samples, first_sample, run)

    def gate_error_rates(self, num_samples, p1, p2, seed=0, first_sample=0, host=False):
        """The direct Monte-Carlo of the measurement under gate-level faults (DESIGN.md section 5e "Direct Monte-Carlo under
        gate-level faults"): every one-operand gate of the rewritten program fails with probability p1, every CNOT as one event with
        probability p2, judged by measurement_error_rates' tally rule, post-selection included (gf2_mc_ft_decode_gate).  Arguments as
        ECCircuit.gate_error_rates'; host=True goes through gf2_gate_outcomes_host and gf2_ft_tally_host and needs no GPU.  Returns a
        dict of FT_FIELDS plus 'samples'."""
        tables, sites = self._tables(), self.gate_sites()[:3]
        if host:
            from . import montecarlo
            counts = montecarlo.host_gate_counts(self.effects, sites,
                                                 lambda words: _native.ft_tally_host(words, self.nsteps, self.measure_mask, *tables),
                                                 len(FT_FIELDS), num_samples, p1, p2, seed, first_sample)
        else:
            counts = _native.default_context().mc_ft_decode_gate(self.device(), self.nsteps, self.measure_mask, *tables, *sites, int(seed),
                                                                 int(first_sample), int(num_samples), float(p1), float(p2))
        return self._dict(counts, num_samples)

    def gate_single_faults(self):
        """The census of every single gate fault, no GPU: (classes, wrong) -- classes (G, 15) uint8, the class byte (CLASS_* bits) of
        kind mask kappa (column kappa - 1; a one-operand gate uses columns 0 .. 2) at every gate of the list; wrong, the accepted
        faults that make the measured bit wrong, as (gate index, gate (kind, a, b), Paulis) in ECCircuit.gate_single_faults' format."""
        return ec_noise.gate_single_faults(self, CLASS_WRONG)

    def single_faults(self):
        """The census of all 3 L single faults, no GPU: (classes, wrong) -- classes (L, 3) uint8, the class byte (CLASS_* bits) of
        an X, Y, Z fault (the columns, KINDS) at every location; wrong, the accepted faults that make the measured bit wrong, as
        (gate index, gate (kind, a, b), qubit, 'X' / 'Y' / 'Z')."""
        eff = self.effects
        words = np.stack((eff[:, 0], eff[:, 0] ^ eff[:, 1], eff[:, 1]), axis=1)              # X, Y, Z
        _, classes = self.tally_host(words.reshape(-1, self.ldr), classes=True)
        classes = classes.reshape(-1, 3)
        wrong = []
        for l, k in zip(*np.nonzero((classes & CLASS_ACCEPTED != 0) & (classes & CLASS_WRONG != 0))):
            g, q = (int(v) for v in self.locations[l])
            wrong.append((g, tuple(int(v) for v in self.gadget.gates[g]), q, KINDS[k]))
        return classes, wrong


def program_for(code, ops):
    """FTProgram(code, ops), cached on the code object."""
    cache = code.__dict__.setdefault("_ft_programs", {})
    key = check_ops(ops)
    if key not in cache:
        cache[key] = FTProgram(code, key)
    return cache[key]


def raw_program_error_rate(ops, p_x, p_y, p_z):
    """The probability that the bare program `ops; MEASURE` on one physical qubit gives the wrong bit under the same fault model: one
    location per gate other than I plus one before the measurement, the bit wrong iff an odd number of them carry an X or a Y:
    (1 - (1 - 2 (p_x + p_y))^m) / 2 for m locations.  p_z does not enter: a Z fault does not flip a Z measurement."""
    m = sum(1 for op in check_ops(ops) if op != 'I') + 1
    return 0.5 * (1.0 - (1.0 - 2.0 * (float(p_x) + float(p_y))) ** m)
