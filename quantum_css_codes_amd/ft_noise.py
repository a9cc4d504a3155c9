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
z_errors, which the reference itself does not do) is a different model.  Programs on several logical qubits with the transversal
CNOT are stream_noise.MultiProgram's; check_instructions, instructions_of_quil and raw_circuit_error_rate here are its program
checker, its quil front end and the bare program's side of its comparison.
"""
import numpy as np

from . import _native
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


class FTProgram(ec_noise.Gadget):
    """The rewritten program `ops; MEASURE` of a code prepared for the Monte-Carlo: the gate list (program_gates), its effect table
    (gf2_circuit_effects_timed, host code, up to MAX_LDR words) and, on first use, the device copy.  The methods are ec_noise.Gadget's,
    with the measurement's tally rule (gf2_ft_tally_host, gf2_mc_ft_decode, ...), FT_FIELDS and this module's CLASS_* bits: what
    single_faults and gate_single_faults list are the accepted faults that make the measured bit wrong."""
    rule, fields, class_names, flip_mask, noun = _native.FT_RULE, FT_FIELDS, CLASS_NAMES, CLASS_WRONG, "program"
    _create, _outcomes_dev = "ft_circuit_create", "ft_outcomes_dev"

    def __init__(self, code, ops):
        gadget = program_gates(code, ops)
        self.ops, self.nsteps, self.measure_mask = gadget.ops, gadget.nsteps, gadget.measure_mask
        ec_noise.Gadget.__init__(self, code, gadget)

    @classmethod
    def from_quil(cls, raw_prog, code):
        """The model of ftqc.rewrite_program(raw_prog, code) for a quil.Program of the accepted shape (ops_of_quil)."""
        return cls(code, ops_of_quil(raw_prog))

    def _head(self):
        return self.nsteps, self.measure_mask

    def measurement_error_rates(self, num_samples, p_x, p_y, p_z, seed=0, first_sample=0):
        """The tally of samples [first_sample, first_sample + num_samples) on the device (gf2_mc_ft_decode): a dict of FT_FIELDS
        plus 'samples'.  wrong / accepted estimates the probability that the rewritten program's measured bit is wrong.  Every
        field after 'accepted' counts among accepted samples; the counts of sample ranges add."""
        return self._error_rates(num_samples, p_x, p_y, p_z, seed, first_sample)


def program_for(code, ops):
    """FTProgram(code, ops), cached on the code object."""
    cache = code.__dict__.setdefault("_ft_programs", {})
    key = check_ops(ops)
    if key not in cache:
        cache[key] = FTProgram(code, key)
    return cache[key]


MAX_LOGICAL_QUBITS = _native.MSTREAM_MAX_FRAMES


def check_instructions(instructions):
    """The instructions of a multi-qubit program (stream_noise.MultiProgram) as a tuple of ('I' | 'X' | 'Y' | 'Z', q), ('CNOT', a, b)
    with a != b and ('MEASURE', q), and the sorted qubit indices that appear: gates first, then one or more MEASUREs on distinct
    qubits and nothing after them, 1 <= Q <= MAX_LOGICAL_QUBITS qubits.  UnsupportedProgramError, naming the instruction, for
    anything else."""
    out, measured, qubits = [], [], set()
    index = lambda q: isinstance(q, (int, np.integer)) and not isinstance(q, bool) and q >= 0
    for inst in instructions:
        inst = tuple(inst) if isinstance(inst, (tuple, list)) else (inst,)
        name, operands = (inst[0], inst[1:]) if inst else (None, ())
        if name in PAULIS and len(operands) == 1 and index(operands[0]):
            shape = "gate"
        elif name == 'CNOT' and len(operands) == 2 and index(operands[0]) and index(operands[1]) and operands[0] != operands[1]:
            shape = "gate"
        elif name == 'MEASURE' and len(operands) == 1 and index(operands[0]):
            shape = "measure"
        else:
            raise UnsupportedProgramError("unsupported instruction: %r (the fault model takes the logical gates I, X, Y, Z and CNOT on "
                                          "distinct qubits, then MEASUREs)" % (inst,))
        if shape == "gate" and measured:
            raise UnsupportedProgramError("unsupported instruction after a MEASURE: %r" % (inst,))
        if shape == "measure":
            if int(operands[0]) in measured:
                raise UnsupportedProgramError("unsupported instruction: %r (qubit %d is measured twice)" % (inst, operands[0]))
            measured.append(int(operands[0]))
        qubits.update(int(q) for q in operands)
        if len(qubits) > MAX_LOGICAL_QUBITS:
            raise UnsupportedProgramError("unsupported instruction: %r (the fault model takes at most %d logical qubits)"
                                          % (inst, MAX_LOGICAL_QUBITS))
        out.append((name,) + tuple(int(q) for q in operands))
    if not measured:
        raise UnsupportedProgramError("unsupported program: it must end with a MEASURE")
    return tuple(out), sorted(qubits)


def instructions_of_quil(raw_prog):
    """The instructions of a quil.Program of the accepted shape (DECLAREs; I, X, Y, Z and CNOT; then MEASUREs) as check_instructions
    takes them; UnsupportedProgramError, naming the instruction, for anything else."""
    out = []
    for inst in raw_prog.instructions:
        if inst[0] == "DECLARE":
            continue
        if inst[0] == "GATE" and (inst[1] in PAULIS or inst[1] == "CNOT") and all(isinstance(q, (int, np.integer)) for q in inst[2]):
            out.append((inst[1],) + tuple(inst[2]))
        elif inst[0] == "MEASURE" and isinstance(inst[1], (int, np.integer)):
            out.append(("MEASURE", inst[1]))
        else:
            raise UnsupportedProgramError("unsupported instruction: {}".format(inst))
    return check_instructions(out)[0]


def raw_circuit_error_rate(instructions, p_x, p_y, p_z):
    """Per MEASURE of the bare program, in program order, the probability that its bit is wrong under the same fault model:
    raw_program_error_rate with one location per Pauli other than I, one per operand of a CNOT (a fault follows its gate) and one
    before every measurement.  An X component copies from control to target through every later CNOT; the bit is wrong iff an odd
    number of the m locations whose X component reaches the measured qubit carry an X or a Y: (1 - (1 - 2 (p_x + p_y))^m) / 2.  p_z
    does not enter."""
    instructions, qubits = check_instructions(instructions)
    reach = {q: set() for q in qubits}                              # the locations whose X component sits on q, modulo 2
    locations, out = 0, []
    for inst in instructions:
        if inst[0] == 'CNOT':
            a, b = inst[1:]
            reach[b] ^= reach[a]
            reach[a] ^= {locations}
            reach[b] ^= {locations + 1}
            locations += 2
        elif inst[0] == 'MEASURE':
            out.append(0.5 * (1.0 - (1.0 - 2.0 * (float(p_x) + float(p_y))) ** (len(reach[inst[1]]) + 1)))
            locations += 1
        elif inst[0] != 'I':
            reach[inst[1]] ^= {locations}
            locations += 1
    return out


def raw_circuit_gate_error_rate(instructions, p1, p2):
    """raw_circuit_error_rate under gate-level faults: a Pauli other than I and a measurement are one-operand
    locations that fail with probability p1 and one of 3 Paulis, a CNOT fails as one event with probability p2 and one of the 15
    two-qubit Paulis (a fault follows its gate).  With raw_circuit_error_rate's reach sets, a one-operand fault that reaches the
    measured qubit flips the bit for 2 of its 3 kinds; a CNOT event of which at least one operand reaches it flips the bit when
    the XOR of the reaching operands' X components is 1, which holds for 8 of the 15 kinds whether one operand reaches or both.
    The events are independent, so per MEASURE in program order the bit is wrong with probability
    (1 - (1 - 4 p1 / 3)^m1 (1 - 16 p2 / 15)^m2) / 2, m1 the reaching one-operand locations with the measurement's own, m2 the
    CNOTs with a reaching operand."""
    instructions, qubits = check_instructions(instructions)
    reach = {q: set() for q in qubits}                              # raw_circuit_error_rate's, with its location numbers
    locations, out, cnot_of = 0, [], {}                             # a CNOT operand's location -> its CNOT's first location
    for inst in instructions:
        if inst[0] == 'CNOT':
            a, b = inst[1:]
            reach[b] ^= reach[a]
            reach[a] ^= {locations}
            reach[b] ^= {locations + 1}
            cnot_of[locations] = cnot_of[locations + 1] = locations
            locations += 2
        elif inst[0] == 'MEASURE':
            mine = reach[inst[1]]
            m_1 = sum(1 for l in mine if l not in cnot_of) + 1
            m_2 = len({cnot_of[l] for l in mine if l in cnot_of})
            out.append(0.5 * (1.0 - (1.0 - 4.0 * float(p1) / 3.0) ** m_1 * (1.0 - 16.0 * float(p2) / 15.0) ** m_2))
            locations += 1
        elif inst[0] != 'I':
            reach[inst[1]] ^= {locations}
            locations += 1
    return out


def raw_program_error_rate(ops, p_x, p_y, p_z):
    """The probability that the bare program `ops; MEASURE` on one physical qubit gives the wrong bit under the same fault model: one
    location per gate other than I plus one before the measurement, the bit wrong iff an odd number of them carry an X or a Y:
    (1 - (1 - 2 (p_x + p_y))^m) / 2 for m locations.  p_z does not enter: a Z fault does not flip a Z measurement."""
    m = sum(1 for op in check_ops(ops) if op != 'I') + 1
    return 0.5 * (1.0 - (1.0 - 2.0 * (float(p_x) + float(p_y))) ** m)
