"""
The fault-tolerant logical measurement on the CPU (DESIGN.md section 5c "Logical measurement"): ft_noise.program_gates / FTProgram,
gf2_ft_tally_host (csrc/gf2_host.cpp).  Every comparison is exact.

  builder         gates, rows and times against tests/ft_ref.py, written from the reference's line numbers, and against the quantum
                  instructions ftqc.rewrite_program emits for the same program (one pass through every loop body)
  effect table    against forward propagation (ec_ref's primitive) for every single fault and seeded random multi-fault sets
  tally           gf2_ft_tally_host against ft_ref's tally on vectors of known errors; refusals; the census
  raw program     the closed form against brute-force enumeration
  end to end      ftqc.rewrite_program of X X X MEASURE for the Steane code, executed by oracle/quil_sim.py with injected faults: ro[0]
                  is wrong exactly when the tally says accepted and wrong
"""
import functools
import itertools

import numpy as np
import pytest

from oracle import cpu_ref, quil_sim
from quantum_css_codes_amd import _native, ft_noise, ftqc
from quantum_css_codes_amd.errors import UnsupportedProgramError
from quantum_css_codes_amd.quil import Program, gates
from tests import ft_ref
from tests.ec_ref import CNOT, H, IDLE, RESET
from tests.test_quil_emission import OracleCode

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
FIELDS = ft_noise.FT_FIELDS
PROGRAMS = [("steane", ""), ("steane", "XXX"), ("steane", "XYZIZYX"), ("rm15", "")]


def rm15_checks():
    cols = np.arange(1, 16)
    h1 = np.array([(cols >> b) & 1 for b in range(4)])
    return h1, np.vstack([h1] + [h1[a] & h1[b] for a in range(4) for b in range(a + 1, 4)])


@functools.lru_cache(maxsize=None)
def oracle_code(name):
    return cpu_ref.CSSCode(STEANE, STEANE) if name == "steane" else cpu_ref.CSSCode(*rm15_checks())


@functools.lru_cache(maxsize=None)
def program(name, ops):
    """(FTProgram, ft_ref.Rewritten) of an oracle code: nothing here needs a GPU."""
    code = oracle_code(name)
    return ft_noise.FTProgram(code, ops), ft_ref.Rewritten(code, ops)


def unpack(eff, rows):
    flat = np.ascontiguousarray(eff).reshape(-1, eff.shape[-1])
    return _native.unpack_rows(flat, rows, dtype=np.uint8).reshape(eff.shape[:-1] + (rows,))


# ---- the builder ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, ops", PROGRAMS)
def test_builder_equals_the_restatement(name, ops):
    prog, ref = program(name, ops)
    got = prog.gadget
    assert got.gates.tolist() == ref.gates.tolist()
    assert (got.qubits, got.ldr, got.nsteps, got.measure_mask) == (3 * prog.code.n, ref.ldr, ref.nsteps, ref.measure_mask)
    assert np.array_equal(got.rows_x, ref.rows_x) and np.array_equal(got.rows_z, ref.rows_z)
    assert np.array_equal(got.row_time, ref.row_time)
    assert np.array_equal(got.row_kind != 0, ref.row_kind != 0)
    assert got.flag_rows.tolist() == np.flatnonzero(ref.row_kind == ft_ref.FLAG).tolist()
    assert bin(got.measure_mask).count("1") == got.trials == 2 * prog.code.t + 1
    assert [got.gates[g].tolist() for g in got.pauli_gates] == [[IDLE, q, 0] for op in ops for q in ft_ref.pauli_qubits(prog.code, op)]


def test_limits_table():
    # (code, k, gates, L, rows, flag rows, ldr): DESIGN.md section 5c; the Steane flag rows are 7 + 14 k + 63
    want = {0: (1094, 1585, 100, 70, 8), 1: (1325, 1918, 120, 84, 9), 2: (1556, 2251, 140, 98, 10), 3: (1787, 2584, 160, 112, 11),
            4: (2018, 2917, 180, 126, 12), 5: (2249, 3250, 200, 140, 14), 6: (2480, 3583, 220, 154, 15), 7: (2711, 3916, 240, 168, 16)}
    for k, row in want.items():
        g = ft_noise.program_gates(oracle_code("steane"), "X" * k)
        assert (len(g.gates), int(len(g.gates) + np.count_nonzero(g.gates[:, 0] == CNOT)), g.num_rows, len(g.flag_rows), g.ldr) == row
        assert g.nsteps == k + 6 and len(g.flag_rows) == 7 + 14 * k + 63
    prog, ref = program("rm15", "")
    assert (len(prog.gadget.gates), prog.num_locations, prog.gadget.num_rows, len(prog.gadget.flag_rows), prog.ldr) == (2538, 3867, 225, 150, 9)
    assert program("steane", "XXX")[0].effects.nbytes == 2584 * 2 * 11 * 8               # about 455 KB


def quantum_events(new_prog):
    """The quantum instructions of a rewritten program as (pc, kind, a, b) in program text order -- one pass through every loop
    body.  A MEASURE into a block's register is a reset (qecc.py:35-49), one into a scratch register a measurement; the X of a reset's
    if_then (JUMP-WHEN, JUMP, LABEL, X, LABEL) and the instructions that only initialise memory (before the first loop, and the
    superfluous MEASURE into ro, css_code.py:584-586) are no events."""
    insts = new_prog.instructions
    first_loop = next(pc for pc, inst in enumerate(insts) if inst[0] == "LABEL")
    events = []
    for pc in range(first_loop, len(insts)):
        inst = insts[pc]
        if inst[0] == "MEASURE":
            if inst[2].name in ("logical_qubit_0", "ancilla_1", "ancilla_2"):
                events.append((pc, RESET, inst[1], 0))
            elif inst[2].name != "ro":
                events.append((pc, IDLE, inst[1], 0))
        elif inst[0] == "GATE":
            name, qubits = inst[1], inst[2]
            if name in ("X", "Y", "Z"):
                if not (name == "X" and insts[pc - 3][0] == "JUMP-WHEN" and insts[pc - 1][0] == "LABEL" and insts[pc + 1][0] == "LABEL"):
                    events.append((pc, IDLE, qubits[0], 0))
            elif name == "H":
                events.append((pc, H, qubits[0], 0))
            else:
                assert name == "CNOT", name
                events.append((pc, CNOT, qubits[0], qubits[1]))
    return events


def raw_program(ops):
    raw = Program()
    ro = raw.declare('ro', 'BIT', 1)
    raw += (getattr(gates, op)(0) for op in ops)
    raw += gates.MEASURE(0, ro[0])
    return raw


@pytest.mark.parametrize("ops", ["", "XXX", "XYZIZYX"])
def test_builder_equals_the_emitted_program(ops):
    steane = OracleCode(STEANE, STEANE)
    new_prog = ftqc.rewrite_program(raw_program(ops), steane)
    events = quantum_events(new_prog)
    got = ft_noise.program_gates(oracle_code("steane"), ops)
    # every gate of the model is one quantum instruction: RESET a reset's MEASURE, a measurement's IDLE its MEASURE, a logical
    # Pauli's IDLE its X / Y / Z, in the same order on the same qubits (D, A1, A2 are addressed 0 .. 3n - 1 in this order)
    assert [list(e[1:]) for e in events] == got.gates.tolist()
    paulis = [new_prog.instructions[events[g][0]][1] for g in got.pauli_gates]
    code = oracle_code("steane")
    x_row, z_row = code.x_operator_matrix()[0], code.z_operator_matrix()[0]
    name = lambda op, q: "Y" if op == "Y" and x_row[q] and z_row[q] else "X" if op != "Z" and x_row[q] else "Z"
    assert paulis == [name(op, q) for op in ops for q in ft_ref.pauli_qubits(code, op)]
    assert ft_noise.FTProgram.from_quil(raw_program(ops), oracle_code("steane")).gadget.gates.tolist() == got.gates.tolist()


# ---- the effect table ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, ops", PROGRAMS)
def test_effects_equal_forward_propagation(name, ops):
    prog, ref = program(name, ops)
    total, rows = prog.num_locations, 64 * prog.ldr
    assert total == ref.locations and prog.effects.shape == (total, 2, ref.ldr)
    want_locs = [(g, q) for g, (kind, a, b) in enumerate(ref.gates.tolist()) for q in ((a, b) if kind == CNOT else (a,))]
    assert prog.locations.tolist() == [list(v) for v in want_locs]
    ident, zero = np.identity(total, dtype=np.uint8), np.zeros((total, total), dtype=np.uint8)
    assert np.array_equal(prog.effects[:, 0], ref.outcome_words(ident, zero)), "X"
    assert np.array_equal(prog.effects[:, 1], ref.outcome_words(zero, ident)), "Z"
    rng = np.random.default_rng(len(ops) + total)
    f_x = (rng.random((total, 300)) < 3.0 / total).astype(np.uint8)                # 300 multi-fault sets, about six faults each
    f_z = (rng.random((total, 300)) < 3.0 / total).astype(np.uint8)
    assert (f_x | f_z).sum(axis=0).max() >= 8
    bits = unpack(prog.effects, rows)
    # (float32 products of 0/1 entries over a few thousand locations are exact)
    got = (f_x.T.astype(np.float32) @ bits[:, 0].astype(np.float32) + f_z.T.astype(np.float32) @ bits[:, 1].astype(np.float32)).astype(np.int64) & 1
    assert np.array_equal(ft_ref.pack_words(got.astype(np.uint8)), ref.outcome_words(f_x, f_z))
    # nothing outside the layout: an EC step's key bits, a MEASURE step's key bits and bit 31, the flag words
    code, any_word = prog.code, np.bitwise_or.reduce(prog.effects.reshape(-1, prog.ldr), axis=0).tolist()
    for s in range(prog.nsteps):
        allowed = ((1 << code.r_2) - 1) | ((1 << 31) if (prog.measure_mask >> s) & 1 else ((1 << code.r_1) - 1) << 32)
        assert any_word[s] & ~allowed == 0 and any_word[s] != 0


# ---- the tally -----------------------------------------------------------------------------------------------------------------

def random_words(rng, code, nsteps, measure_mask, ldr, count):
    """Outcome words that meet every branch: most accepted, quiet keys and arbitrary ones, raw parities, some rejected through the
    first flag word only, some through the last only."""
    words = np.zeros((count, ldr), dtype=np.uint64)
    key_x = rng.integers(0, 1 << code.r_2, (count, nsteps), dtype=np.uint64)
    key_z = rng.integers(0, 1 << code.r_1, (count, nsteps), dtype=np.uint64)
    quiet = rng.random((count, nsteps)) < 0.75
    key_x[quiet], key_z[quiet] = 0, 0
    parity = (rng.random((count, nsteps)) < 0.15).astype(np.uint64)
    for s in range(nsteps):
        measure = (measure_mask >> s) & 1
        words[:, s] = key_x[:, s] | (parity[:, s] << np.uint64(31) if measure else key_z[:, s] << np.uint64(32))
    pick = rng.random(count)
    words[pick < 0.1, nsteps] = rng.integers(1, 1 << 62, int((pick < 0.1).sum()), dtype=np.uint64)
    last = (pick >= 0.1) & (pick < 0.2)
    words[last, ldr - 1] = np.uint64(1) << rng.integers(0, 64, int(last.sum()), dtype=np.uint64)
    return words


@pytest.mark.parametrize("name, ops", PROGRAMS)
def test_tally_host_equals_the_restatement(name, ops):
    prog, ref = program(name, ops)
    words = random_words(np.random.default_rng(len(ops) + 1), prog.code, prog.nsteps, prog.measure_mask, prog.ldr, 4000)
    if prog.ldr - prog.nsteps >= 2:
        assert np.any((words[:, prog.nsteps] == 0) & (words[:, prog.ldr - 1] != 0))   # rejected by the last flag word only
    got, classes = prog.tally_host(words, classes=True)
    want, want_classes = ref.tally(words)
    print("\n%s %r: %s" % (name, ops, dict(zip(FIELDS, want))))
    assert [got[f] for f in FIELDS] == want and got['samples'] == 4000
    assert np.array_equal(classes, want_classes)
    assert [prog.tally_host(words)[f] for f in FIELDS] == want
    # accepted, rejected, wrong, right, split and (where the table is not perfect: rm15's key_x) unmatched samples all occur
    assert 0 < got['accepted'] < 4000 and 0 < got['wrong'] < got['accepted'] and got['split_vote'] > 0
    assert got['first_trial_wrong'] > 0 and got['trial_wrong'] > got['wrong']
    assert np.any(classes & 0x0b == 0x03) and np.any(classes & 0x0b == 0x09)       # wrong and unanimous; right although split
    if name == "rm15":
        assert got['unmatched_x'] > 0


def test_tally_host_with_unmatched_keys_on_both_sides():
    # the tally needs only tables and steps: random full-rank checks of 5 and 6 rows on 9 bits with tables that hold a part of the
    # keys miss on both sides (the test codes' C1 tables are perfect), every entry the lowest vector with its key as its syndrome
    # (the restatement recomputes the syndrome of the known errors from the check matrix, the library from the keys); the steps are
    # not the builder's: EC and MEASURE in any order, one to five trials
    rng = np.random.default_rng(7)
    vectors = np.array(list(itertools.product((0, 1), repeat=9)))

    def side(r, entries):
        while True:
            check = rng.integers(0, 2, (r, 9))
            keys = np.array([cpu_ref.vec_to_int(v) for v in (vectors @ check.T) % 2])
            if len(set(keys.tolist())) == 1 << r:                      # full rank
                break
        table = {int(k): vectors[np.flatnonzero(keys == k)[0]] for k in rng.choice(1 << r, entries, replace=False)}
        return check, table

    class Tables(object):
        n, r_1, r_2 = 9, 5, 6
        x_op, z_op = rng.integers(0, 2, (1, 9)), rng.integers(0, 2, (1, 9))
        x_operator_matrix = lambda self: self.x_op
        z_operator_matrix = lambda self: self.z_op

    code = Tables()
    (code.parity_check_c1, code._c1_syndromes), (code.parity_check_c2, code._c2_syndromes) = side(5, 12), side(6, 20)
    keys1 = np.array(list(code._c1_syndromes), dtype=np.uint64)
    flips1 = np.array([int(code.x_op[0] @ v) & 1 for v in code._c1_syndromes.values()], dtype=np.uint8)
    keys2 = np.array(list(code._c2_syndromes), dtype=np.uint64)
    flips2 = np.array([int(code.z_op[0] @ v) & 1 for v in code._c2_syndromes.values()], dtype=np.uint8)
    for steps in ([ft_ref.MEASURE], [ft_ref.EC, ft_ref.MEASURE, ft_ref.MEASURE, ft_ref.EC, ft_ref.MEASURE],
                  [ft_ref.MEASURE, ft_ref.EC] * 5 + [ft_ref.EC] * 4):
        nsteps, ldr = len(steps), len(steps) + 2
        mask = sum(1 << s for s, kind in enumerate(steps) if kind == ft_ref.MEASURE)
        words = random_words(rng, code, nsteps, mask, ldr, 3000)
        counts, classes = _native.ft_tally_host(words, nsteps, mask, 5, keys1, flips1, 6, keys2, flips2, classes=True)
        want, want_classes = ft_ref.tally(code, steps, words)
        assert counts.tolist() == want and np.array_equal(classes, want_classes)
        assert want[5] > 0 and (want[6] > 0 or ft_ref.EC not in steps) and want[1] > 0 and (want[4] > 0 or nsteps == 1)
    # ldw > ldr: the words of a sample lie ldw apart
    wide = np.zeros((3000, ldr + 3), dtype=np.uint64)
    wide[:, :ldr], wide[:, ldr:] = words, 1
    assert _native.ft_tally_host(wide, nsteps, mask, 5, keys1, flips1, 6, keys2, flips2, ldr=ldr).tolist() == want


def test_single_fault_census():
    prog, ref = program("steane", "XXX")
    classes, wrong = prog.single_faults()
    total = prog.num_locations
    assert classes.shape == (total, 3)
    ident, zero = np.identity(total, dtype=np.uint8), np.zeros((total, total), dtype=np.uint8)
    for column, (f_x, f_z) in enumerate(((ident, zero), (ident, ident), (zero, ident))):      # X, Y, Z
        _, want = ref.tally(ref.outcome_words(f_x, f_z))
        assert np.array_equal(classes[:, column], want), "XYZ"[column]
    accepted = classes & 1 != 0
    where = list(zip(*np.nonzero(accepted & (classes & 2 != 0))))
    want_list = [(int(prog.locations[l, 0]), tuple(ref.gates[prog.locations[l, 0]].tolist()), int(prog.locations[l, 1]), "XYZ"[k]) for l, k in where]
    assert wrong == want_list and len(wrong) >= 1                    # the measurement is not strictly fault tolerant
    outvoted = accepted & (classes & 2 == 0) & (classes & 8 != 0)
    print("\nSteane XXX: %d single faults, %d accepted, %d of them make the result wrong, %d more flip a trial and are outvoted:"
          % (3 * total, accepted.sum(), len(wrong), outvoted.sum()))
    for (l, k), (g, gate, q, kind) in zip(where, wrong):
        print("  gate %d %r: %s on qubit %d -> class %#x" % (g, gate, kind, q, classes[l, k]))


def test_refusals():
    steane = oracle_code("steane")
    with pytest.raises(ValueError, match="ldr 17.*more than 16"):
        ft_noise.program_gates(steane, "X" * 8)
    assert ft_noise.program_gates(steane, "X" * 7).ldr == 16

    class Wide(object):
        n, r_1, r_2, t = 65, 32, 32, 1
    with pytest.raises(ValueError, match="r_1, r_2 <= 31"):
        ft_noise.program_gates(Wide(), "")
    for ops, text in (("XHX", "'H'"), (["X", "CNOT"], "'CNOT'"), ("XS", "'S'")):
        with pytest.raises(UnsupportedProgramError, match=text):
            ft_noise.program_gates(steane, ops)
    raw = Program()
    ro = raw.declare('ro', 'BIT', 2)
    for insts, text in (([gates.H(0), gates.MEASURE(0, ro[0])], "'H'"), ([gates.X(0), gates.X(1), gates.MEASURE(0, ro[0])], "one logical qubit"),
                        ([gates.X(0), gates.MEASURE(0, ro[0]), gates.X(0)], "after the final MEASURE"), ([gates.X(0)], "end with a MEASURE"),
                        ([gates.MEASURE(0, ro[0]), gates.MEASURE(0, ro[1])], "after the final MEASURE"),
                        ([gates.X(0), ("JUMP", "somewhere"), gates.MEASURE(0, ro[0])], "JUMP"), ([gates.CNOT(0, 1), gates.MEASURE(0, ro[0])], "CNOT")):
        with pytest.raises(UnsupportedProgramError, match=text):
            ft_noise.FTProgram.from_quil(Program(raw, insts), steane)
    prog, _ = program("steane", "XXX")
    _, keys1, flips1, _, keys2, flips2 = prog._tables()
    words = np.zeros((2, 17), dtype=np.uint64)
    #   nsteps, mask, r1, r2, ldr
    for nsteps, mask, r1, r2, ldr, text in ((9, 0b10101000, 32, 3, 11, "r_1, r_2 <= 31"), (9, 0b10101000, 3, 32, 11, "r_1, r_2 <= 31"),
                                            (9, 0b10101000, 3, 3, 17, "ldr <= 16"), (9, 0b00101000, 3, 3, 11, "odd number of trials"),
                                            (9, 0, 3, 3, 11, "odd number of trials"), (9, 0b1000101000, 3, 3, 11, "at or above nsteps"),
                                            (11, 0b10101000, 3, 3, 11, "F >= 1"), (0, 0, 3, 3, 11, "nsteps >= 1")):
        with pytest.raises(_native.GF2Error, match=text):
            _native.ft_tally_host(words, nsteps, mask, r1, keys1, flips1, r2, keys2, flips2, ldr=ldr)
    with pytest.raises(_native.GF2Error, match="occurs twice"):
        _native.ft_tally_host(words, 9, 0b10101000, 3, np.array([1, 1], dtype=np.uint64), np.zeros(2, np.uint8), 3, keys2, flips2, ldr=11)
    with pytest.raises(_native.GF2Error, match="ldw >= ldr"):
        _native.ft_tally_host(words[:, :10], 9, 0b10101000, 3, keys1, flips1, 3, keys2, flips2, ldr=11)
    empty = _native.ft_tally_host(np.zeros((0, 11), dtype=np.uint64), 9, 0b10101000, 3, keys1, flips1, 3, keys2, flips2)
    assert empty.tolist() == [0] * 7
    assert ft_noise.program_for(steane, "XXX") is ft_noise.program_for(steane, ("X", "X", "X"))


# ---- the bare program ----------------------------------------------------------------------------------------------------------

def test_raw_program_error_rate_equals_enumeration():
    for ops, (p_x, p_y, p_z) in itertools.product(("", "X", "XXX", "XIZY", "IIII"), ((0.01, 0.002, 0.03), (0.2, 0.1, 0.3), (0.0, 0.0, 0.5))):
        m = sum(op != 'I' for op in ops) + 1                           # one location per gate, one before the measurement
        want = 0.0
        for kinds in itertools.product("IXYZ", repeat=m):              # the bit is flipped by every X or Y
            weight = np.prod([{"I": 1 - p_x - p_y - p_z, "X": p_x, "Y": p_y, "Z": p_z}[k] for k in kinds])
            want += weight * (sum(k in "XY" for k in kinds) & 1)
        assert abs(ft_noise.raw_program_error_rate(ops, p_x, p_y, p_z) - want) < 1e-15
    assert ft_noise.raw_program_error_rate("XXX", 0.0, 0.0, 0.1) == 0.0
    with pytest.raises(UnsupportedProgramError):
        ft_noise.raw_program_error_rate("XH", 0.1, 0.0, 0.0)


# ---- end to end against the emitted program ------------------------------------------------------------------------------------

def injection(events, gadget, location):
    """The pc before which a fault at (gate, qubit) is injected: after its instruction for a gate or a logical Pauli; before its
    MEASURE for a measurement error; after the whole reset of its block (its next instruction that is no reset) for a RESET."""
    g = int(location[0])
    kind = int(gadget.gates[g, 0])
    if kind == RESET:
        return next(events[h][0] for h in range(g + 1, len(events)) if events[h][1] != RESET)
    if kind == IDLE and g not in gadget.pauli_gates:
        return events[g][0]
    return events[g][0] + 1


def test_emitted_program_gives_the_wrong_bit_exactly_when_the_tally_says_so():
    steane = OracleCode(STEANE, STEANE)
    new_prog = ftqc.rewrite_program(raw_program("XXX"), steane)
    events = quantum_events(new_prog)
    prog, _ = program("steane", "XXX")
    gadget, total = prog.gadget, prog.num_locations
    assert quil_sim.run(new_prog, seed=0)['ro'][0] == 1
    classes, wrong = prog.single_faults()
    rng = np.random.default_rng(31)
    marked = [(int(l), k) for l, k in zip(*np.nonzero((classes & 3) == 3))]
    others = [(int(l), int(k)) for l, k in zip(rng.integers(0, total, 100), rng.integers(0, 3, 100)) if (classes[l, k] & 3) != 3]
    pairs = [tuple((int(l), int(k)) for l, k in zip(rng.choice(total, 2, replace=False), rng.integers(0, 3, 2))) for _ in range(120)]
    effect = lambda l, k: (prog.effects[l, 0] if k < 2 else 0) ^ (prog.effects[l, 1] if k > 0 else 0)   # kinds X, Y, Z
    seen = {"wrong": 0, "right": 0, "rejected": 0}
    for i, faults in enumerate([(f,) for f in marked + others] + pairs):
        words = np.bitwise_xor.reduce([effect(l, k) for l, k in faults], axis=0).reshape(1, -1)
        _, byte = prog.tally_host(words, classes=True)
        accepted, says_wrong = bool(byte[0] & 1), bool(byte[0] & 2)
        inject = {}
        for l, k in faults:
            inject.setdefault(injection(events, gadget, prog.locations[l]), []).append(("XYZ"[k], int(prog.locations[l, 1])))
        bit = int(quil_sim.run(new_prog, seed=i, faults=inject)['ro'][0])
        if len(faults) == 1 or accepted:
            # (a rejected single fault: the preparation is repeated without it, the retry is clean and the bit is right.  Of a
            # rejected pair the model says nothing: post-selection describes accepted attempts, and the retry removes one fault only)
            assert (bit != 1) == (accepted and says_wrong), (faults, byte[0], bit)
        seen["wrong" if accepted and says_wrong else "right" if accepted else "rejected"] += 1
    assert len(marked) == len(wrong) and seen["wrong"] >= len(marked) and seen["right"] > 10 and seen["rejected"] > 10
