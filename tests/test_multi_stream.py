"""
The multi-block streamed route (DESIGN.md section 5d "Multi-block programs") without a GPU: rewritten programs on several logical
qubits with the transversal CNOT.

  gate list       MultiProgram.gates() equals, gate for gate, the quantum instructions ftqc.rewrite_program emits for the same
                  program (one pass through every loop body, as tests/test_ft.py reads them for one qubit)
  restatement     gf2_mstream_words_host equals tests/multi_stream_ref.py, which pushes full Pauli-frame vectors on (Q + 2) n qubits
                  gate by gate, on the sampler's own faults and on every single fault, for Steane and Reed-Muller [[15,1,3]]
  dense check     dense_effects() rebuilt from the block tables equals gf2_circuit_effects_timed on the whole gate list
  Q = 1           words and the shared counts equal StreamedGadget.program's host statements bit for bit
  direction       which block's next EC word shows a single fault placed before the CNOT
  records         'reference' against 'propagated'
  tally           gf2_mstream_tally_host against the restatement that keeps vectors of known errors per block
  refusals        of the plan and of the program checker, by message
  bare program    raw_circuit_error_rate against brute-force enumeration
"""
import functools
import itertools

import numpy as np
import pytest

from oracle import cpu_ref
from quantum_css_codes_amd import _native, ft_noise, ftqc, stream_noise
from quantum_css_codes_amd.errors import UnsupportedProgramError
from quantum_css_codes_amd.quil import Program, gates
from tests import multi_stream_ref, stream_ref
from tests.ec_ref import CNOT, H, IDLE, RESET
from tests.test_ft import STEANE, oracle_code
from tests.test_quil_emission import OracleCode

CNOT_MEASURE = (('CNOT', 0, 1), ('MEASURE', 1))
X_CNOT_TWO = (('X', 0), ('CNOT', 0, 1), ('MEASURE', 0), ('MEASURE', 1))
THREE = (('Y', 2), ('CNOT', 0, 2), ('CNOT', 2, 5), ('Z', 5), ('CNOT', 5, 0), ('MEASURE', 5), ('MEASURE', 0))
NONE, EC, MEASURE, CNOT_KIND = stream_noise.NONE, stream_noise.EC, stream_noise.MEASURE, stream_noise.CNOT


@functools.lru_cache(maxsize=None)
def multi(name, instructions):
    """(MultiProgram, multi_stream_ref.Rewritten) of an oracle code: nothing here needs a GPU."""
    code = oracle_code(name)
    return stream_noise.MultiProgram(code, instructions), multi_stream_ref.Rewritten(code, instructions)


# ---- the builder ---------------------------------------------------------------------------------------------------------------

def quantum_events(new_prog):
    """tests/test_ft.py's quantum_events for any number of logical qubits: (kind, a, b) in program text order."""
    insts = new_prog.instructions
    first_loop = next(pc for pc, inst in enumerate(insts) if inst[0] == "LABEL")
    events = []
    for pc in range(first_loop, len(insts)):
        inst = insts[pc]
        if inst[0] == "MEASURE":
            if inst[2].name.startswith("logical_qubit_") or inst[2].name in ("ancilla_1", "ancilla_2"):
                events.append([RESET, inst[1], 0])
            elif inst[2].name != "ro":
                events.append([IDLE, inst[1], 0])
        elif inst[0] == "GATE":
            name, qubits = inst[1], inst[2]
            if name in ("X", "Y", "Z"):
                if not (name == "X" and insts[pc - 3][0] == "JUMP-WHEN" and insts[pc - 1][0] == "LABEL" and insts[pc + 1][0] == "LABEL"):
                    events.append([IDLE, qubits[0], 0])
            elif name == "H":
                events.append([H, qubits[0], 0])
            else:
                assert name == "CNOT", name
                events.append([CNOT, qubits[0], qubits[1]])
    return events


def raw_program(instructions):
    raw = Program()
    ro = raw.declare('ro', 'BIT', 4)
    bit = 0
    for inst in instructions:
        if inst[0] == 'MEASURE':
            raw += gates.MEASURE(inst[1], ro[bit])
            bit += 1
        else:
            raw += getattr(gates, inst[0])(*inst[1:])
    return raw


@pytest.mark.parametrize("instructions", [CNOT_MEASURE, X_CNOT_TWO, THREE])
def test_builder_equals_the_emitted_program(instructions):
    new_prog = ftqc.rewrite_program(raw_program(instructions), OracleCode(STEANE, STEANE))
    got, ref = multi("steane", instructions)
    # the qubits of D_0 .. D_{Q-1}, A1, A2 are addressed 0 .. (Q + 2) n - 1 in this order
    assert quantum_events(new_prog) == got.gates().tolist()
    assert got.gates().tolist() == ref.gates.tolist()
    assert (got.num_locations, got.nsteps, got.ldw) == (ref.locations, ref.nsteps, ref.ldr)
    assert np.array_equal(got.locations()[:, 0], np.repeat(np.arange(len(ref.gates)), 1 + (ref.gates[:, 0] == CNOT)))
    from_quil = stream_noise.MultiProgram.from_quil(raw_program(instructions), oracle_code("steane"))
    assert from_quil.instructions == got.instructions and from_quil.gates().tolist() == got.gates().tolist()


def test_blocks():
    got, _ = multi("steane", X_CNOT_TWO)
    assert got.qubits == [0, 1] and got.measured == [0, 1] and got.trials == 3
    assert [t.name for t in got.types] == ['prepare data', 'logical X, EC', 'EC', 'CNOT', 'MEASURE trial']
    cnot = got.types[3]
    assert (cnot.num_locations, cnot.num_flags) == (14, 0) and not cnot.effects[:, :, 2].any()
    kinds = got.block_kind.tolist()
    assert kinds == [NONE, NONE, EC, EC, CNOT_KIND, EC, EC] + [MEASURE, EC, EC] * 6
    assert got.block_a.tolist() == [0, 1, 0, 1, 0, 0, 1] + [0, 0, 1] * 3 + [1, 0, 1] * 3
    assert got.block_b.tolist() == [-1] * 4 + [1] + [-1] * 20
    three, _ = multi("steane", THREE)
    assert three.qubits == [0, 2, 5] and three.nframes == 3
    assert [t.name for t in three.types] == ['prepare data', 'logical Y', 'EC', 'CNOT', 'logical Z', 'MEASURE trial']


# ---- the words -----------------------------------------------------------------------------------------------------------------

def single_faults(locations):
    first = np.arange(3 * locations + 1, dtype=np.int64)
    return first, np.tile(np.arange(locations, dtype=np.int32), 3), np.repeat(np.array([1, 2, 3], dtype=np.uint8), locations)


@pytest.mark.parametrize("name, instructions", [("steane", CNOT_MEASURE), ("steane", THREE), ("rm15", CNOT_MEASURE),
                                                ("rm15", (('CNOT', 1, 0), ('MEASURE', 0), ('MEASURE', 1)))])
def test_words_equal_the_restatement(name, instructions):
    got, ref = multi(name, instructions)
    assert ref.code.r_1 != ref.code.r_2 or name == "steane"           # Reed-Muller: a mix-up of the two halves shows
    sampled = stream_ref.sampled_faults(got.num_locations, 11, 1 << 33, 1500, (4e-4, 3e-4, 5e-4))
    for faults in (sampled, single_faults(got.num_locations)):
        words = got.words_of_faults(*faults)
        want = ref.outcome_words(*stream_ref.dense_faults(got.num_locations, *faults))
        assert words.shape == want.shape and np.array_equal(words, want)
        assert np.count_nonzero(words[:, :got.nsteps]) > 0 and np.count_nonzero(words[:, got.nsteps:]) > 0


def test_dense_effects_equal_the_whole_gate_list():
    got, _ = multi("steane", CNOT_MEASURE)
    assert got.ldw == 14 <= _native.FT_MAX_LDR
    rows_x, rows_z, row_time = got.outcome_rows()
    eff, locations = _native.circuit_effects_timed(got.gates(), (got.nframes + 2) * 7, _native.pack_rows(rows_x), _native.pack_rows(rows_z),
                                                   row_time, ldr=got.ldw)
    assert np.array_equal(locations, got.locations())
    assert np.array_equal(got.dense_effects(), eff)


@pytest.mark.parametrize("name, ops, p", [("steane", "", 5e-4), ("steane", "XYZIZYX", 2e-4), ("rm15", "X", 2e-4)])
def test_one_qubit_programs_equal_the_streamed_route(name, ops, p):
    code = oracle_code(name)
    one = stream_noise.StreamedGadget.program(code, ops)
    got = stream_noise.MultiProgram(code, [(op, 3) for op in ops] + [('MEASURE', 3)])
    assert got.block_kind.tolist() == one.block_kind.tolist() and got.num_locations == one.num_locations
    faults = stream_ref.sampled_faults(got.num_locations, 3, 0, 3000, (p, p, p))
    words = got.words_of_faults(*faults)
    assert np.array_equal(words, one.words_of_faults(*faults))
    want = one.tally_host(words)
    for records in ('reference', 'propagated'):
        tally = got.tally_host(words, records=records)
        flat = dict(tally, **tally['measurements'][0])
        assert {f: flat[f] for f in ft_noise.FT_FIELDS} == {f: want[f] for f in ft_noise.FT_FIELDS}
        assert flat['wrong_any'] == flat['wrong'] and flat['samples'] == 3000 and flat['qubit'] == 3
    assert want['accepted'] > 100


# ---- the direction of the CNOT -------------------------------------------------------------------------------------------------

def quiet_location_before(prog, block, frame):
    """The last fault location before block `block` on a qubit of data block `frame` whose X and Z faults fire no verification."""
    n = int(prog.code.n)
    where = prog.locations()
    for l in range(int(prog.block_start[block]) - 1, -1, -1):
        if where[l, 1] // n == frame:
            words = prog.words_of_faults([0, 1, 2], [l, l], [1, 2])
            if not words[:, prog.nsteps:].any():
                return l
    raise AssertionError("no such location")


def test_direction_of_the_cnot():
    got, _ = multi("steane", CNOT_MEASURE)
    cnot = int(np.flatnonzero(got.block_kind == CNOT_KIND)[0])
    assert (got.block_a[cnot], got.block_b[cnot]) == (0, 1)
    # the next EC steps after the CNOT: step 0 is block 0's, step 1 block 1's
    assert got.block_step[cnot + 1:cnot + 3].tolist() == [0, 1] and got.block_a[cnot + 1:cnot + 3].tolist() == [0, 1]
    control, target = quiet_location_before(got, cnot, 0), quiet_location_before(got, cnot, 1)
    key_x = lambda word: int(word) & 0x7
    key_z = lambda word: (int(word) >> 32) & 0x7
    for location, kind, key, shows in ((control, 1, key_x, (True, True)), (target, 2, key_z, (True, True)),
                                       (target, 1, key_x, (False, True)), (control, 2, key_z, (True, False))):
        words = got.words_of_faults([0, 1], [location], [kind])[0]
        assert not words[got.nsteps:].any()
        assert (key(words[0]) != 0, key(words[1]) != 0) == shows, (location, kind)
        if all(shows):
            assert key(words[0]) == key(words[1])


# ---- the records ---------------------------------------------------------------------------------------------------------------

def test_records_do_not_matter_without_a_cnot():
    got = stream_noise.MultiProgram(oracle_code("steane"), (('X', 0), ('Z', 1), ('MEASURE', 1), ('MEASURE', 0)))
    assert CNOT_KIND not in got.block_kind.tolist()
    words = got.words_of_faults(*stream_ref.sampled_faults(got.num_locations, 9, 0, 4000, (3e-4, 3e-4, 3e-4)))
    reference = got.tally_host(words, records='reference', fields=True)
    assert reference.tolist() == got.tally_host(words, records='propagated', fields=True).tolist() and reference[0] > 100


def test_records_matter_with_a_cnot():
    # a correction recorded on the control before the CNOT, then a second fault on the target: X on qubit i of D_0 before the round
    # that follows `I 0`, which records it; the CNOT copies it onto D_1; X on qubit j != i of D_1 from the CNOT block's own
    # location.  The rewritten program ('reference') meets a weight-2 error on D_1 it knows nothing of and decodes it into a logical
    # X: the bit is wrong.  With the record moved through the CNOT ('propagated') the round on D_1 finds X_j alone: the bit is right.
    got, ref = multi("steane", (('I', 0), ('CNOT', 0, 1), ('MEASURE', 1)))
    first_round = int(np.flatnonzero(got.block_kind == EC)[0])
    cnot = int(np.flatnonzero(got.block_kind == CNOT_KIND)[0])
    where = got.locations()
    one = quiet_location_before(got, first_round, 0)
    i = int(where[one, 1])
    two = next(l for l in range(int(got.block_start[cnot]), int(got.block_start[cnot + 1])) if where[l, 1] == 7 + (i + 1) % 7)
    words = got.words_of_faults([0, 2], [one, two], [1, 1])
    assert not words[0, got.nsteps:].any()
    reference = got.tally_host(words, records='reference')
    propagated = got.tally_host(words, records='propagated')
    assert reference['accepted'] == propagated['accepted'] == 1
    assert reference['measurements'][0]['wrong'] == 1 and reference['measurements'][0]['trial_wrong'] == 3 and reference['wrong_any'] == 1
    assert propagated['measurements'][0]['wrong'] == 0 and propagated['measurements'][0]['trial_wrong'] == 0
    # ... and the restatement on vectors of known errors says the same
    assert ref.tally(words, 'reference') == got.tally_host(words, records='reference', fields=True).tolist()
    assert ref.tally(words, 'propagated') == got.tally_host(words, records='propagated', fields=True).tolist()
    # the first fault alone is handled by both
    alone = got.words_of_faults([0, 1], [one], [1])
    assert got.tally_host(alone, records='reference', fields=True).tolist() == got.tally_host(alone, records='propagated', fields=True).tolist()


# ---- the tally -----------------------------------------------------------------------------------------------------------------

def random_words(rng, r_1, r_2, events, ldw, count):
    """Words that meet every branch: most accepted, quiet keys and arbitrary ones, raw parities, some rejected."""
    steps = [e for e in events if e[0] != multi_stream_ref.GATE_CNOT]
    nsteps = len(steps)
    words = np.zeros((count, ldw), dtype=np.uint64)
    key_x = rng.integers(0, 1 << r_2, (count, nsteps), dtype=np.uint64)
    key_z = rng.integers(0, 1 << r_1, (count, nsteps), dtype=np.uint64)
    quiet = rng.random((count, nsteps)) < 0.75
    key_x[quiet], key_z[quiet] = 0, 0
    parity = (rng.random((count, nsteps)) < 0.2).astype(np.uint64)
    for s, step in enumerate(steps):
        words[:, s] = key_x[:, s] | (parity[:, s] << np.uint64(31) if step[0] == multi_stream_ref.MEASURE else key_z[:, s] << np.uint64(32))
    pick = rng.random(count)
    words[pick < 0.1, nsteps] = rng.integers(1, 1 << 62, int((pick < 0.1).sum()), dtype=np.uint64)
    last = (pick >= 0.1) & (pick < 0.2)
    words[last, ldw - 1] = np.uint64(1) << rng.integers(0, 64, int(last.sum()), dtype=np.uint64)
    return words


@pytest.mark.parametrize("name, instructions", [("steane", X_CNOT_TWO), ("steane", THREE),
                                                ("rm15", (('I', 0), ('CNOT', 0, 1), ('MEASURE', 1)))])
def test_tally_host_equals_the_restatement(name, instructions):
    got, ref = multi(name, instructions)
    words = random_words(np.random.default_rng(len(instructions)), got.code.r_1, got.code.r_2, ref.events, got.ldw, 3000)
    counts = {}
    for records in ('reference', 'propagated'):
        counts[records], classes = got.tally_host(words, records=records, fields=True, classes=True)
        want = ref.tally(words, records)
        assert counts[records].tolist() == want
        assert int((classes & 1).sum()) == want[0] and int(((classes >> 1) & 1).sum()) == want[1]
        assert [int(((classes >> (2 + m)) & 1).sum()) for m in range(4)] == want[4::4]
        assert 0 < want[0] < 3000 and 0 < want[4] < want[0] and want[7] > 0 and want[5] > want[4] and want[6] > 0
    assert counts['reference'].tolist() != counts['propagated'].tolist()
    as_dict = got.tally_host(words)
    assert [m['qubit'] for m in as_dict['measurements']] == got.measured and as_dict['samples'] == 3000
    assert as_dict['measurements'][-1]['split_vote'] == int(counts['reference'][4 * len(got.measured) + 3])


def test_tally_host_with_unmatched_keys_on_both_sides():
    # tests/test_ft.py's construction: random full-rank checks on 9 bits with tables that hold a part of the keys; the blocks are
    # not the builder's -- four frames, CNOTs in both directions, one to five trials
    rng = np.random.default_rng(17)
    vectors = np.array(list(itertools.product((0, 1), repeat=9)))

    def side(r, entries):
        while True:
            check = rng.integers(0, 2, (r, 9))
            keys = np.array([cpu_ref.vec_to_int(v) for v in (vectors @ check.T) % 2])
            if len(set(keys.tolist())) == 1 << r:
                break
        return check, {int(k): vectors[np.flatnonzero(keys == k)[0]] for k in rng.choice(1 << r, entries, replace=False)}

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
    E, M, C = multi_stream_ref.EC, multi_stream_ref.MEASURE, multi_stream_ref.GATE_CNOT
    for frames, events in ((1, [(M, 0, 0)]),
                           (2, [(E, 0), (E, 1), (C, 0, 1), (E, 0), (E, 1), (C, 1, 0), (E, 1)] + [(M, 1, 0), (E, 0), (E, 1)] * 3),
                           (4, [(E, 3), (C, 3, 0), (E, 0), (C, 0, 2), (E, 2), (C, 2, 1), (E, 1), (C, 1, 3)] + [(M, 2, 0), (E, 2), (E, 1)] * 5 +
                               [(M, 0, 1), (E, 3)] * 5 + [(M, 3, 2)] * 5 + [(M, 1, 3), (C, 0, 1)] * 5)):
        kind_of = {E: EC, M: MEASURE, C: CNOT_KIND}
        kinds = [kind_of[e[0]] for e in events]
        frame_a = [e[1] for e in events]
        frame_b = [e[2] if e[0] == C else -1 for e in events]
        nsteps = sum(e[0] != C for e in events)
        words = random_words(rng, 5, 6, events, nsteps + 2, 3000)
        for records in ('reference', 'propagated'):
            counts = _native.mstream_tally_host(words, kinds, frame_a, frame_b, frames, 2, stream_noise.RECORDS[records], 5, keys1, flips1,
                                                6, keys2, flips2)
            want = multi_stream_ref.tally(code, events, frames, words, records)
            assert counts.tolist() == want
            assert want[2] > 0 and (want[3] > 0 or frames == 1) and want[1] > 0 and (want[7] > 0 or frames == 1)
    wide = np.zeros((3000, nsteps + 5), dtype=np.uint64)              # ldw > nsteps + F: the words of a sample lie ldw apart
    wide[:, :nsteps + 2], wide[:, nsteps + 2:] = words, 1
    assert _native.mstream_tally_host(wide, kinds, frame_a, frame_b, 4, 2, 1, 5, keys1, flips1, 6, keys2, flips2).tolist() == want


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def test_program_checker_refusals():
    steane = oracle_code("steane")
    for instructions, text in (([('H', 0), ('MEASURE', 0)], "'H'"), ([('CZ', 0, 1), ('MEASURE', 0)], "'CZ'"), ([('S', 0), ('MEASURE', 0)], "'S'"),
                               ([('CNOT', 1, 1), ('MEASURE', 1)], r"\('CNOT', 1, 1\)"), ([('CNOT', 0), ('MEASURE', 0)], r"\('CNOT', 0\)"),
                               ([('X', 0, 1), ('MEASURE', 0)], r"\('X', 0, 1\)"), ([('X', -1), ('MEASURE', 0)], r"\('X', -1\)"),
                               ([('JUMP', 'somewhere'), ('MEASURE', 0)], "'JUMP'"),
                               ([('MEASURE', 0), ('X', 0)], r"after a MEASURE: \('X', 0\)"),
                               ([('MEASURE', 0), ('CNOT', 0, 1)], r"after a MEASURE: \('CNOT', 0, 1\)"),
                               ([('MEASURE', 0), ('MEASURE', 1), ('MEASURE', 0)], "qubit 0 is measured twice"),
                               ([('X', 0)], "end with a MEASURE"), ([], "end with a MEASURE"),
                               ([('CNOT', 0, 1), ('CNOT', 2, 3), ('X', 4), ('MEASURE', 0)], r"\('X', 4\).*at most 4 logical qubits")):
        with pytest.raises(UnsupportedProgramError, match=text):
            stream_noise.MultiProgram(steane, instructions)
        with pytest.raises(UnsupportedProgramError, match=text):
            ft_noise.raw_circuit_error_rate(instructions, 0.1, 0.0, 0.0)
    raw = Program()
    ro = raw.declare('ro', 'BIT', 2)
    for insts, text in (([gates.H(0), gates.MEASURE(0, ro[0])], "'H'"), ([gates.CZ(0, 1), gates.MEASURE(0, ro[0])], "'CZ'"),
                        ([gates.X(0), ("JUMP", "somewhere"), gates.MEASURE(0, ro[0])], "JUMP"),
                        ([gates.CNOT(0, 1), gates.MEASURE(0, ro[0]), gates.X(0)], "after a MEASURE"),
                        ([gates.CNOT(0, 1)], "end with a MEASURE")):
        with pytest.raises(UnsupportedProgramError, match=text):
            stream_noise.MultiProgram.from_quil(Program(raw, insts), steane)
    got, _ = multi("steane", CNOT_MEASURE)
    with pytest.raises(ValueError, match="'reference' or 'propagated'"):
        got.tally_host(np.zeros((1, got.ldw), dtype=np.uint64), records='moved')
    assert stream_noise.multi_program_for(steane, CNOT_MEASURE) is stream_noise.multi_program_for(steane, [list(i) for i in CNOT_MEASURE])


def test_plan_refusals():
    got, _ = multi("steane", CNOT_MEASURE)
    eff, locs, flags, types, kinds, frame_a, frame_b, frames = got._sequence()
    none = (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint8))
    cnot = int(np.flatnonzero(kinds == CNOT_KIND)[0])
    trial = int(np.flatnonzero(kinds == MEASURE)[0])

    def changed(array, at, value):
        out = array.copy()
        out[at] = value
        return out

    cases = ((dict(nframes=0), "1 <= nframes <= 4 data frames"), (dict(nframes=5), "1 <= nframes <= 4 data frames"),
             (dict(kinds=changed(kinds, 2, 3)), "block 2 is a FINAL step, this route has none"),
             (dict(kinds=changed(kinds, 2, 5)), "block 2 has kind 5, not NONE"),
             (dict(a=changed(frame_a, 3, 2)), r"block 3 has frame 2 outside \[0, nframes = 2\)"),
             (dict(b=changed(frame_b, cnot, 2)), "CNOT block %d has target frame 2 outside" % cnot),
             (dict(b=changed(frame_b, cnot, 0)), "CNOT block %d has frame 0 as control and as target" % cnot),
             (dict(b=changed(frame_b, 0, 1)), "block 0 is no CNOT block, its second frame must be -1, got 1"),
             (dict(a=changed(frame_a, trial + 3, 0)), "frame 1 is measured twice"),
             (dict(kinds=np.where(kinds == MEASURE, EC, kinds)), "at least one MEASURE step"),
             (dict(kinds=changed(kinds, trial, EC)), "same odd number of MEASURE steps"),
             (dict(types=changed(types, cnot, 0)), "CNOT block %d has a type with 7 flag rows" % cnot),
             (dict(types=changed(types, 0, 9)), r"block 0 has type 9 outside \[0, 4\)"),
             (dict(flags=changed(flags, 0, 65)), "block type 0 has 65 flag rows"),
             (dict(flags=changed(flags, 0, 3)), "set flag bits at or above its 3 flag rows"))
    for change, text in cases:
        args = dict(eff=eff, locs=locs, flags=flags, types=types, kinds=kinds, a=frame_a, b=frame_b, nframes=frames)
        args.update(change)
        with pytest.raises(_native.GF2Error, match=text):
            _native.mstream_words_host(args['eff'], args['locs'], args['flags'], args['types'], args['kinds'], args['a'], args['b'],
                                       args['nframes'], *none, got.ldw)
    with pytest.raises(_native.GF2Error, match="ldw >= nsteps \\+ F = 14 words"):
        _native.mstream_words_host(*got._sequence(), *none, got.ldw - 1)
    with pytest.raises(_native.GF2Error, match=r"location 3382 outside \[0, L = 3382\)"):
        got.words_of_faults([0, 1], [3382], [1])
    with pytest.raises(_native.GF2Error, match="kind 4, not 1"):
        got.words_of_faults([0, 1], [0], [4])
    words = np.zeros((2, got.ldw), dtype=np.uint64)
    tables = got._tables()
    for change, text in ((dict(records=2), r"records must be GF2_MSTREAM_REFERENCE \(0\) or GF2_MSTREAM_PROPAGATED \(1\), got 2"),
                         (dict(flag_words=0), "F >= 1"), (dict(nframes=5), "1 <= nframes <= 4"),
                         (dict(kinds=changed(kinds, trial, EC)), "same odd number of MEASURE steps"),
                         (dict(flag_words=4), "ldw >= nsteps \\+ F = 15 words")):
        args = dict(kinds=kinds, nframes=frames, flag_words=got.flag_words, records=0)
        args.update(change)
        with pytest.raises(_native.GF2Error, match=text):
            _native.mstream_tally_host(words, args['kinds'], frame_a, frame_b, args['nframes'], args['flag_words'], args['records'], *tables)
    with pytest.raises(_native.GF2Error, match="r_1, r_2 <= 31"):
        _native.mstream_tally_host(words, kinds, frame_a, frame_b, frames, got.flag_words, 0, 32, *tables[1:])
    empty = _native.mstream_tally_host(np.zeros((0, got.ldw), dtype=np.uint64), kinds, frame_a, frame_b, frames, got.flag_words, 1, *tables)
    assert empty.tolist() == [0] * 20


def test_plan_refusals_of_the_shared_rules():
    # the rules gf2_mstream_plan states in its own text beside gf2_stream_plan's (tests/test_stream.py pins those for that plan only)
    got, _ = multi("steane", CNOT_MEASURE)
    eff, locs, flags, types, kinds, frame_a, frame_b, frames = got._sequence()
    none = (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint8))
    trial_type = int(types[np.flatnonzero(kinds == MEASURE)[0]])
    round_type = int(types[np.flatnonzero(kinds == EC)[0]])

    def one_frame(eff, locs, flags, types, kinds, faults=none, ldw=8):
        return _native.mstream_words_host(eff, locs, flags, types, kinds, np.zeros(len(kinds), dtype=np.int32),
                                          np.full(len(kinds), -1, dtype=np.int32), 1, *faults, ldw)

    row = np.zeros((1, 2, 3), dtype=np.uint64)
    assert one_frame(row, [1], [0], [0], [MEASURE]).shape == (0, 8)
    for ntypes in (0, 65):
        with pytest.raises(_native.GF2Error, match="1 <= ntypes <= 64 block types, got %d" % ntypes):
            one_frame(np.zeros((ntypes, 2, 3), dtype=np.uint64), [1] * ntypes, [0] * ntypes, [0], [MEASURE])
    assert one_frame(np.zeros((64, 2, 3), dtype=np.uint64), [1] * 64, [0] * 64, [63], [MEASURE]).shape == (0, 8)
    for nblocks in (0, (1 << 20) + 1):
        with pytest.raises(_native.GF2Error, match=r"1 <= nblocks <= 1048576 blocks, got %d" % nblocks):
            one_frame(row, [1], [0], np.zeros(nblocks, dtype=np.int32), np.full(nblocks, MEASURE, dtype=np.int32))
    with pytest.raises(_native.GF2Error, match=r"block type 1 needs 1 <= locations <= 1048576 \(2\^20\), got 0"):
        one_frame(row, [1, 0], [0, 0], [0], [MEASURE])
    with pytest.raises(_native.GF2Error, match=r"block type 0 needs 1 <= locations <= 1048576 \(2\^20\), got 1048577"):
        one_frame(np.zeros(((1 << 20) + 1, 2, 3), dtype=np.uint64), [(1 << 20) + 1], [0], [0], [MEASURE])
    with pytest.raises(_native.GF2Error, match=r"the block types have more than 1048576 \(2\^20\) locations in all"):
        one_frame(np.zeros(((1 << 20) + 1, 2, 3), dtype=np.uint64), [1 << 20, 1], [0, 0], [0], [MEASURE])
    # 3200 rounds on frame 0, then the trial: the Steane round's locations pass 2^20 on the way
    assert 3200 * int(locs[round_type]) > 1 << 20
    long_types, long_kinds = np.array([round_type] * 3200 + [trial_type], dtype=np.int32), np.array([EC] * 3200 + [MEASURE], dtype=np.int32)
    with pytest.raises(_native.GF2Error, match=r"the sequence has more than L = 1048576 \(2\^20\) fault locations"):
        one_frame(eff, locs, flags, long_types, long_kinds, ldw=4000)

    words = lambda first, where, kind: _native.mstream_words_host(eff, locs, flags, types, kinds, frame_a, frame_b, frames, first, where, kind, got.ldw)
    assert words((0, 1), (5,), (1,)).shape == (1, got.ldw)
    for faults, text in ((((1, 1), (5,), (1,)), r"fault_first\[0\] must be 0"),
                         (((0, 1, 0, 1), (5,), (1,)), r"fault_first must not descend \(sample 1\)"),
                         (((0, 1), (-1,), (1,)), r"location -1 outside \[0, L = 3382\)"),
                         (((0, 1), (5,), (0,)), "has kind 0, not 1")):
        with pytest.raises(_native.GF2Error, match=text):
            words(*faults)
    # a fault count without the lists: the wrapper never passes that, the entry point is called as a C caller would
    keep, seq = _native._mstream_sequence(eff, locs, flags, types, kinds, frame_a, frame_b, frames)
    first, out = np.array([0, 1], dtype=np.int64), np.zeros((1, got.ldw), dtype=np.uint64)
    with pytest.raises(_native.GF2Error, match="gf2_mstream_words_host: null fault list"):
        _native.check(_native.lib().gf2_mstream_words_host(*seq, _native._ptr(first), None, None, 1, _native._ptr(out), got.ldw))
    with pytest.raises(_native.GF2Error, match="gf2_mstream_words_host: null argument"):
        _native.check(_native.lib().gf2_mstream_words_host(*seq, None, None, None, 1, _native._ptr(out), got.ldw))

    # the tally: a key twice in a table; the number of trials, odd and at most 255
    r1, keys1, flips1, r2, keys2, flips2 = got._tables()
    good = np.zeros((2, got.ldw), dtype=np.uint64)
    assert len(keys1) > 1 and len(keys2) > 1
    with pytest.raises(_native.GF2Error, match="gf2_mstream_tally_host: a syndrome key occurs twice in a table"):
        _native.mstream_tally_host(good, kinds, frame_a, frame_b, frames, got.flag_words, 0, r1, np.zeros(len(keys1), dtype=np.uint64), flips1,
                                   r2, keys2, flips2)
    with pytest.raises(_native.GF2Error, match="gf2_mstream_tally_host: a syndrome key occurs twice in a table"):
        _native.mstream_tally_host(good, kinds, frame_a, frame_b, frames, got.flag_words, 1, r1, keys1, flips1, r2,
                                   np.full(len(keys2), keys2[0], dtype=np.uint64), flips2)

    def trials_tally(trials):
        steps = np.full(trials, MEASURE, dtype=np.int32)
        return _native.mstream_tally_host(np.zeros((2, trials + 1), dtype=np.uint64), steps, np.zeros(trials, dtype=np.int32),
                                          np.full(trials, -1, dtype=np.int32), 1, 1, 0, r1, keys1, flips1, r2, keys2, flips2)

    assert trials_tally(255).tolist() == [2] + [0] * 19
    with pytest.raises(_native.GF2Error, match="same odd number of MEASURE steps .*, at most 255; measurement 0 has 257, measurement 0 has 257"):
        trials_tally(257)
    with pytest.raises(_native.GF2Error, match="same odd number of MEASURE steps .*, at most 255; measurement 0 has 254"):
        trials_tally(254)


# ---- the bare program ----------------------------------------------------------------------------------------------------------

def brute_force_rates(instructions, p_x, p_y, p_z):
    """Per MEASURE, the probability of a wrong bit summed over every assignment of I, X, Y, Z to the bare circuit's locations: a
    Pauli frame pushed through the gates, a fault entering after its gate (before a measurement)."""
    qubits = sorted({q for inst in instructions for q in inst[1:]})
    sites = []
    for inst in instructions:
        if inst[0] == 'CNOT':
            sites += [(inst, inst[1]), (inst, inst[2])]
        elif inst[0] != 'I':
            sites.append((inst, inst[1]))
    measures = sum(inst[0] == 'MEASURE' for inst in instructions)
    out = [0.0] * measures
    weight_of = {"I": 1 - p_x - p_y - p_z, "X": p_x, "Y": p_y, "Z": p_z}
    for kinds in itertools.product("IXYZ", repeat=len(sites)):
        weight = float(np.prod([weight_of[k] for k in kinds]))
        x = {q: 0 for q in qubits}
        at, bit = 0, 0
        for inst in instructions:
            if inst[0] == 'CNOT':
                x[inst[2]] ^= x[inst[1]]
                x[inst[1]] ^= kinds[at] in "XY"
                x[inst[2]] ^= kinds[at + 1] in "XY"
                at += 2
            elif inst[0] == 'MEASURE':
                x[inst[1]] ^= kinds[at] in "XY"
                out[bit] += weight * x[inst[1]]
                at, bit = at + 1, bit + 1
            elif inst[0] != 'I':
                x[inst[1]] ^= kinds[at] in "XY"
                at += 1
    return out


def test_raw_circuit_error_rate_equals_enumeration():
    programs = (CNOT_MEASURE, X_CNOT_TWO, (('X', 0), ('CNOT', 0, 1), ('CNOT', 0, 1), ('MEASURE', 1)),
                (('CNOT', 0, 1), ('I', 0), ('CNOT', 1, 2), ('MEASURE', 2), ('MEASURE', 0)), (('Z', 4), ('MEASURE', 4)))
    for instructions, p in itertools.product(programs, ((0.01, 0.002, 0.03), (0.2, 0.1, 0.3), (0.0, 0.0, 0.5))):
        got = ft_noise.raw_circuit_error_rate(instructions, *p)
        want = brute_force_rates(instructions, *p)
        assert len(got) == len(want) and all(abs(g - w) < 1e-14 for g, w in zip(got, want)), instructions
    # one qubit: raw_program_error_rate
    assert ft_noise.raw_circuit_error_rate([('X', 0), ('I', 0), ('Y', 0), ('MEASURE', 0)], 0.01, 0.02, 0.3) == \
        [ft_noise.raw_program_error_rate("XIY", 0.01, 0.02, 0.3)]
    # either bit sees three locations: X 0 reaches both, a CNOT's own two faults follow the gate and stay where they are
    assert ft_noise.raw_circuit_error_rate(X_CNOT_TWO, 0.1, 0.0, 0.0) == [0.5 * (1 - 0.8 ** 3), 0.5 * (1 - 0.8 ** 3)]
