"""
The multi-block streamed route on the GPU (stream_noise.MultiProgram, csrc/gf2_mstream.hip; DESIGN.md section 5d "Multi-block
programs").  Every comparison is exact.

The device words must equal gf2_mstream_words_host on the faults of the restated sampler (the oracle's, over the L locations:
tests/stream_ref.py), and the device counts the host tally rule over the stored words, under both settings of `records`.  The host
statements themselves are checked against the NumPy restatement without a GPU (tests/test_multi_stream.py).  A case's reference is
computed once and shared by its tests.

The cases are the smallest at which mstream_kernel takes another path: one, two and four frames (the three instantiations; three
frames run as four), a three-qubit program whose CNOTs use all six ordered pairs of frames (every arm of the select chains),
Reed-Muller (r_1 != r_2, blocks that span segments), tables staged in LDS and tables of 186 KB read through L2, no fault at all, and
a program of 300 gates.  The rates are a few 1e-4 per kind: the programs have 6 000 to 17 000 locations and every preparation is
post-selected, so at 1e-3 nothing would be accepted; each case keeps a few hundred of its 2^14 samples, and says so.
"""
import functools

import numpy as np
import pytest

from quantum_css_codes_amd import _native, stream_noise
from tests import stream_ref
from tests.test_gpu_stream import make_code

pytestmark = pytest.mark.gpu

SAMPLES = 1 << 14
PAIRS = tuple(('CNOT', a, b) for a, b in ((0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1)))
#        code, instructions, p_kind, seed, first_sample
CASES = {
    "steane-2": ("steane", (('X', 0), ('CNOT', 0, 1), ('MEASURE', 0), ('MEASURE', 1)), 3e-4, 5, 3),
    "steane-4": ("steane", (('X', 0), ('CNOT', 0, 1), ('CNOT', 2, 3), ('Y', 3), ('CNOT', 1, 2), ('MEASURE', 3), ('MEASURE', 0)), 1.5e-4, 6, 1 << 33),
    "rm15-2": ("rm15", (('CNOT', 0, 1), ('MEASURE', 1)), 2e-4, 7, 0),
    "steane-3-pairs": ("steane", PAIRS + (('MEASURE', 0), ('MEASURE', 1), ('MEASURE', 2)), 1.5e-4, 8, 11),
    "rm15-unstaged": ("rm15", (('X', 0), ('Y', 0), ('Z', 0), ('CNOT', 0, 1), ('MEASURE', 1)), 1e-4, 9, 0),   # seven types, 186 KB: read through L2
}
STAGED_LIMIT = 160 * 1024 - (2 * 513 * 8 + 256 * 17 * 4 + 32 * 4)       # what mstream_launch leaves for the tables


@functools.lru_cache(maxsize=None)
def program(name, instructions):
    return stream_noise.multi_program_for(make_code(name), instructions)


@functools.lru_cache(maxsize=None)
def reference(case):
    """(the host statement's words on the restated sampler's faults, its counts under either setting); never modified."""
    name, instructions, p, seed, first = CASES[case]
    prog = program(name, instructions)
    words = prog.words_of_faults(*stream_ref.sampled_faults(prog.num_locations, seed, first, SAMPLES, (p, p / 2, p)))
    words.setflags(write=False)
    return words, {records: prog.tally_host(words, records=records, fields=True) for records in stream_noise.RECORDS}


@pytest.mark.parametrize("case", sorted(CASES))
def test_words_and_counts_equal_the_host_statements(case):
    name, instructions, p, seed, first = CASES[case]
    prog = program(name, instructions)
    want_words, want = reference(case)
    assert (prog.type_eff.nbytes > STAGED_LIMIT) == (case == "rm15-unstaged")
    got = prog.outcomes(SAMPLES, p, p / 2, p, seed=seed, first_sample=first)
    assert got.shape == want_words.shape and np.array_equal(got, want_words)
    print("\n%s: L = %d, %d blocks, reference %s, propagated %s" % (case, prog.num_locations, len(prog.block_type), want['reference'].tolist(),
                                                                   want['propagated'].tolist()))
    # a test that accepts nothing proves nothing: a few hundred accepted samples, and some of them with a wrong trial
    assert want['reference'][0] >= 300 and SAMPLES - want['reference'][0] >= 300 and want['reference'][5] >= 1
    for records in stream_noise.RECORDS:
        counts = prog.counts(SAMPLES, p, p / 2, p, seed=seed, first_sample=first, records=records)
        assert counts.tolist() == want[records].tolist() == prog.tally_host(got, records=records, fields=True).tolist()
    as_dict = prog.error_rates(SAMPLES, p, p / 2, p, seed=seed, first_sample=first, records='propagated')
    assert as_dict == prog.tally_host(got, records='propagated')


def test_records_change_the_counts_of_a_case():
    # all six ordered pairs: records recorded before a CNOT are moved by it, and some sample of the 2^14 tallies differently
    _, want = reference("steane-3-pairs")
    assert want['reference'].tolist() != want['propagated'].tolist() and want['reference'][0] == want['propagated'][0]


@pytest.mark.parametrize("name, ops, p", [("steane", "", 5e-4), ("steane", "XYZIZYX", 2e-4), ("rm15", "X", 2e-4)])
def test_one_qubit_programs_equal_the_streamed_kernel(name, ops, p):
    code = make_code(name)
    one = stream_noise.stream_for(code, "program", tuple(ops))
    prog = program(name, tuple((op, 0) for op in ops) + (('MEASURE', 0),))
    want = one.counts(SAMPLES, p, p, p, seed=3, first_sample=9)       # gf2_mc_stream_decode's twelve
    assert want[0] >= 300
    for records in stream_noise.RECORDS:
        got = prog.counts(SAMPLES, p, p, p, seed=3, first_sample=9, records=records)
        assert [int(got[k]) for k in (0, 2, 3, 4, 5, 6, 7)] == [int(want[k]) for k in (0, 6, 7, 8, 9, 10, 11)]
        assert got[1] == got[4] and not got[8:].any()
    assert np.array_equal(prog.outcomes(2000, p, p, p, seed=3, first_sample=9), one.outcomes(2000, p, p, p, seed=3, first_sample=9))


def test_no_faults_no_failures():
    for case in ("steane-2", "steane-3-pairs", "rm15-unstaged"):
        name, instructions, _, _, _ = CASES[case]
        prog = program(name, instructions)
        for records in stream_noise.RECORDS:
            counts = prog.counts(5000, 0.0, 0.0, 0.0, seed=1, records=records)
            assert counts.tolist() == [5000] + [0] * 19
        assert not prog.outcomes(300, 0.0, 0.0, 0.0).any()


def test_shards_add_up():
    name, instructions, p, seed, first = CASES["steane-2"]
    prog = program(name, instructions)
    _, want = reference("steane-2")
    for records in stream_noise.RECORDS:
        total = np.zeros(20, dtype=np.uint64)
        at = first
        for count in (1, 255, 1000, 0, 4097, SAMPLES - 1 - 255 - 1000 - 4097):      # a count of 1, counts that are no multiple of 256
            total += prog.counts(count, p, p / 2, p, seed=seed, first_sample=at, records=records)
            at += count
        assert total.tolist() == want[records].tolist()
    words, _ = reference("steane-2")
    assert np.array_equal(prog.outcomes(1, p, p / 2, p, seed=seed, first_sample=first + 777), words[777:778])
    assert np.array_equal(prog.outcomes(301, p, p / 2, p, seed=seed, first_sample=first + 5000), words[5000:5301])


def test_a_long_program():
    # 300 gates on two qubits: 612 EC steps and 6 MEASURE steps, 205 490 locations, 402 segments
    gates = [(('X', 'CNOT', 'Z', 'CNOT', 'Y')[g % 5],) + ((g % 2, 1 - g % 2) if g % 5 in (1, 3) else (g % 2,)) for g in range(300)]
    prog = program("steane", tuple(gates) + (('MEASURE', 1), ('MEASURE', 0)))
    assert prog.num_locations > 190000 and prog.nsteps > 600
    p, count = 4e-6, 1 << 10
    want = prog.words_of_faults(*stream_ref.sampled_faults(prog.num_locations, 21, 5, count, (p, p, p)))
    got = prog.outcomes(count, p, p, p, seed=21, first_sample=5)
    assert np.array_equal(got, want)
    for records in stream_noise.RECORDS:
        tally = prog.tally_host(want, records=records, fields=True)
        assert prog.counts(count, p, p, p, seed=21, first_sample=5, records=records).tolist() == tally.tolist()
    assert 50 <= tally[0] < count


def test_refusals_of_the_device_entry_points():
    name, instructions, p, _, _ = CASES["steane-2"]
    prog = program(name, instructions)
    ctx = _native.default_context()
    with pytest.raises(_native.GF2Error, match="records must be GF2_MSTREAM_REFERENCE"):
        ctx.mc_mstream_decode(prog.device(), 2, *prog._tables(), 0, 0, 10, p, p, p)
    with pytest.raises(_native.GF2Error, match="ldo must be at least the sequence's nsteps \\+ F = 27 words"):
        ctx.outcomes(ctx.mstream_outcomes_dev, prog.device(), 0, 0, 10, p, p, p, prog.ldw - 1)
    with pytest.raises(_native.GF2Error, match="r_1, r_2 <= 31"):
        ctx.mc_mstream_decode(prog.device(), 0, 32, *prog._tables()[1:], 0, 0, 10, p, p, p)
    with pytest.raises(_native.GF2Error, match="beyond the layout"):
        ctx.mc_mstream_decode(prog.device(), 0, 2, *prog._tables()[1:], 0, 0, 10, p, p, p)
    # a segment of 512 locations over more than eight blocks: nine Pauli blocks of three locations each
    eff, locs, flags, types, kinds, frame_a, frame_b, frames = prog._sequence()
    pauli = stream_noise.BlockType(prog.code, "logical X", stream_noise.NONE, stream_noise._emit_pauli([0, 1, 2]))
    many = (np.concatenate([eff, pauli.effects]), list(locs) + [3], list(flags) + [0], [len(locs)] * 9 + list(types), [0] * 9 + list(kinds),
            [0] * 9 + list(frame_a), [-1] * 9 + list(frame_b), frames)
    with pytest.raises(_native.GF2Error, match="locations 0 .. 511 .* overlap 1[0-9] blocks, more than 8 \\(GF2_STREAM_MAX_OVERLAP\\)"):
        ctx.mstream_create(*many)
    assert _native.mstream_words_host(*many, [0, 1], [0], [1], prog.ldw).shape == (1, prog.ldw)   # (the host statement has no such rule)
