"""
The fault-tolerant logical measurement on the GPU (quantum_css_codes_amd/ft_noise.py, csrc/gf2_ft.hip).  Every
comparison is exact.

  outcome words   gf2_ft_outcomes_dev against tests/ft_ref.py fed by the oracle's sampler run over the L locations
                  (c_oracle.sample_errors with n := L): 4096 samples at (0.01, 0.005, 0.01), where every 512-location segment draws
                  several faults (Floyd's map), for every LDR the test programs have: Steane with 0, 3 and 7 logical gates (LDR 8, 11,
                  16; 4, 6 and 8 sampler segments) and Reed-Muller [[15,1,3]] with none (LDR 9; r_1 != r_2)
  counts          gf2_mc_ft_decode against gf2_ft_tally_host of the device's own stored words, same seed and range, 2^18 samples,
                  all seven fields, at rates low enough for samples to be accepted

The rates of the count cases were chosen on the CPU: tests/ft_ref.py with the oracle's sampler on all 2^18 samples of each case's
own stream (same seed and first_sample; 8 to 20 seconds a case, too slow for this file) gave
    steane-0  accepted 105134  wrong 541  trial_wrong 2075  first_trial_wrong 325  split_vote 1186  unmatched_x 0     unmatched_z 0
    steane-3  accepted 108398  wrong 669  trial_wrong 2233  first_trial_wrong 575  split_vote 594   unmatched_x 0     unmatched_z 0
    steane-7  accepted 107829  wrong 727  trial_wrong 2343  first_trial_wrong 678  split_vote 358   unmatched_x 0     unmatched_z 0
    rm15-0    accepted 62957   wrong 12   trial_wrong 59    first_trial_wrong 7    split_vote 43    unmatched_x 1119  unmatched_z 0
(REFERENCE_COUNTS below; the host tally of the device's words must give exactly these), so accepted, rejected, wrong and split
samples occur in every case.  An unmatched key cannot occur for the Steane code, whose tables hold all 2^3 syndromes, nor on the z
side of the Reed-Muller code (C1 is the Hamming code: all 2^4); it occurs for the Reed-Muller code's key_x (16 of 2^10 syndromes are
in the table), and the test asserts it there.  tests/test_ft.py meets unmatched keys on both sides on the host.
"""
import functools

import numpy as np
import pytest

from oracle import c_oracle
from quantum_css_codes_amd import _native, ft_noise
from quantum_css_codes_amd.css_code import CSSCode
from tests import ft_ref

pytestmark = pytest.mark.gpu

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
FIELDS = ft_noise.FT_FIELDS
DENSE = (0.01, 0.005, 0.01)
#        code, logical gates, seed, first_sample of the outcome words; (p_x, p_y, p_z), seed, first_sample of the counts
CASES = {
    "steane-0": ("steane", "", 1, 0, (0.0004, 0.0002, 0.0004), 11, 0),                 # LDR 8
    "steane-3": ("steane", "XXX", 2, (1 << 33) + 5, (0.00024, 0.00012, 0.00024), 12, 3),   # LDR 11
    "steane-7": ("steane", "XYZIZYX", 3, 0, (0.00016, 0.00008, 0.00016), 13, 1 << 40),  # LDR 16
    "rm15-0": ("rm15", "", 4, 0, (0.00024, 0.00012, 0.00024), 14, 0),                  # LDR 9
}
COUNT = 1 << 18
REFERENCE_COUNTS = {                                                                 # tests/ft_ref.py and the oracle's sampler alone (see above)
    "steane-0": (105134, 541, 2075, 325, 1186, 0, 0),
    "steane-3": (108398, 669, 2233, 575, 594, 0, 0),
    "steane-7": (107829, 727, 2343, 678, 358, 0, 0),
    "rm15-0": (62957, 12, 59, 7, 43, 1119, 0),
}


def checks_of(name):
    if name == "steane":
        return STEANE, STEANE
    cols = np.arange(1, 16)
    h1 = np.array([(cols >> b) & 1 for b in range(4)])
    return h1, np.vstack([h1] + [h1[a] & h1[b] for a in range(4) for b in range(a + 1, 4)])


@functools.lru_cache(maxsize=None)
def make_code(name):
    return CSSCode(*checks_of(name))


@functools.lru_cache(maxsize=None)
def program(case):
    name, ops = CASES[case][:2]
    code = make_code(name)
    return ft_noise.program_for(code, ops), ft_ref.Rewritten(code, ops)


def reference_words(ref, seed, first, count, p, chunk=4096):
    parts = []
    for start in range(0, count, chunk):
        now = min(chunk, count - start)
        faults = []
        for packed in c_oracle.sample_errors(ref.locations, seed, first + start, now, *p):
            sample, location = np.nonzero(c_oracle.unpack_rows(packed, ref.locations, dtype=np.uint8))
            dense = np.zeros((ref.locations, now), dtype=np.uint8)                   # (L, samples): a location's faults lie together
            dense[location, sample] = 1
            faults.append(dense)
        parts.append(ref.outcome_words(*faults))
    return np.concatenate(parts)


@functools.lru_cache(maxsize=None)
def device_words(case):
    """The device's stored outcome words of a count case and their host tally; computed once, never modified."""
    prog, _ = program(case)
    p, seed, first = CASES[case][4:]
    words = prog.outcomes(COUNT, *p, seed=seed, first_sample=first)
    words.setflags(write=False)
    return words, prog.tally_host(words)


@pytest.mark.parametrize("case", sorted(CASES))
def test_outcome_words_equal_the_restatement(case):
    name, ops, seed, first = CASES[case][:4]
    prog, ref = program(case)
    assert (prog.num_locations, prog.ldr, prog.nsteps, prog.measure_mask) == (ref.locations, ref.ldr, ref.nsteps, ref.measure_mask)
    want = reference_words(ref, seed, first, 4096, DENSE)
    got = prog.outcomes(4096, *DENSE, seed=seed, first_sample=first)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.count_nonzero(want.any(axis=1)) > 4000                                 # (at these rates nearly every sample has faults)


def test_cases_cover_the_kernel_instantiations():
    assert [program(c)[0].ldr for c in ("steane-0", "rm15-0", "steane-3", "steane-7")] == [8, 9, 11, 16]
    assert [-(-program(c)[0].num_locations // 512) for c in ("steane-0", "steane-3", "steane-7", "rm15-0")] == [4, 6, 8, 8]
    assert sum(CASES[c][3] != 0 for c in CASES) == 1 and sum(CASES[c][6] != 0 for c in CASES) == 2


@pytest.mark.parametrize("case", sorted(CASES))
def test_counts_equal_the_host_tally_of_the_stored_words(case):
    prog, ref = program(case)
    p, seed, first = CASES[case][4:]
    words, want = device_words(case)
    print("\n%s: %s" % (case, want))
    # not an all-rejected run: accepted, rejected, wrong, right and split samples, and unmatched keys where the table can miss
    assert 0 < want['accepted'] < COUNT and 0 < want['wrong'] < want['accepted'] and want['split_vote'] > 0
    assert want['first_trial_wrong'] > 0 and want['trial_wrong'] > want['wrong']
    assert (want['unmatched_x'] > 0) == (case == "rm15-0") and want['unmatched_z'] == 0
    assert tuple(want[f] for f in FIELDS) == REFERENCE_COUNTS[case]
    got = prog.measurement_error_rates(COUNT, *p, seed=seed, first_sample=first)
    assert got == want
    # the restatement's tally agrees on a slice of the words (its classification is Python per distinct word)
    head = ref.tally(words[:20480])[0]
    assert [prog.tally_host(words[:20480])[f] for f in FIELDS] == head


def test_adjacent_ranges_add_up_and_tiny_counts():
    prog, ref = program("steane-3")
    p, seed, first = CASES["steane-3"][4:]
    _, want = device_words("steane-3")
    parts = [prog.measurement_error_rates(n, *p, seed=seed, first_sample=first + start) for start, n in ((0, 100001), (100001, COUNT - 100001))]
    assert [parts[0][f] + parts[1][f] for f in FIELDS] == [want[f] for f in FIELDS]
    assert [prog.measurement_error_rates(0, *p, seed=seed)[f] for f in FIELDS] == [0] * 7
    words = prog.outcomes(3, *DENSE, seed=seed, first_sample=first)
    for i in range(3):                                                               # count = 1, sample by sample
        one = prog.measurement_error_rates(1, *DENSE, seed=seed, first_sample=first + i)
        assert [one[f] for f in FIELDS] == ref.tally(words[i:i + 1])[0]
    assert prog.outcomes(0, *p).shape == (0, prog.ldr)
    quiet = prog.measurement_error_rates(5000, 0.0, 0.0, 0.0, seed=3)
    assert [quiet[f] for f in FIELDS] == [5000, 0, 0, 0, 0, 0, 0]


def test_code_level_entry_points():
    code = make_code("steane")
    p, seed, first = CASES["steane-3"][4:]
    got = code.logical_program_error_rates("XXX", COUNT, *p, seed=seed, first_sample=first)
    assert got == device_words("steane-3")[1]
    classes, wrong = code.logical_program_single_faults("XXX")
    assert classes.shape == (2584, 3) and len(wrong) >= 1


def test_old_entry_points_refuse_a_wide_circuit():
    ctx = _native.default_context()
    prog, _ = program("steane-3")
    circ = prog.device()
    assert circ.ldr == 11
    r1, keys1, flips1, r2, keys2, flips2 = prog._tables()
    buf = ctx.alloc(16 * 11 * 8)
    calls = {
        "gf2_circuit_outcomes_dev": lambda: ctx.circuit_outcomes_dev(circ, 0, 0, 16, 0.01, 0.0, 0.0, buf, 11),
        "gf2_mc_circuit_run": lambda: ctx.mc_circuit_run(circ, r1, r2, 0, 0, 16, 0.01, 0.0, 0.0, _native.HIST_WEIGHT),
        "gf2_mc_circuit_decode": lambda: ctx.mc_circuit_decode(circ, r1, keys1, flips1, r2, keys2, flips2, 0, 0, 16, 0.01, 0.0, 0.0),
        "gf2_mc_circuit_decode_strata": lambda: ctx.mc_circuit_decode_strata(circ, r1, keys1, flips1, r2, keys2, flips2, 0, 0, [1], [16], 1.0, 1.0, 1.0),
        "gf2_mc_ec_decode": lambda: ctx.mc_ec_decode(circ, 1, r1, keys1, flips1, r2, keys2, flips2, 0, 0, 16, 0.01, 0.0, 0.0),
        "gf2_circuit_enumerate": lambda: ctx.circuit_enumerate(circ, r1, keys1, flips1, r2, keys2, flips2, 1, 0, 16),
    }
    for name, call in calls.items():
        with pytest.raises(_native.GF2Error, match=name) as refused:
            call()
        assert refused.value.code == _native.GF2_E_ARG, name
    buf.free()
    with pytest.raises(_native.GF2Error, match="ldr <= 8"):                          # gf2_circuit_create itself still stops at 8
        ctx.circuit_create(prog.effects)
    with pytest.raises(_native.GF2Error, match="gf2_ft_circuit_create: needs 1 <= ldr <= 16"):
        ctx.ft_circuit_create(np.zeros((4, 2, 17), dtype=np.uint64))


def test_argument_errors():
    ctx = _native.default_context()
    prog, _ = program("steane-3")
    circ = prog.device()
    r1, keys1, flips1, r2, keys2, flips2 = prog._tables()
    run = lambda c, nsteps, mask, a, b: ctx.mc_ft_decode(c, nsteps, mask, a, keys1, flips1, b, keys2, flips2, 0, 0, 10, 0.001, 0.0, 0.0)
    small = ctx.ft_circuit_create(np.zeros((4, 2, 7), dtype=np.uint64))
    for c, nsteps, mask, a, b, text in ((circ, 9, 0b10101000, 32, 3, "r_1, r_2 <= 31"), (circ, 9, 0b10101000, 3, 32, "r_1, r_2 <= 31"),
                                        (circ, 9, 0b00101000, 3, 3, "odd number of trials"), (circ, 9, 1 << 9, 3, 3, "at or above nsteps"),
                                        (circ, 11, 0b10101000, 3, 3, "F >= 1"), (circ, 0, 0, 3, 3, "nsteps >= 1"),
                                        (circ, 9, 0b10101000, 2, 3, "bits beyond the layout"), (circ, 9, 0b10100100, 3, 3, "bits beyond the layout"),
                                        (circ, 9, 0b100101000, 3, 3, "bits beyond the layout"), (small, 6, 0b10101, 3, 3, "8 <= ldr <= 16")):
        with pytest.raises(_native.GF2Error, match=text):
            run(c, nsteps, mask, a, b)
    with pytest.raises(_native.GF2Error, match="negative range"):
        ctx.mc_ft_decode(circ, 9, 0b10101000, r1, keys1, flips1, r2, keys2, flips2, 0, -1, 10, 0.001, 0.0, 0.0)
    with pytest.raises(_native.GF2Error, match="occurs twice"):
        ctx.mc_ft_decode(circ, 9, 0b10101000, r1, np.array([1, 1], dtype=np.uint64), np.zeros(2, np.uint8), r2, keys2, flips2, 0, 0, 10, 0.001, 0.0, 0.0)
    buf = ctx.alloc(16 * 11 * 8)
    with pytest.raises(_native.GF2Error, match="ldo must be at least"):
        ctx.ft_outcomes_dev(circ, 0, 0, 16, 0.001, 0.0, 0.0, buf, 10)
    # a narrow circuit made by gf2_ft_circuit_create is stored by the old kernel: the same words as gf2_circuit_outcomes_dev
    eff = np.arange(4 * 2 * 7, dtype=np.uint64).reshape(4, 2, 7)
    a, b = ctx.ft_circuit_create(eff), ctx.circuit_create(eff)
    outs = []
    for store, c in ((ctx.ft_outcomes_dev, a), (ctx.circuit_outcomes_dev, b)):
        store(c, 5, 0, 16, 0.2, 0.1, 0.2, buf, 7)
        outs.append(buf.download((16, 7), np.uint64))
    assert np.array_equal(outs[0], outs[1]) and outs[0].any()
    buf.free()
