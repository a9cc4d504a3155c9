"""
The error-correction cycle on the GPU (quantum_css_codes_amd/ec_noise.py, csrc/gf2_ec.hip).  Every comparison
is exact, against tests/ec_ref.py: the faults of the oracle's sampler run over the L locations (c_oracle.sample_errors with
n := L), forward propagation with RESET and timed rows, quil_classical_correct on a vector of known errors with the code's own
table dicts.  A case's reference is computed once and shared by the test of the outcome words and the test of the counts.

The cases are the smallest shapes at which gf2_mc_ec_decode takes another path: every LDR from 3 to 8 that a cycle of the two test
codes has, the effect table staged in LDS and read through L2, one and several sampler segments, one and two flag words,
r_1 != r_2, final frames the table does not hold, several faults per segment (Floyd's map) and 11-bit keys with capped tables.
"""
import functools

import numpy as np
import pytest

from oracle import c_oracle, cpu_ref
from quantum_css_codes_amd import _native, css_code, ec_noise
from quantum_css_codes_amd.css_code import CSSCode
from tests import ec_ref

pytestmark = pytest.mark.gpu

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
FIELDS = ec_noise.EC_FIELDS

#        code, rounds, (p_x, p_y, p_z), samples, seed, first_sample
CASES = {
    "steane-1": ("steane", 1, (0.002, 0.001, 0.002), 100003, 1, 0),               # LDR 3, staged, one segment
    "steane-2": ("steane", 2, (0.002, 0.001, 0.002), 100003, 2, 5),               # L = 660: two segments; 42 KB of effects: unstaged
    "steane-4": ("steane", 4, (0.001, 0.0005, 0.001), 100000, 3, 0),              # LDR 6
    "steane-5": ("steane", 5, (0.001, 0.0005, 0.001), 100000, 4, 1 << 33),        # F = 2, LDR 8
    "rm15-1": ("rm15", 1, (0.001, 0.0005, 0.001), 100000, 5, 0),                  # LDR 3; r_1 != r_2; final misses occur
    "rm15-3": ("rm15", 3, (0.001, 0.0005, 0.001), 100000, 6, 7),                  # F = 2, LDR 6
    "steane-1-dense": ("steane", 1, (0.01, 0.0, 0.02), 100000, 7, 0),             # several faults per segment, Floyd's map
    "pair23-1": ("pair23", 1, (0.0006, 0.0003, 0.0006), 100000, 8, 0),            # max_table_weight set; wide keys
}


def full_rank(mat):
    return np.count_nonzero(cpu_ref.reduced_row_echelon_form(mat).any(axis=1)) == mat.shape[0]


def dual_pair(rng, n, r1):
    """H1 (r1 x n, full rank) and all but one row of a random basis of its dual: a k = 1 CSS pair.  (The basis is mixed first: the
    nullspace comes in standard form, and dropping a row of that would leave H2 a zero column, a code that corrects nothing.)"""
    while True:
        h1 = rng.integers(0, 2, (r1, n))
        if full_rank(h1):
            break
    null = cpu_ref.nullspace(h1)
    while True:
        mix = rng.integers(0, 2, (len(null), len(null)))
        if full_rank(mix):
            break
    return h1, ((mix @ null) % 2)[:-1]


def checks_of(name):
    if name == "steane":
        return STEANE, STEANE, None
    if name == "rm15":
        cols = np.arange(1, 16)
        h1 = np.array([(cols >> b) & 1 for b in range(4)])
        return h1, np.vstack([h1] + [h1[a] & h1[b] for a in range(4) for b in range(a + 1, 4)]), None
    return dual_pair(np.random.default_rng(23), 23, 11) + (1,)


@functools.lru_cache(maxsize=None)
def make_code(name):
    h1, h2, cap = checks_of(name)
    return CSSCode(h1, h2, max_table_weight=cap)


@functools.lru_cache(maxsize=None)
def cycle(name, rounds):
    code = make_code(name)
    return ec_noise.circuit_for(code, rounds), ec_ref.Cycle(code, rounds)


def reference_words(ref, seed, first, count, p, chunk=16384):
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
    return np.concatenate(parts) if parts else np.zeros((0, ref.ldr), dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def reference(case):
    """(outcome words, counts) of a case under the restatement alone; computed once, never modified."""
    name, rounds, p, count, seed, first = CASES[case]
    circ, ref = cycle(name, rounds)
    words = reference_words(ref, seed, first, count, p)
    words.setflags(write=False)
    counts, _ = ref.tally(words)
    return words, tuple(counts)


@pytest.mark.parametrize("case", sorted(CASES))
def test_outcome_words_equal_the_restatement(case):
    name, rounds, p, count, seed, first = CASES[case]
    circ, ref = cycle(name, rounds)
    assert (circ.num_locations, circ.ldr) == (ref.locations, ref.ldr)
    want, _ = reference(case)
    got = circ.outcomes(count, *p, seed=seed, first_sample=first)
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("case", sorted(CASES))
def test_counts_equal_the_restatement(case):
    name, rounds, p, count, seed, first = CASES[case]
    circ, ref = cycle(name, rounds)
    _, want = reference(case)
    print("\n%s: %s" % (case, dict(zip(FIELDS, want))))
    assert want[0] >= 500 and want[1] >= 10 and want[2] >= 10, "the case must keep 500 accepted samples and 10 flips per side"
    got = circ.logical_error_rates(count, *p, seed=seed, first_sample=first)
    assert [got[f] for f in FIELDS] == list(want) and got['samples'] == count


def test_cases_cover_the_kernel_paths():
    staged = lambda circ: circ.effects.nbytes <= 20480
    assert [cycle("steane", r)[0].ldr for r in (1, 2, 4, 5)] == [3, 4, 6, 8] and [cycle("rm15", r)[0].ldr for r in (1, 3)] == [3, 6]
    assert staged(cycle("steane", 1)[0]) and not staged(cycle("steane", 2)[0])
    assert cycle("steane", 1)[0].num_locations <= 512 < cycle("steane", 2)[0].num_locations
    assert reference("rm15-1")[1][4] + reference("rm15-1")[1][5] > 0                 # final frames outside the tables
    code = make_code("pair23")
    assert (code.r_1, code.r_2, code.t) == (11, 11, 1) and len(code._c1_syndromes) == len(code._c2_syndromes) == 24


def test_no_faults_no_failures():
    for name, rounds in (("steane", 1), ("steane", 5), ("rm15", 3)):
        got = cycle(name, rounds)[0].logical_error_rates(5000, 0.0, 0.0, 0.0, seed=3)
        assert [got[f] for f in FIELDS] == [5000, 0, 0, 0, 0, 0, 0, 0]


def test_shards_add_up_and_tiny_counts():
    name, rounds, p, count, seed, first = CASES["steane-2"]
    circ, ref = cycle(name, rounds)
    _, want = reference("steane-2")
    parts = [circ.logical_error_rates(n, *p, seed=seed, first_sample=first + start) for start, n in ((0, 40001), (40001, count - 40001))]
    assert [parts[0][f] + parts[1][f] for f in FIELDS] == list(want)
    assert [circ.logical_error_rates(0, *p, seed=seed)[f] for f in FIELDS] == [0] * 8
    words = circ.outcomes(3, *p, seed=seed, first_sample=first)
    for i in range(3):                                                               # count = 1, sample by sample
        one = circ.logical_error_rates(1, *p, seed=seed, first_sample=first + i)
        assert [one[f] for f in FIELDS] == ref.tally(words[i:i + 1])[0]
    assert circ.outcomes(0, *p).shape == (0, circ.ldr)


def test_code_level_entry_points():
    code = make_code("steane")
    name, rounds, p, count, seed, first = CASES["steane-2"]
    got = code.error_correct_logical_error_rates(count, *p, rounds=rounds, seed=seed, first_sample=first)
    assert [got[f] for f in FIELDS] == list(reference("steane-2")[1])
    assert code.error_correct_gates(2).gates.tolist() == cycle("steane", 2)[1].gates.tolist()
    classes, flipping = code.error_correct_single_faults()
    assert classes.shape == (330, 3) and len(flipping) >= 1
    tallied = cycle("steane", 2)[0].tally_host(reference("steane-2")[0])
    assert [tallied[f] for f in FIELDS] == list(reference("steane-2")[1])
    idle = code.error_correct_logical_error_rates(20000, *p, rounds=1, seed=9, idle_data=True)
    ref = ec_ref.Cycle(code, 1, idle_data=True)
    assert [idle[f] for f in FIELDS] == ref.tally(reference_words(ref, 9, 0, 20000, p))[0]


def test_reset_stays_out_of_the_conjugation():
    # (a GPU test: transform_stabilisers has no host check of the kinds -- gf2_conjugate_gates refuses a gate when conjugate_kernel
    # reaches it, and the ValueError is made from the code and the gate index that call returns)
    with pytest.raises(ValueError, match="cannot conjugate gate 3"):
        css_code.transform_stabilisers(np.identity(4, dtype=int), np.array([(0, 0, 0), (3, 1, 0)], dtype=np.int32))


def test_argument_errors():
    ctx = _native.default_context()
    circ = cycle("steane", 1)[0]
    r1, keys1, flips1, r2, keys2, flips2 = circ._tables()
    run = lambda c, rounds, a, b: ctx.mc_ec_decode(c, rounds, a, keys1, flips1, b, keys2, flips2, 0, 0, 10, 0.01, 0.0, 0.0)
    for c, rounds, a, b, text in ((circ.device(), 1, 32, 3, "r_1, r_2 <= 31"), (circ.device(), 1, 3, 32, "r_1, r_2 <= 31"),
                                  (circ.device(), 0, 3, 3, "1 <= rounds <= 6"), (circ.device(), 7, 3, 3, "1 <= rounds <= 6"),
                                  (circ.device(), 2, 3, 3, "1 . rounds . F"), (circ.device(), 1, 2, 3, "bits beyond")):
        with pytest.raises(_native.GF2Error, match=text):
            run(c, rounds, a, b)
    with pytest.raises(_native.GF2Error, match="ldr <= 8"):                          # ldr = 9: no such circuit can be made
        ctx.circuit_create(np.zeros((4, 2, 9), dtype=np.uint64))
    with pytest.raises(_native.GF2Error, match="negative range"):
        ctx.mc_ec_decode(circ.device(), 1, r1, keys1, flips1, r2, keys2, flips2, 0, -1, 10, 0.01, 0.0, 0.0)
    with pytest.raises(_native.GF2Error, match="occurs twice"):
        ctx.mc_ec_decode(circ.device(), 1, r1, np.array([1, 1], dtype=np.uint64), np.zeros(2, np.uint8), r2, keys2, flips2, 0, 0, 10, 0.01, 0.0, 0.0)
