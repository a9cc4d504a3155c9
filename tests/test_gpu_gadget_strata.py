"""
Sampled strata of the two post-selected gadgets on the GPU (DESIGN.md sections 5b "Sampled strata of the cycle" and 5c "Sampled strata
of the measurement"): gadget_strata_kernel (csrc/gf2_gadget_strata.hip) through gf2_mc_ec_decode_strata / gf2_mc_ft_decode_strata,
ECCircuit / FTProgram.strata and CSSCode.error_correct_strata / logical_program_strata.  Every comparison of counts is exact.

  host statement  the device against gf2_stratum_outcomes_host followed by gf2_ec_tally_host / gf2_ft_tally_host, count for count, and
                  against the literals of tests/test_gadget_strata.py (re-derived with the NumPy restatement)
  instantiations  every (LDR, rule, staged) of the kernel on synthetic effect tables
  counts add      sample ranges in pieces, strata together and apart, empty strata, weight 16 of 17 locations
  entry points    the public methods, the merge with the exact strata, the single-fault census within 5 sigma
  refusals        every argument error of the two entry points, one by one

Every test runs under a time limit of its own, none provokes a fault.
"""
import faulthandler
import math

import numpy as np
import pytest

from quantum_css_codes_amd import _native, ec_noise, ft_noise, montecarlo
from tests.test_gadget_strata import CYCLE_LITERAL, LITERAL_SAMPLES, PROGRAM_LITERAL
from tests.test_gpu_strata import make_code

pytestmark = pytest.mark.gpu

SEED0 = 20261018 + 900
TIME_LIMIT = 600                                                             # seconds per test
EC, FT = ec_noise.EC_FIELDS, ft_noise.FT_FIELDS
WEIGHTS = [0, 1, 2, 3, 8, 16]
STAGE_LIMIT = 20480                                                          # bytes: effect tables up to this size are staged in LDS


@pytest.fixture(autouse=True)
def own_time_limit():
    faulthandler.dump_traceback_later(TIME_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def cycle(rounds):
    return ec_noise.circuit_for(make_code("steane"), rounds)


def program(name, ops):
    return ft_noise.program_for(make_code(name), ops)


# ---- 1: the device against the host statement ------------------------------------------------------------------------------------

GADGETS = {"cycle-1": lambda: cycle(1), "cycle-5": lambda: cycle(5), "steane-gate-free": lambda: program("steane", ""),
           "steane-XXX": lambda: program("steane", "XXX"), "rm15-gate-free": lambda: program("rm15", "")}
LAYOUT = {"cycle-1": (3, True), "cycle-5": (8, False), "steane-gate-free": (8, False), "steane-XXX": (11, False), "rm15-gate-free": (9, False)}


@pytest.mark.parametrize("name", list(GADGETS))
def test_device_counts_are_the_host_statement(name):
    gadget = GADGETS[name]()
    ldr, staged = LAYOUT[name]
    assert gadget.ldr == ldr and (gadget.effects.nbytes <= STAGE_LIMIT) == staged
    got = gadget.strata(WEIGHTS, 1 << 16, kinds=(2, 1, 3), seed=SEED0, first_sample=12345)
    want = gadget.strata(WEIGHTS, 1 << 16, kinds=(2, 1, 3), seed=SEED0, first_sample=12345, host=True)
    assert isinstance(got, montecarlo.SampledPostSelectedStrata) and got.fields == want.fields and got.nb == gadget.num_locations
    assert np.array_equal(got.counts, want.counts), (got.counts.tolist(), want.counts.tolist())
    assert int(got.counts[0, 0]) == 1 << 16 and 0 < int(got.counts[3, 0]) < 1 << 16


def test_the_committed_literals():
    got = cycle(1).strata([2], LITERAL_SAMPLES)
    assert got.counts[0].tolist() == CYCLE_LITERAL
    got = program("steane", "").strata([2], LITERAL_SAMPLES)
    assert got.counts[0].tolist() == PROGRAM_LITERAL


# ---- 2: every instantiation on synthetic effect tables -----------------------------------------------------------------------------

def synthetic_tables(rng, keys_x, keys_z):
    """Tables 1 (key_z) and 2 (key_x) holding half of the keys that occur."""
    out = []
    for keys in (keys_z, keys_x):
        half = np.ascontiguousarray(np.unique(keys)[::2]).astype("<u8")
        out += [half, rng.integers(0, 2, len(half), dtype=np.uint8)]
    return out


def flag_words(rng, locations, nflag):
    """Sparse flag bits: a tenth of the effects trip one of two verifications, so that samples of sixteen faults are still accepted
    now and then, and two faults can hide each other."""
    words = np.zeros((locations, 2, nflag), dtype="<u8")
    hit = rng.random((locations, 2)) < 0.1
    words[hit, rng.integers(0, nflag, int(hit.sum()))] = rng.integers(1, 3, int(hit.sum())).astype(np.uint64)
    return words


def synthetic_cycle(rng, r1, r2, rounds, nflag, locations):
    eff = np.zeros((locations, 2, 1 + rounds + nflag), dtype="<u8")
    key_x = rng.integers(0, 1 << r2, (locations, 2, 1 + rounds)).astype(np.uint64)
    key_z = rng.integers(0, 1 << r1, (locations, 2, 1 + rounds)).astype(np.uint64)
    eff[:, :, :1 + rounds] = key_x | key_z << np.uint64(32)
    eff[:, :, 0] |= rng.integers(0, 2, (locations, 2)).astype(np.uint64) << np.uint64(31) | rng.integers(0, 2, (locations, 2)).astype(np.uint64) << np.uint64(63)
    eff[:, :, 1 + rounds:] = flag_words(rng, locations, nflag)
    return eff, synthetic_tables(rng, key_x, key_z)


def synthetic_program(rng, r1, r2, nsteps, mask, nflag, locations):
    eff = np.zeros((locations, 2, nsteps + nflag), dtype="<u8")
    key_x = rng.integers(0, 1 << r2, (locations, 2, nsteps)).astype(np.uint64)
    key_z = rng.integers(0, 1 << r1, (locations, 2, nsteps)).astype(np.uint64)
    for s in range(nsteps):
        if (mask >> s) & 1:
            eff[:, :, s] = key_x[:, :, s] | rng.integers(0, 2, (locations, 2)).astype(np.uint64) << np.uint64(31)
        else:
            eff[:, :, s] = key_x[:, :, s] | key_z[:, :, s] << np.uint64(32)
    eff[:, :, nsteps:] = flag_words(rng, locations, nflag)
    return eff, synthetic_tables(rng, key_x, key_z)


#              rounds, flag words -> LDR 3 .. 8
CYCLE_CASES = [(1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1), (1, 3), (2, 5)]
#                nsteps, measure_mask, flag words -> LDR 8 .. 16
PROGRAM_CASES = [(7, 0b0010101, 1), (7, 0b1000000, 2), (9, 0b001010100, 1), (8, 0b00101010, 3), (11, 0b00101010101, 1), (12, 0b000000010101, 1),
                 (13, 0b0101010000000, 1), (13, 0b1010101010101, 2), (15, 0b001010101010101, 1)]
CYCLE_LOCATIONS, PROGRAM_LOCATIONS = (40, 500), (500,)
SYNTHETIC_WEIGHTS, SYNTHETIC_SAMPLES = [1, 5, 16], 1 << 14


def test_cases_cover_the_kernel_instantiations():
    staged = {(1 + r + f, 2 * loc * (1 + r + f) * 8 <= STAGE_LIMIT) for r, f in CYCLE_CASES for loc in CYCLE_LOCATIONS}
    assert staged == {(ldr, s) for ldr in range(3, 9) for s in (True, False)}
    assert {r for r, _ in CYCLE_CASES} == set(range(1, ec_noise.MAX_ROUNDS + 1))
    assert all(2 * 500 * ldr * 8 > STAGE_LIMIT and 2 * 40 * ldr * 8 <= STAGE_LIMIT for ldr in range(3, 9))
    assert {s + f for s, _, f in PROGRAM_CASES} == set(range(8, ft_noise.MAX_LDR + 1))
    assert all(bin(m).count("1") % 2 == 1 and m >> s == 0 for s, m, _ in PROGRAM_CASES)


def check_synthetic(device_fn, host_tally, eff):
    first = 777
    got = device_fn(first, SYNTHETIC_WEIGHTS, [SYNTHETIC_SAMPLES] * len(SYNTHETIC_WEIGHTS), (1, 2, 1))
    want = np.array([host_tally(_native.stratum_outcomes_host(eff, w, SYNTHETIC_SAMPLES, (1, 2, 1), SEED0, first)) for w in SYNTHETIC_WEIGHTS])
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    return got


@pytest.mark.parametrize("case", CYCLE_CASES, ids=lambda c: "rounds%d-ldr%d" % (c[0], 1 + c[0] + c[1]))
def test_every_cycle_instantiation(case):
    rounds, nflag = case
    ctx = _native.default_context()
    rng = np.random.default_rng(SEED0 + 16 * rounds + nflag)
    r1, r2 = 5, 4
    for locations in CYCLE_LOCATIONS:
        eff, tables = synthetic_cycle(rng, r1, r2, rounds, nflag, locations)
        circ = ctx.circuit_create(eff)
        args = (rounds, r1, tables[0], tables[1], r2, tables[2], tables[3])
        got = check_synthetic(lambda first, ws, ns, ks: ctx.mc_ec_decode_strata(circ, *args, SEED0, first, ws, ns, *ks),
                              lambda words: _native.ec_tally_host(words, *args), eff)
        assert got.shape == (3, len(EC)) and (got[:, 0] > 0).all() and (got[:, 0] < SYNTHETIC_SAMPLES).all(), (case, locations)
        assert got[:, 3].min() > 0 and got[:, 6:].max() > 0                  # flips and unmatched round keys occur
        circ.free()


@pytest.mark.parametrize("case", PROGRAM_CASES, ids=lambda c: "steps%d-ldr%d" % (c[0], c[0] + c[2]))
def test_every_measurement_instantiation(case):
    nsteps, mask, nflag = case
    ctx = _native.default_context()
    rng = np.random.default_rng(SEED0 + 32 * nsteps + nflag)
    r1, r2 = 4, 5
    for locations in PROGRAM_LOCATIONS:
        eff, tables = synthetic_program(rng, r1, r2, nsteps, mask, nflag, locations)
        circ = ctx.ft_circuit_create(eff)
        args = (nsteps, mask, r1, tables[0], tables[1], r2, tables[2], tables[3])
        got = check_synthetic(lambda first, ws, ns, ks: ctx.mc_ft_decode_strata(circ, *args, SEED0, first, ws, ns, *ks),
                              lambda words: _native.ft_tally_host(words, *args), eff)
        assert got.shape == (3, len(FT)) and (got[:, 0] > 0).all() and (got[:, 0] < SYNTHETIC_SAMPLES).all(), (case, locations)
        assert got[:, 1].min() > 0 and got[:, 5].max() > 0
        circ.free()


# ---- 3: counts add -------------------------------------------------------------------------------------------------------------------

def test_counts_add():
    for gadget in (cycle(2), program("steane", "X")):
        whole = gadget.strata([3, 8], 100001, seed=SEED0 + 3, first_sample=50)
        parts = [gadget.strata([3, 8], n, seed=SEED0 + 3, first_sample=first) for first, n in ((50, 1), (51, 40000), (40051, 60000))]
        assert np.array_equal(parts[0].counts + parts[1].counts + parts[2].counts, whole.counts)
        apart = np.concatenate([gadget.strata([w], 100001, seed=SEED0 + 3, first_sample=50).counts for w in (3, 8)])
        assert np.array_equal(apart, whole.counts)
        # one first sample per stratum: two native calls
        mixed = gadget.strata([3, 8], [100001, 60000], seed=SEED0 + 3, first_sample=[50, 40051])
        assert np.array_equal(mixed.counts[0], whole.counts[0]) and np.array_equal(mixed.counts[1], parts[2].counts[1])
        empty = gadget.strata([3, 5, 8], [0, 300, 0], seed=SEED0 + 3)
        assert not empty.counts[[0, 2]].any() and int(empty.counts[1, 0]) > 0
        assert not gadget.strata([3, 5], 0).counts.any() and gadget.strata([], 10).counts.shape == (0, len(gadget.strata([], 10).fields))


def test_weight_16_of_17_locations():
    ctx = _native.default_context()
    rng = np.random.default_rng(SEED0 + 4)
    eff, tables = synthetic_cycle(rng, 3, 3, 1, 1, 17)
    circ = ctx.circuit_create(eff)
    args = (1, 3, tables[0], tables[1], 3, tables[2], tables[3])
    got = ctx.mc_ec_decode_strata(circ, *args, SEED0, 0, [16, 15], [5000, 5000], 1.0, 1.0, 1.0)
    want = [_native.ec_tally_host(_native.stratum_outcomes_host(eff, w, 5000, (1, 1, 1), SEED0, 0), *args) for w in (16, 15)]
    assert np.array_equal(got, np.array(want)) and int(got[0, 0]) > 0
    with pytest.raises(_native.GF2Error, match=r"weight 17 outside \[0, min\(L = 17, 16\)\]"):
        ctx.mc_ec_decode_strata(circ, *args, SEED0, 0, [17], [10], 1.0, 1.0, 1.0)
    circ.free()


# ---- 4: public entry points ----------------------------------------------------------------------------------------------------------

def test_public_entry_points():
    code = make_code("steane")
    exact = code.logical_program_strata_exact('XXX', [0, 1])
    sampled = code.logical_program_strata('XXX', [2, 3, 4], 1 << 15, seed=SEED0 + 5)
    assert isinstance(sampled, montecarlo.SampledPostSelectedStrata) and sampled.fields == FT and sampled.nb == 2584
    merged = exact.merged(sampled)
    assert isinstance(merged, montecarlo.MergedPostSelectedStrata)
    estimate, lower, upper = exact.rate(1e-3, (1, 1, 1), 'wrong')
    got = merged.rate(1e-3, 'wrong')
    assert lower <= got.lower <= got.estimate <= got.upper <= upper and got.stderr > 0
    assert got.upper - got.lower < 0.5 * (upper - lower)
    ec_exact = code.error_correct_strata_exact([0, 1, 2])
    ec_sampled = code.error_correct_strata([3, 4], 1 << 15, rounds=1, seed=SEED0 + 5)
    assert ec_sampled.fields == EC and ec_sampled.nb == 330
    estimate, lower, upper = ec_exact.rate(1e-3, (1, 1, 1), 'logical_any')
    got = ec_exact.merged(ec_sampled).rate(1e-3, 'logical_any')
    assert lower <= got.lower <= got.estimate <= got.upper <= upper and got.stderr > 0
    alone = montecarlo.gadget_strata_sharded(ec_noise.circuit_for(code, 1), [3, 4], 1 << 15, seed=SEED0 + 5)   # no process group: the one shard
    assert np.array_equal(alone.counts, ec_sampled.counts) and alone.samples.tolist() == [1 << 15] * 2


def test_single_faults_sampled_agree_with_the_census():
    """Stratum 1 of Steane `X X X MEASURE`, kinds (1, 1, 1): 3032 of the 7752 single faults are accepted and 15 make the bit wrong
    (DESIGN.md 5c).  2^16 samples must lie within 5 sigma = 5 sqrt(f (1 - f) / N) of both fractions: a correct sampler misses with
    probability 6e-7 per comparison.  With this seed the host statement gives accepted 25511 (z = -0.97) and wrong 133 (z = +0.55)."""
    n = 1 << 16
    got = make_code("steane").logical_program_strata('XXX', [1], n, seed=SEED0 + 6)
    want = program("steane", "XXX").strata([1], n, seed=SEED0 + 6, host=True)
    assert np.array_equal(got.counts, want.counts)
    for col, census in ((0, 3032), (1, 15)):
        f = census / 7752
        sigma = math.sqrt(f * (1 - f) / n)
        print("census %d/7752 = %.6f sampled %d/%d = %.6f sigma %.2e" % (census, f, int(got.counts[0, col]), n, int(got.counts[0, col]) / n, sigma))
        assert abs(int(got.counts[0, col]) / n - f) <= 5 * sigma


# ---- 5: refusals -----------------------------------------------------------------------------------------------------------------------

def test_refusals_of_the_cycle_entry_point():
    code = make_code("steane")
    ctx = _native.default_context()
    circ = ec_noise.circuit_for(code, 1)
    r1, keys1, flips1, r2, keys2, flips2 = tables = circ._tables()
    dev = circ.device()

    def call(circuit=dev, rounds=1, tables=tables, first=0, weights=(1,), counts=(10,), kinds=(1.0, 1.0, 1.0)):
        return ctx.mc_ec_decode_strata(circuit, rounds, *tables, SEED0, first, list(weights), list(counts), *kinds)

    rng = np.random.default_rng(SEED0 + 7)
    five = rng.integers(0, 1 << 62, (30, 2, 5)).astype("<u8")              # the Monte-Carlo layout is no cycle: its effects leave the layout
    five_dev = ctx.circuit_create(five)
    program_dev = ft_noise.program_for(code, "XXX").device()                 # 11 words
    for fn, text in ((lambda: call(tables=(32, keys1, flips1, r2, keys2, flips2)), "<= 31"), (lambda: call(tables=(r1, keys1, flips1, 0, keys2, flips2)), "<= 31"),
                     (lambda: call(rounds=0), "rounds <= 6"), (lambda: call(rounds=7), "rounds <= 6"),
                     (lambda: call(program_dev, rounds=6), "ldr <= 8"), (lambda: call(rounds=2), "rounds need"),
                     (lambda: call(five_dev, rounds=2), "beyond"),
                     (lambda: call(tables=(r1, np.append(keys1, keys1[:1]), np.append(flips1, 0), r2, keys2, flips2)), "twice"),
                     (lambda: call(weights=[1] * 257, counts=[1] * 257), "nstrata <= 256"),
                     (lambda: call(weights=[17]), r"weight 17 outside \[0, min\(L = 330, 16\)\]"), (lambda: call(weights=[2, -1], counts=[1, 1]), "stratum 1 has weight -1"),
                     (lambda: call(counts=[-1]), "negative sample count"), (lambda: call(first=-1), "negative range"),
                     (lambda: call(kinds=(0.0, 0.0, 0.0)), "kind weights"), (lambda: call(kinds=(1.0, -1.0, 1.0)), "kind weights")):
        with pytest.raises(_native.GF2Error, match=text) as err:
            fn()
        assert err.value.code == _native.GF2_E_ARG and "gf2_mc_ec_decode_strata" in err.value.message, text
    five_dev.free()
    assert call(weights=[], counts=[]).shape == (0, 8) and not call(counts=[0]).any()
    for bad in (lambda: circ.strata([17], 10), lambda: circ.strata([1], -1), lambda: circ.strata([1], 10, kinds=(0, 0, 0))):
        with pytest.raises(ValueError):
            bad()


def test_refusals_of_the_measurement_entry_point():
    code = make_code("steane")
    ctx = _native.default_context()
    prog = ft_noise.program_for(code, "")
    r1, keys1, flips1, r2, keys2, flips2 = tables = prog._tables()
    dev = prog.device()

    def call(circuit=dev, nsteps=prog.nsteps, mask=prog.measure_mask, tables=tables, first=0, weights=(1,), counts=(10,), kinds=(1.0, 1.0, 1.0)):
        return ctx.mc_ft_decode_strata(circuit, nsteps, mask, *tables, SEED0, first, list(weights), list(counts), *kinds)

    assert (prog.ldr, prog.nsteps, prog.measure_mask) == (8, 6, 0b010101)
    cycle_dev = ec_noise.circuit_for(code, 1).device()                       # the cycle's 3 words are no program
    rng = np.random.default_rng(SEED0 + 8)
    wide = ctx.ft_circuit_create(rng.integers(0, 1 << 62, (30, 2, 8)).astype("<u8"))
    for fn, text in ((lambda: call(tables=(r1, keys1, flips1, 32, keys2, flips2)), "<= 31"), (lambda: call(cycle_dev, nsteps=2, mask=0b01), "8 <= ldr"),
                     (lambda: call(nsteps=0, mask=0), "nsteps >= 1"), (lambda: call(nsteps=8, mask=0b010101), "F >= 1"),
                     (lambda: call(mask=1 << 6), "at or above nsteps"), (lambda: call(mask=0b010100), "odd number"),
                     (lambda: call(wide), "beyond"),
                     (lambda: call(tables=(r1, keys1, flips1, r2, np.append(keys2, keys2[:1]), np.append(flips2, 0))), "twice"),
                     (lambda: call(weights=[1] * 257, counts=[1] * 257), "nstrata <= 256"),
                     (lambda: call(weights=[17]), r"weight 17 outside \[0, min\(L = 1585, 16\)\]"), (lambda: call(weights=[-1]), "weight -1 outside"),
                     (lambda: call(counts=[-1]), "negative sample count"), (lambda: call(first=-1), "negative range"),
                     (lambda: call(kinds=(0.0, 0.0, 0.0)), "kind weights"), (lambda: call(kinds=(float("inf"), 1.0, 1.0)), "kind weights")):
        with pytest.raises(_native.GF2Error, match=text) as err:
            fn()
        assert err.value.code == _native.GF2_E_ARG and "gf2_mc_ft_decode_strata" in err.value.message, text
    wide.free()
    assert call(weights=[], counts=[]).shape == (0, 7) and not call(counts=[0]).any()
