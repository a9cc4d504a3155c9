"""
Sampled strata of the two post-selected gadgets on the CPU (DESIGN.md sections 5b "Sampled strata of the cycle" and 5c "Sampled
strata of the measurement"): gf2_stratum_outcomes_host followed by gf2_ec_tally_host / gf2_ft_tally_host (csrc/gf2_host.cpp),
ECCircuit / FTProgram.strata(host=True) and montecarlo.SampledPostSelectedStrata / MergedPostSelectedStrata.

  host statement  against tests/gadget_strata_ref.py (strata_ref.stratum_draws, gadget_enumerate_ref.effect_words, ec_ref / ft_ref's
                  tally), word for word and count for count
  literals        the weight-2 strata of the one-round Steane cycle and of the gate-free Steane program, 2^18 samples
  exact strata    those runs within 5 sigma of the exact weight-2 fractions (gadget_enumerate_ref.pairs)
  estimator       the merge, the ratio, its bounds and its delta-method error; the refusals
  refusals        the argument errors of the three entry points that need no device
"""
import ctypes
import functools
import math

import numpy as np
import pytest

from quantum_css_codes_amd import _native, ec_noise, ft_noise, montecarlo
from quantum_css_codes_amd.montecarlo import MergedPostSelectedStrata, PostSelectedStrata, SampledPostSelectedStrata
from tests import ec_ref, ft_ref
from tests import gadget_enumerate_ref as ger
from tests import gadget_strata_ref as gsr
from tests.test_ft import oracle_code

EC, FT = ec_noise.EC_FIELDS, ft_noise.FT_FIELDS
WEIGHTS = (0, 1, 2, 3, 7, 16)
KINDS = ((1, 1, 1), (1, 0, 0), (2, 1, 3))
SAMPLES = 4096

# Seed 0, first sample 0, kinds (1, 1, 1), w = 2, 2^18 samples: re-derived with tests/gadget_strata_ref.py alone (stratum_counts of
# the restated gadget over its own effect_words); no native code took part.
LITERAL_SAMPLES = 1 << 18
CYCLE_LITERAL = [43616, 4132, 1441, 5454, 0, 0, 0, 0]                        # one-round Steane cycle, L = 330, ldr 3
PROGRAM_LITERAL = [39476, 847, 3071, 373, 1840, 0, 0]                        # gate-free Steane program, L = 1585, ldr 8


@functools.lru_cache(maxsize=None)
def gadget(kind, name, arg):
    """(ECCircuit or FTProgram, the restated gadget, the restatement's effect words): nothing here needs a GPU."""
    code = oracle_code(name)
    if kind == "cycle":
        ref = ec_ref.Cycle(code, arg)
        return ec_noise.ECCircuit(code, arg), ref, ger.effect_words(ref)
    ref = ft_ref.Rewritten(code, arg)
    return ft_noise.FTProgram(code, arg), ref, ger.effect_words(ref)


GADGETS = [("cycle", "steane", 1), ("cycle", "steane", 2), ("program", "steane", ""), ("cycle", "rm15", 1)]


# ---- the host statement against the restatement ----------------------------------------------------------------------------------

@pytest.mark.parametrize("which", GADGETS, ids=lambda g: "%s-%s-%s" % g)
def test_host_statement_is_the_restatement(which):
    native, ref, eff = gadget(*which)
    assert native.num_locations == ref.locations and native.ldr == ref.ldr and np.array_equal(native.effects, eff)
    seen = 0
    for kinds in KINDS:
        for first, seed in ((0, 0), (123457, 11)):
            got = native.strata(WEIGHTS, SAMPLES, kinds=kinds, seed=seed, first_sample=first, host=True)
            assert isinstance(got, SampledPostSelectedStrata) and got.nb == ref.locations and got.fields == (EC if which[0] == "cycle" else FT)
            assert got.samples.tolist() == [SAMPLES] * len(WEIGHTS) and got.weights.tolist() == list(WEIGHTS)
            for w, counts in zip(WEIGHTS, got.counts):
                want_words = gsr.stratum_words(eff, seed, first, SAMPLES, w, kinds)
                words = _native.stratum_outcomes_host(native.effects, w, SAMPLES, kinds, seed, first)
                assert np.array_equal(words, want_words), (kinds, first, w)
                want, _ = ref.tally(want_words)
                assert counts.tolist() == [int(v) for v in want], (kinds, first, w)
                assert native.tally_host(words)['accepted'] == int(counts[0])
            seen += int(got.counts[:, 0].sum())
            assert int(got.counts[0, 0]) == SAMPLES and not got.counts[0, 1:].any()      # no fault: accepted, nothing wrong
    assert seen > 6 * SAMPLES


def test_words_past_ldr_are_left_untouched_and_ranges_join():
    native = gadget("cycle", "steane", 1)[0]
    eff = np.ascontiguousarray(native.effects, dtype="<u8")
    out = np.full((50, 5), 0xDEADBEEF, dtype="<u8")
    _native.check(_native.lib().gf2_stratum_outcomes_host(eff.ctypes.data, eff.shape[0], 3, 3, 9, 40, 50, 1.0, 1.0, 1.0, out.ctypes.data, 5))
    assert (out[:, 3:] == 0xDEADBEEF).all()
    whole = _native.stratum_outcomes_host(native.effects, 3, 90, seed=9)
    assert np.array_equal(out[:, :3], whole[40:]) and np.array_equal(_native.stratum_outcomes_host(native.effects, 3, 40, seed=9), whole[:40])
    assert _native.stratum_outcomes_host(native.effects, 3, 0).shape == (0, 3)
    two = native.strata([3, 5], [1000, 0], first_sample=[0, 7], host=True)
    assert two.counts[0].tolist() == native.strata([3], 1000, host=True).counts[0].tolist() and not two.counts[1].any()


# ---- the committed literals and the exact weight-2 strata --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def literal_run(kind):
    native, ref, eff = gadget("cycle", "steane", 1) if kind == "cycle" else gadget("program", "steane", "")
    return native.strata([2], LITERAL_SAMPLES, host=True), ref, eff


@pytest.mark.parametrize("kind, literal", [("cycle", CYCLE_LITERAL), ("program", PROGRAM_LITERAL)])
def test_literals(kind, literal):
    got, ref, eff = literal_run(kind)
    assert got.counts[0].tolist() == literal
    assert gsr.stratum_counts(ref, eff, 0, 0, LITERAL_SAMPLES, 2) == literal      # the restatement alone


@pytest.mark.parametrize("kind", ["cycle", "program"])
def test_sampled_weight_2_agrees_with_the_exact_stratum(kind):
    """|sampled fraction - exact fraction| <= 5 sigma, sigma = sqrt(f (1 - f) / N), for every field but the sum trial_wrong: under a
    correct sampler one comparison fails with probability 6e-7.  (The restatement's largest |z| with this seed is 1.0.)"""
    got, ref, eff = literal_run(kind)
    fields = EC if kind == "cycle" else FT
    exact = ger.pairs(ref, eff)                                               # [n_x][n_y][F] over all 9 C(L, 2) configurations
    total = 9 * math.comb(ref.locations, 2)
    checked = 0
    for col, name in enumerate(fields):
        if name == 'trial_wrong':
            continue
        f = int(exact[:, :, col].sum()) / total                               # kinds (1, 1, 1): every configuration weighs the same
        sigma = math.sqrt(f * (1.0 - f) / LITERAL_SAMPLES)
        z = abs(int(got.counts[0, col]) / LITERAL_SAMPLES - f)
        print("%s %s: exact %.6f sampled %.6f sigma %.2e" % (kind, name, f, int(got.counts[0, col]) / LITERAL_SAMPLES, sigma))
        assert z <= 5.0 * sigma, (kind, name, f, sigma)
        checked += 1
    assert checked == len(fields) - (kind == "program")
    assert abs(int(exact[:, :, 0].sum()) / total - (0.166 if kind == "cycle" else 0.151)) < 1e-3


# ---- the estimator ----------------------------------------------------------------------------------------------------------------

def toy_exact():
    """nb = 6 positions, weights 0 .. 3 with hand-made counts (accepted, wrong, trial_wrong)."""
    fields = ('accepted', 'wrong', 'trial_wrong')
    counts = [np.zeros((w + 1, w + 1, 3), dtype=np.uint64) for w in range(4)]
    counts[0][0, 0] = (1, 0, 0)
    counts[1][1, 0], counts[1][0, 1], counts[1][0, 0] = (6, 1, 1), (4, 0, 0), (5, 2, 3)
    counts[2][2, 0], counts[2][1, 1], counts[2][0, 2], counts[2][1, 0], counts[2][0, 1], counts[2][0, 0] = \
        (12, 3, 4), (20, 5, 9), (9, 1, 1), (22, 8, 8), (17, 2, 5), (10, 4, 6)
    counts[3][3, 0], counts[3][0, 0], counts[3][1, 1] = (15, 6, 7), (12, 5, 9), (40, 9, 11)
    return PostSelectedStrata(6, range(4), counts, fields)


def test_counts_at_the_exact_fractions_reproduce_the_exact_rate():
    exact = toy_exact()
    kinds, p = (1, 1, 1), 0.07
    # N_w a multiple of 3^w C(6, w): N_w times the exact fractions are whole numbers
    weights, samples, counts = [1, 2, 3], [], []
    for w in weights:
        n_w = 5 * 3**w * math.comb(6, w)
        samples.append(n_w)
        counts.append([5 * int(exact.counts[w][:, :, f].sum()) for f in range(3)])
    sampled = SampledPostSelectedStrata(6, weights, samples, counts, exact.fields, kinds)
    want = exact.rate(p, kinds, 'wrong')
    head = PostSelectedStrata(6, [0], exact.counts[:1], exact.fields)
    for merged in (head.merged(sampled), PostSelectedStrata(6, [0, 1], exact.counts[:2], exact.fields).merged(sampled),
                   exact.merged(sampled)):
        got = merged.rate(p, 'wrong')
        assert isinstance(got, montecarlo.PostSelectedRate) and isinstance(merged, MergedPostSelectedStrata)
        for a, b in zip((got.estimate, got.lower, got.upper), want):
            assert abs(a - b) <= 1e-12 * abs(b)
        assert abs(merged.joint(p, 'wrong') - exact.joint(p, kinds, 'wrong')) <= 1e-12 * exact.joint(p, kinds, 'wrong')
        for a, b in zip(merged.acceptance(p), exact.acceptance(p, kinds)):
            assert abs(a - b) <= 1e-12 * b
    assert exact.merged(sampled).rate(p, 'wrong').stderr == 0.0              # every weight has its exact stratum: no variance
    assert head.merged(sampled).rate(p, 'wrong').stderr > 0.0


def test_stderr_of_one_sampled_stratum_is_the_binomial_error_of_the_ratio():
    sampled = SampledPostSelectedStrata(50, [3], [10000], [[2500, 300, 700]], ('accepted', 'wrong', 'trial_wrong'))
    for p in (1e-3, 0.2):
        got = sampled.rate(p, 'wrong')
        r = 300 / 2500
        assert abs(got.estimate - r) < 1e-15
        assert abs(got.stderr - math.sqrt(r * (1 - r) / (10000 * 0.25))) <= 1e-12 * got.stderr
        b = montecarlo.binomial_weights(50, p)
        t = 1.0 - b[3]
        assert abs(got.lower - b[3] * 0.03 / (b[3] * 0.25 + t)) < 1e-12 and abs(got.upper - (b[3] * 0.03 + t) / (b[3] * 0.25 + t)) < 1e-12
        assert got.lower <= got.estimate <= got.upper


def test_two_strata_by_hand():
    """nb = 4, p = 1/2: B_w = C(4, w) / 16, so B_1 = 1/4 and B_2 = 3/8.  Stratum 1: 100 samples, 40 accepted, 10 wrong; stratum 2: 200
    samples, 50 accepted, 20 wrong.  N = 0.25 * 0.1 + 0.375 * 0.1 = 0.0625, D = 0.25 * 0.4 + 0.375 * 0.25 = 0.19375, R = 10 / 31,
    T = 1 - 5/8 = 0.375.  Brackets: n (1 - R)^2 + (a - n) R^2 - (n - R a)^2 with (n, a) = (0.1, 0.4) and (0.1, 0.25)."""
    sampled = SampledPostSelectedStrata(4, [1, 2], [100, 200], [[40, 10], [50, 20]], ('accepted', 'wrong'))
    got = sampled.rate(0.5, 'wrong')
    r = 10.0 / 31.0
    assert abs(got.estimate - r) < 1e-15
    assert abs(got.lower - 0.0625 / 0.56875) < 1e-15 and abs(got.upper - 0.4375 / 0.56875) < 1e-15
    v_1 = 0.1 * (21 / 31)**2 + 0.3 * (10 / 31)**2 - (0.1 - 4 / 31)**2
    v_2 = 0.1 * (21 / 31)**2 + 0.15 * (10 / 31)**2 - (0.1 - 2.5 / 31)**2
    assert abs(v_1 - 73.29 / 961) < 1e-15 and abs(v_2 - 58.74 / 961) < 1e-15    # (44.1 + 30 - 0.81 and 44.1 + 15 - 0.36, over 31^2)
    want = math.sqrt(0.0625 * v_1 / 100 + 0.140625 * v_2 / 200) / 0.19375
    assert abs(got.stderr - want) < 1e-15 and abs(want - 0.0491389) < 1e-6
    assert all(abs(a - b) < 1e-15 for a, b in zip(sampled.acceptance(0.5), (0.19375, 0.56875))) and abs(sampled.joint(0.5, 'wrong') - 0.0625) < 1e-15


def test_exact_weights_count_as_covered():
    exact = toy_exact()
    sampled = SampledPostSelectedStrata(6, [2, 4], [900, 500], [[300, 30, 40], [100, 20, 25]], exact.fields)
    part = PostSelectedStrata(6, [0, 1, 2], exact.counts[:3], exact.fields)
    merged = part.merged(sampled)
    assert merged.weights.tolist() == [0, 1, 2, 4]
    b = montecarlo.binomial_weights(6, 0.1)
    d, d_t = merged.acceptance(0.1)
    assert abs((d_t - d) - (b[3] + b[5] + b[6])) < 1e-15
    # weight 2 has an exact stratum: it is used, and the sampled one of that weight adds no variance
    a_2 = float(part.coefficients((1, 1, 1), 'accepted')[2]) / math.comb(6, 2)
    assert abs(d - (b[0] + b[1] * 15 / 18 + b[2] * a_2 + b[4] * 0.2)) < 1e-15
    alone = SampledPostSelectedStrata(6, [4], [500], [[100, 20, 25]], exact.fields)
    assert merged.rate(0.1, 'wrong') == part.merged(alone).rate(0.1, 'wrong')
    assert merged.rate(0.1, 'wrong').stderr > 0
    # a stratum without samples covers nothing
    empty = SampledPostSelectedStrata(6, [4, 5], [500, 0], [[100, 20, 25], [0, 0, 0]], exact.fields)
    assert part.merged(empty).weights.tolist() == [0, 1, 2, 4]
    assert part.merged([alone, SampledPostSelectedStrata(6, [5], [10], [[4, 1, 1]], exact.fields)]).weights.tolist() == [0, 1, 2, 4, 5]


def test_refusals_of_the_merge():
    exact = toy_exact()
    ok = SampledPostSelectedStrata(6, [4], [500], [[100, 20, 25]], exact.fields)
    with pytest.raises(ValueError, match="positions"):
        exact.merged(SampledPostSelectedStrata(7, [4], [500], [[100, 20, 25]], exact.fields))
    with pytest.raises(ValueError, match="kinds"):
        exact.merged([ok, SampledPostSelectedStrata(6, [5], [500], [[100, 20, 25]], exact.fields, kinds=(1, 0, 0))])
    with pytest.raises(ValueError, match="kinds"):
        exact.merged(ok, kinds=(2, 1, 1))
    assert exact.merged(SampledPostSelectedStrata(6, [4], [500], [[100, 20, 25]], exact.fields, kinds=(3, 3, 3))).kinds == (3.0, 3.0, 3.0)
    with pytest.raises(ValueError, match="one weight"):
        exact.merged([ok, SampledPostSelectedStrata(6, [5, 4], [10, 10], [[1, 0, 0], [1, 0, 0]], exact.fields)])
    with pytest.raises(ValueError, match="fields"):
        exact.merged(SampledPostSelectedStrata(6, [4], [500], [[100, 20]], ('accepted', 'wrong')))
    with pytest.raises(ValueError, match="sum"):
        exact.merged(ok).rate(0.01, 'trial_wrong')
    with pytest.raises(ValueError, match="sum"):
        ok.rate(0.01, 'trial_wrong')
    with pytest.raises(ValueError, match="no field"):
        ok.rate(0.01, 'logical_any')
    with pytest.raises(ValueError, match="distinct"):
        SampledPostSelectedStrata(6, [4, 4], [1, 1], [[1, 0, 0], [1, 0, 0]], exact.fields)
    with pytest.raises(ValueError, match="accepted"):
        SampledPostSelectedStrata(6, [4], [1], [[1, 0]], ('wrong', 'accepted'))
    with pytest.raises(ValueError, match="no accepted"):
        SampledPostSelectedStrata(6, [4], [10], [[0, 0, 0]], exact.fields).rate(0.1, 'wrong')
    native = gadget("cycle", "steane", 1)[0]
    for call in (lambda: native.strata([17], 10, host=True), lambda: native.strata([-1], 10, host=True), lambda: native.strata([2], -1, host=True),
                 lambda: native.strata([2], 10, kinds=(0, 0, 0), host=True), lambda: native.strata([2], 10, first_sample=-1, host=True),
                 lambda: native.strata([2, 2], 10, host=True)):
        with pytest.raises(ValueError):
            call()


def test_merged_rate_of_the_gate_free_program_lies_inside_the_exact_bounds():
    prog = gadget("program", "steane", "")[0]
    exact = prog.enumerate_strata([0, 1], host=True)
    sampled = prog.strata([2, 3, 4], 1 << 13, seed=3, host=True)
    est, lower, upper = exact.rate(1e-3, (1, 1, 1), 'wrong')
    got = exact.merged(sampled).rate(1e-3, 'wrong')
    assert lower <= got.lower <= got.estimate <= got.upper <= upper and got.stderr > 0
    assert got.upper - got.lower < 0.1 * (upper - lower)


# ---- refused arguments of the entry points ----------------------------------------------------------------------------------------

def test_refused_arguments_of_the_host_entry_point():
    native = gadget("cycle", "steane", 1)[0]
    eff = native.effects
    call = lambda eff=eff, w=2, count=4, kinds=(1, 1, 1), first=0, ldw=None: _native.stratum_outcomes_host(eff, w, count, kinds, 0, first, ldw)
    seventeen = np.zeros((17, 2, 3), dtype="<u8")
    for fn, text in ((lambda: call(w=17), r"min\(L = 330, 16\)"), (lambda: call(w=-1), "weight"), (lambda: call(eff[:5], w=6), r"min\(L = 5, 16\)"),
                     (lambda: call(seventeen, w=17), "16"), (lambda: call(count=-1), "negative range"), (lambda: call(first=-1), "negative range"),
                     (lambda: call(ldw=2), "ldw"), (lambda: call(np.zeros((4, 2, 17), dtype="<u8")), "ldr <= 16"),
                     (lambda: call(kinds=(0, 0, 0)), "kind weights"), (lambda: call(kinds=(1, -1, 1)), "kind weights"),
                     (lambda: call(kinds=(float("inf"), 1, 1)), "kind weights")):
        with pytest.raises(_native.GF2Error, match=text) as err:
            fn()
        assert err.value.code == _native.GF2_E_ARG and "gf2_stratum_outcomes_host" in err.value.message, text
    assert call(seventeen, w=16, count=3).shape == (3, 3)
    lib = _native.lib()
    out = np.zeros(3, dtype="<u8")
    assert lib.gf2_stratum_outcomes_host(None, 4, 3, 1, 0, 0, 1, 1.0, 1.0, 1.0, out.ctypes.data, 3) == _native.GF2_E_ARG
    assert lib.gf2_stratum_outcomes_host(seventeen.ctypes.data, 17, 3, 1, 0, 0, 1, 1.0, 1.0, 1.0, None, 3) == _native.GF2_E_ARG
    assert b"null buffer" in lib.gf2_last_error()
    assert lib.gf2_stratum_outcomes_host(seventeen.ctypes.data, 0, 3, 0, 0, 0, 1, 1.0, 1.0, 1.0, out.ctypes.data, 3) == _native.GF2_E_ARG
    assert b"locations" in lib.gf2_last_error()
    assert lib.gf2_stratum_outcomes_host(seventeen.ctypes.data, 17, 3, 1, 0, 0, 0, 1.0, 1.0, 1.0, None, 3) == _native.GF2_OK     # count 0


def test_device_entry_points_refuse_null_arguments_without_a_device():
    lib = _native.lib()
    counts = np.zeros(8, dtype=np.uint64)
    weights, samples = np.array([1], dtype=np.int32), np.array([1], dtype=np.int64)
    tail = (0, 0, 1, weights.ctypes.data, samples.ctypes.data, 1.0, 1.0, 1.0, counts.ctypes.data)
    assert lib.gf2_mc_ec_decode_strata(None, None, 1, 3, None, None, 0, 3, None, None, 0, *tail) == _native.GF2_E_ARG
    assert b"gf2_mc_ec_decode_strata: null argument" in lib.gf2_last_error()
    assert lib.gf2_mc_ft_decode_strata(None, None, 7, 0b0010101, 3, None, None, 0, 3, None, None, 0, *tail) == _native.GF2_E_ARG
    assert b"gf2_mc_ft_decode_strata: null argument" in lib.gf2_last_error()
    assert isinstance(ctypes.c_int, type) and not counts.any()
