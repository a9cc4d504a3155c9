"""
Exact strata of the two post-selected gadgets on the CPU (DESIGN.md sections 5b "Exact strata of the cycle" and 5c "Exact strata of the
measurement"): gf2_ec_enumerate_host / gf2_ft_enumerate_host (csrc/gf2_host.cpp), ECCircuit / FTProgram.enumerate_strata(host=True)
and montecarlo.PostSelectedStrata.  Every comparison is exact: integers or Fractions.

  host statement  against tests/gadget_enumerate_ref.py (itertools, identity fault vectors through the restated gadgets, ec_ref / ft_ref's
                  tally) on whole strata and windows; ranges add; the weight-1 strata are the single-fault censuses
  literals        the full weight-2 stratum of the gate-free Steane program against PAIR_COUNTS
  series          PostSelectedStrata's coefficients, bounds and refusals
  refusals        the argument errors of the two entry points
"""
import functools
import itertools
import math
from fractions import Fraction

import numpy as np
import pytest

from quantum_css_codes_amd import _native, ec_noise, ft_noise, montecarlo
from quantum_css_codes_amd.montecarlo import PostSelectedStrata
from tests import ec_ref, ft_ref
from tests import gadget_enumerate_ref as ger
from tests.test_ft import oracle_code

EC, FT = ec_noise.EC_FIELDS, ft_noise.FT_FIELDS

# The whole weight-2 strata of the gate-free programs, [n_x][n_y] ('accepted', 'wrong'), and the sums of the two sum fields that
# occur.  Derived with tests/gadget_enumerate_ref.py alone -- pairs(ft_ref.Rewritten(code, ""), effect_words(...)): identity fault
# vectors through Rewritten.outcome_words, all 9 C(L, 2) words judged by ft_ref.tally -- in 10 s (Steane, L = 1585, 11 297 880
# configurations) and 90 s (RM15, L = 3867, 67 274 199); no native code took part.
PAIR_COUNTS = {
    "steane": {'accepted': [[301283, 252329, 53910], [578785, 240855, 0], [282098, 0, 0]],
               'wrong': [[0, 102, 3044], [4620, 13500, 0], [15829, 0, 0]],
               'trial_wrong': [[0, 459, 10089], [20790, 45780, 0], [55580, 0, 0]],
               'unmatched_x': [[0, 0, 0], [0, 0, 0], [0, 0, 0]]},
    "rm15": {'accepted': [[1386873, 1196949, 259879], [2865349, 1232807, 0], [1505330, 0, 0]],
             'wrong': [[0, 0, 24], [0, 1812, 0], [3699, 0, 0]],
             'trial_wrong': [[0, 0, 108], [0, 6968, 0], [13994, 0, 0]],
             'unmatched_x': [[0, 2331, 1053], [118800, 55760, 0], [132682, 0, 0]]},
}
# The weight-1 strata, [n_x][n_y] (accepted, wrong): Z, Y / X of FTProgram.single_faults' census
SINGLE_COUNTS = {"steane": [[[770, 0], [317, 0]], [[748, 6], [0, 0]]], "rm15": [[[1650, 0], [707, 0]], [[1732, 0], [0, 0]]]}


@functools.lru_cache(maxsize=None)
def cycle(rounds):
    """(ECCircuit, ec_ref.Cycle, the restatement's effect words) of the Steane code: nothing here needs a GPU."""
    code = oracle_code("steane")
    ref = ec_ref.Cycle(code, rounds)
    return ec_noise.ECCircuit(code, rounds), ref, ger.effect_words(ref)


@functools.lru_cache(maxsize=None)
def program(name, ops):
    code = oracle_code(name)
    ref = ft_ref.Rewritten(code, ops)
    return ft_noise.FTProgram(code, ops), ref, ger.effect_words(ref)


def host(gadget, w, first=None, count=None):
    return gadget.enumerate_strata([w], first_rank=first, count=count, max_configurations=1 << 40, host=True).counts[0]


def same(got, want):
    return got.shape == want.shape and got.astype(object).tolist() == want.tolist()


# ---- the host statement against the restatement --------------------------------------------------------------------------------

@pytest.mark.parametrize("rounds", [1, 2])
def test_cycle_whole_strata(rounds):
    circ, ref, eff = cycle(rounds)
    assert circ.num_locations == ref.locations and circ.ldr == ref.ldr
    for w in (0, 1, 2):
        got = host(circ, w)
        assert same(got, ger.enumerate_range(ref, eff, w, 0, math.comb(ref.locations, w))), w
        assert got.shape == (w + 1, w + 1, len(EC))
    assert int(got[:, :, 0].sum()) < 9 * math.comb(ref.locations, 2) and int(got[:, :, 3].sum()) > 0


def test_gate_free_steane_program():
    prog, ref, eff = program("steane", "")
    L = ref.locations
    assert (L, prog.ldr) == (1585, 8)
    for w in (0, 1):
        assert same(host(prog, w), ger.enumerate_range(ref, eff, w, 0, math.comb(L, w))), w
    total = math.comb(L, 2)
    for first, count in ((0, 1), (12345, 4097), (total - 1000, 1000)):
        assert same(host(prog, 2, first, count), ger.enumerate_range(ref, eff, 2, first, count)), (first, count)
    first = math.comb(L, 3) // 2 + 54321                                     # 257 ranks deep inside weight 3
    got = host(prog, 3, first, 257)
    assert same(got, ger.enumerate_range(ref, eff, 3, first, 257)) and got.shape == (4, 4, len(FT))


def test_gate_free_rm15_program_has_unmatched_keys():
    prog, ref, eff = program("rm15", "")
    L = ref.locations
    assert (L, prog.ldr) == (3867, 9)
    got = host(prog, 1)
    assert same(got, ger.enumerate_range(ref, eff, 1, 0, L)) and got[:, :, :2].tolist() == SINGLE_COUNTS["rm15"]
    got = host(prog, 2, 2000000, 30001)
    assert same(got, ger.enumerate_range(ref, eff, 2, 2000000, 30001))
    assert int(got[:, :, FT.index('unmatched_x')].sum()) > 0 and int(got[:, :, 0].sum()) > 0


def test_ranges_add():
    circ = cycle(1)[0]
    total = math.comb(circ.num_locations, 2)
    cuts = [0, 1, 20011, total]
    parts = [host(circ, 2, lo, hi - lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(parts[0] + parts[1] + parts[2], host(circ, 2))
    prog = program("steane", "")[0]
    cuts = [0, 777, 1000, 1585]
    parts = [host(prog, 1, lo, hi - lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(parts[0] + parts[1] + parts[2], host(prog, 1))


def census_counts(classes, bits):
    """(L, 3) class bytes (columns X, Y, Z) -> per kind, the number of accepted faults with every bit of `bits` set."""
    hit = (classes & 1 != 0) & (classes & bits == bits)
    return hit.sum(axis=0).tolist()


def by_kind(counts, field):
    return [int(counts[1, 0, field]), int(counts[0, 1, field]), int(counts[0, 0, field])]    # X, Y, Z


def test_weight_1_strata_are_the_censuses():
    circ = cycle(1)[0]
    got = host(circ, 1)
    classes, flipping = circ.single_faults()
    assert classes.shape == (330, 3) and int(got[:, :, 0].sum()) == 390 and int(got[:, :, 1].sum()) == 3
    for field, bits in ((0, 0), (1, ec_noise.CLASS_FLIP_X), (2, ec_noise.CLASS_FLIP_Z), (4, ec_noise.CLASS_UNCORRECTABLE_X), (5, ec_noise.CLASS_UNCORRECTABLE_Z)):
        assert by_kind(got, field) == census_counts(classes, bits), EC[field]
    assert int(got[:, :, 3].sum()) == len(flipping)
    for name, ops, accepted, wrong in (("steane", "XXX", 3032, 15), ("rm15", "", 4089, 0), ("steane", "", 1835, 6)):
        prog = program(name, ops)[0]
        got = host(prog, 1)
        classes, bad = prog.single_faults()
        assert 3 * len(classes) == {"XXX": 7752}.get(ops, 3 * len(classes))
        assert (int(got[:, :, 0].sum()), int(got[:, :, 1].sum()), len(bad)) == (accepted, wrong, wrong)
        for field, bits in ((0, 0), (1, ft_noise.CLASS_WRONG), (3, ft_noise.CLASS_FIRST_TRIAL_WRONG), (4, ft_noise.CLASS_SPLIT_VOTE)):
            assert by_kind(got, field) == census_counts(classes, bits), (name, ops, FT[field])
        assert [int(v > 0) for v in by_kind(got, 5)] == [int(v > 0) for v in census_counts(classes, ft_noise.CLASS_UNMATCHED_X)]
    assert host(program("steane", "")[0], 1)[:, :, :2].tolist() == SINGLE_COUNTS["steane"]


# ---- the committed weight-2 table ---------------------------------------------------------------------------------------------

def test_full_weight_2_of_the_gate_free_steane_program():
    got = host(program("steane", "")[0], 2)                                  # 11 297 880 configurations
    for name, want in PAIR_COUNTS["steane"].items():
        assert got[:, :, FT.index(name)].tolist() == want, name
    assert int(got[:, :, 0].sum()) == 1709260 and int(got[:, :, 1].sum()) == 37095
    assert sum(sum(row) for row in PAIR_COUNTS["rm15"]['accepted']) == 8447187 and sum(sum(row) for row in PAIR_COUNTS["rm15"]['wrong']) == 5535


# ---- PostSelectedStrata ---------------------------------------------------------------------------------------------------------

def literal_strata(name):
    """The strata 0, 1, 2 of a gate-free program from the committed literals (accepted and wrong only)."""
    nb = {"steane": 1585, "rm15": 3867}[name]
    pair = np.stack((np.array(PAIR_COUNTS[name]['accepted']), np.array(PAIR_COUNTS[name]['wrong'])), axis=2)
    return PostSelectedStrata(nb, [0, 1, 2], [np.array([[[1, 0]]]), np.array(SINGLE_COUNTS[name]), pair], ('accepted', 'wrong'))


def test_series_of_the_programs():
    prog = program("steane", "")[0]
    strata = prog.enumerate_strata([0, 1, 2], host=True)
    assert isinstance(strata, PostSelectedStrata) and strata.fields == FT and strata.nb == 1585
    assert strata.series((1, 1, 1), 'wrong') == [0, 2, Fraction(8701, 3)]
    assert strata.series((1, 0, 0), 'wrong')[1] == 6 and strata.series((1, 1, 1), 'wrong', order=1) == [0, 2]
    assert strata.leading_order((1, 1, 1), 'wrong') == (1, 2) and strata.leading_order((0, 0, 1), 'wrong') is None
    assert literal_strata("steane").series() == [0, 2, Fraction(8701, 3)]
    xxx = program("steane", "XXX")[0].enumerate_strata([0, 1], host=True)
    assert xxx.series((1, 1, 1), 'wrong') == [0, 5] and xxx.series((1, 0, 0), 'wrong') == [0, 15]
    assert literal_strata("rm15").leading_order((1, 1, 1), 'wrong') == (2, 615)
    assert strata.series((1, 1, 1), 'trial_wrong')[1] > 0                    # a sum field: the series of the conditional expectation
    assert strata.configurations() == [1, 3 * 1585, 9 * math.comb(1585, 2)]


def toy():
    """nb = 4 positions, every weight: a configuration (kinds per position, 0 = none) is accepted unless position 0 carries a Z, wrong
    when the number of X and Y among positions 1 .. 3 is odd, and 'trial_wrong' counts them.  Returns (strata, all 4^4 configurations)."""
    fields = ('accepted', 'wrong', 'trial_wrong')
    counts = [np.zeros((w + 1, w + 1, 3), dtype=np.uint64) for w in range(5)]
    configs = []
    for kinds in itertools.product((0, 1, 2, 3), repeat=4):                  # 0 none, 1 X, 2 Y, 3 Z
        w, n_x, n_y = sum(k != 0 for k in kinds), kinds.count(1), kinds.count(2)
        accepted = kinds[0] != 3
        flips = sum(k in (1, 2) for k in kinds[1:])
        configs.append((kinds, accepted, flips))
        if accepted:
            counts[w][n_x, n_y] += np.array([1, flips & 1, flips], dtype=np.uint64)
    return PostSelectedStrata(4, range(5), counts, fields), configs


def test_rate_bounds_against_brute_force():
    strata, configs = toy()
    p, kinds = Fraction(1, 10), (Fraction(1, 2), Fraction(1, 3), Fraction(1, 6))
    prob = lambda ks: math.prod((1 - p) if k == 0 else p * kinds[k - 1] for k in ks)
    d = sum(prob(ks) for ks, acc, _ in configs if acc)
    n = sum(prob(ks) for ks, acc, flips in configs if acc and flips & 1)
    estimate, lower, upper = strata.rate(float(p), kinds, 'wrong')
    assert lower == estimate == upper and abs(estimate - float(n / d)) < 1e-15
    assert abs(strata.joint(float(p), kinds, 'accepted') - float(d)) < 1e-15 and strata.acceptance(float(p), kinds)[0] == strata.acceptance(float(p), kinds)[1]
    # the series, exactly: N(p) and D(p) as polynomials in p from the brute-force sum; series * D = N up to the order of the series
    def poly(select):
        out = [Fraction(0)] * 5
        for ks, acc, flips in configs:
            if acc and select(flips):
                w = sum(k != 0 for k in ks)
                weight = math.prod(kinds[k - 1] for k in ks if k)
                for j in range(4 - w + 1):                                   # p^w (1 - p)^(4 - w)
                    out[w + j] += weight * math.comb(4 - w, j) * (-1)**j
        return out
    num, den = poly(lambda flips: flips & 1), poly(lambda flips: True)
    series = strata.series(kinds, 'wrong')
    assert len(series) == 5 and all(sum(series[i] * den[k - i] for i in range(k + 1)) == num[k] for k in range(5))
    assert all(isinstance(c, Fraction) for c in series) and series[0] == 0 and series[1] == 3 * (kinds[0] + kinds[1])
    # some weights missing: the bounds open and hold the full value
    part = PostSelectedStrata(4, [0, 1, 2], strata.counts[:3], strata.fields)
    estimate, lower, upper = part.rate(float(p), kinds, 'wrong')
    assert lower < estimate < upper and lower <= float(n / d) <= upper
    low, high = part.acceptance(float(p), kinds)
    assert low <= float(d) <= high and low < high
    assert part.series(kinds, 'wrong') == series[:3]


def test_refusals_of_the_strata_object():
    strata, _ = toy()
    with pytest.raises(ValueError, match="sum"):
        strata.rate(0.01, (1, 1, 1), 'trial_wrong')
    assert strata.series((1, 1, 1), 'trial_wrong')[1] == 2                   # 3 positions x (X or Y of three kinds)
    with pytest.raises(ValueError, match="weight 0"):
        PostSelectedStrata(4, [1, 2], strata.counts[1:3], strata.fields).series()
    with pytest.raises(ValueError, match="no field"):
        strata.rate(0.01, (1, 1, 1), 'logical_any')
    with pytest.raises(ValueError, match="accepted"):
        PostSelectedStrata(4, [0], strata.counts[:1], ('wrong', 'accepted'))
    with pytest.raises(ValueError, match="kinds"):
        strata.series((0, 0, 0))
    rejected = [c.copy() for c in strata.counts]
    rejected[0][0, 0, 0] = 0
    with pytest.raises(ValueError, match="A_0"):
        PostSelectedStrata(4, range(5), rejected, strata.fields).series()
    prog = program("steane", "")[0]
    with pytest.raises(ValueError, match="more than max_configurations"):
        prog.enumerate_strata([3], host=True)
    with pytest.raises(ValueError, match="weight"):
        prog.enumerate_strata([9], host=True)
    with pytest.raises(ValueError, match="leave"):
        prog.enumerate_strata([1], first_rank=1000, count=586, host=True)


# ---- refused arguments of the entry points ----------------------------------------------------------------------------------------

def test_refused_arguments_of_the_host_entry_points():
    circ, prog = cycle(1)[0], program("steane", "")[0]
    tables = circ._tables()
    r1, keys1, flips1, r2, keys2, flips2 = tables
    ec = lambda eff=circ.effects, rounds=1, tables=tables, w=1, first=0, count=1: _native.ec_enumerate_host(eff, rounds, *tables, w, first, count)
    ft = lambda eff=prog.effects, nsteps=prog.nsteps, mask=prog.measure_mask, tables=tables, w=1, first=0, count=1: \
        _native.ft_enumerate_host(eff, nsteps, mask, *tables, w, first, count)
    wide_ec, wide_ft = np.zeros((4, 2, 9), dtype="<u8"), np.zeros((4, 2, 17), dtype="<u8")
    for call, text in ((lambda: ec(w=9), "weight"), (lambda: ec(w=-1), "weight"), (lambda: ec(np.zeros((2, 2, 3), dtype="<u8"), w=3), "weight"),
                       (lambda: ec(w=2, count=math.comb(330, 2) + 1), "leave"), (lambda: ec(first=330, count=1), "leave"),
                       (lambda: ec(first=-1), "leave"), (lambda: ec(count=-1), "leave"),
                       (lambda: ec(wide_ec, rounds=2), "ldr <= 8"), (lambda: ec(rounds=2), "F >= 1"), (lambda: ec(rounds=0), "rounds"),
                       (lambda: ec(np.zeros((4, 2, 8), dtype="<u8"), rounds=7), "rounds <= 6"),
                       (lambda: ec(tables=(32, keys1, flips1, r2, keys2, flips2)), "<= 31"), (lambda: ec(tables=(r1, keys1, flips1, 0, keys2, flips2)), "<= 31"),
                       (lambda: ec(tables=(r1, np.append(keys1, keys1[:1]), np.append(flips1, 0), r2, keys2, flips2)), "twice"),
                       (lambda: ec(circ.effects | np.uint64(1 << 20)), "beyond"),
                       (lambda: ft(w=9), "weight"), (lambda: ft(w=2, first=math.comb(1585, 2), count=1), "leave"),
                       (lambda: ft(wide_ft, nsteps=6), "ldr <= 16"), (lambda: ft(nsteps=8), "F >= 1"), (lambda: ft(nsteps=0, mask=0), "nsteps >= 1"),
                       (lambda: ft(mask=0b010100), "odd number"), (lambda: ft(mask=1 << 6), "at or above nsteps"),
                       (lambda: ft(tables=(r1, keys1, flips1, 32, keys2, flips2)), "<= 31"),
                       (lambda: ft(prog.effects | np.uint64(1 << 40)), "beyond")):
        with pytest.raises(_native.GF2Error, match=text) as err:
            call()
        assert err.value.code == _native.GF2_E_ARG, text
    assert not ec(w=2, first=100, count=0).any() and ec(w=2, first=100, count=0).shape == (3, 3, 8)
    assert not ft(w=2, first=100, count=0).any() and ft(w=2, first=100, count=0).shape == (3, 3, 7)
