"""
Sampled strata under gate-level faults on the CPU (DESIGN.md section 5e "Sampled strata under gate-level faults"):
gf2_gate_stratum_outcomes_host followed by gf2_ec_tally_host / gf2_ft_tally_host (csrc/gf2_host.cpp), ECCircuit /
FTProgram.gate_strata(host=True) and montecarlo.SampledGateStrata / MergedGateStrata.

  host statement  against tests/gate_strata_ref.py, bit for bit: sites and kinds (through a one-hot effect table), words, c
  distribution    10^6 host samples: subsets and kinds uniform, two strata of one seed independent, the Floyd mutant rejected
  exactness       the one-round Steane cycle against gf2_ec_gate_enumerate_host's exact fractions, cell by cell
  estimator       the merge, the ratio, its bounds, T and the delta-method error (also against the spread of 200 runs)
  refusals        the argument errors, each naming its limit

Seeds are 20261019 + the case's index.  A statistical case fails below p = 10^-6 in either tail (oracle.exact_dist).
"""
import functools
import itertools
import math

import numpy as np
import pytest

from oracle import exact_dist as ed
from quantum_css_codes_amd import _native, ec_noise, ft_noise, montecarlo
from quantum_css_codes_amd.montecarlo import GateStrata, MergedGateStrata, SampledGateStrata
from tests import ec_ref, ft_ref
from tests import gadget_enumerate_ref as ger
from tests import gate_strata_ref as gsr
from tests.test_ft import oracle_code

SEED = 20261019
EC, FT = ec_noise.EC_FIELDS, ft_noise.FT_FIELDS
SITE_TABLES = ((1, 1), (3, 2), (16, 0), (0, 16), (40, 25), (700, 600))
FIRSTS = (0, (1 << 32) + 12345)


def strata_of(n1, n2):
    """The strata of the bit-for-bit cases that fit (n1, n2)."""
    want = [(0, 0), (1, 0), (0, 1), (n1, n2), (16, 0), (0, 16), (8, 8), (3, 5)]
    out = []
    for a, b in want:
        if a <= n1 and b <= n2 and a + b <= 16 and (a, b) not in out:
            out.append((a, b))
    return out


def one_hot_table(locations):
    """eff (L, 2, ldr) with bit 2 l + component set in effect (l, component): the XOR over distinct picks is the set of their effects."""
    ldr = (2 * locations + 63) // 64
    eff = np.zeros((locations, 2, ldr), dtype="<u8")
    for l in range(locations):
        for comp in range(2):
            bit = 2 * l + comp
            eff[l, comp, bit >> 6] = np.uint64(1) << np.uint64(bit & 63)
    return eff


def one_hot_words(site_loc, site, kappa, ldr):
    """What the one-hot table gives for the reference's sites and kind masks, computed without the table."""
    words = np.zeros((len(site), ldr), dtype=np.uint64)
    rows = np.arange(len(site))
    for k in range(site.shape[1]):
        loc = np.asarray(site_loc, dtype=np.int64)[site[:, k]]
        for bit in range(4):
            has = ((kappa[:, k] >> bit) & 1).astype(bool)
            at = 2 * loc[has] + bit
            np.bitwise_xor.at(words, (rows[has], at >> 6), np.uint64(1) << (at & 63).astype(np.uint64))
    return words


# ---- the host statement against the restatement ----------------------------------------------------------------------------------

@pytest.mark.parametrize("case, table", list(enumerate(SITE_TABLES)), ids=lambda v: str(v))
def test_host_statement_is_the_restatement_bit_for_bit(case, table):
    n1, n2 = table
    seed = SEED + case
    rng = np.random.default_rng(seed)
    locations = n1 + 2 * n2
    site_loc = gsr.synthetic_sites(n1, n2, rng)
    random_eff = rng.integers(0, 1 << 63, (locations, 2, 5), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (locations, 2, 5), dtype=np.uint64)
    hot = one_hot_table(locations) if 2 * locations <= 1024 else None
    count = 1500
    for a, b in strata_of(n1, n2):
        for first in FIRSTS:
            site, kappa = gsr.gate_stratum_draws(seed, first, count, n1, n2, a, b)
            assert site.shape == (count, a + b)
            if a + b:
                assert (np.sort(site, axis=1)[:, 1:] != np.sort(site, axis=1)[:, :-1]).all()              # distinct sites
                assert (site[:, :a] < n1).all() and (site[:, a:] >= n1).all() and site.max() < n1 + n2
                assert kappa.min() >= 1 and (kappa[:, :a] <= 3).all() and kappa.max() <= 15
            want_words, want_c = gsr.gate_stratum_words(random_eff, site_loc, n1, n2, seed, first, count, a, b)
            words, c = _native.gate_stratum_outcomes_host(random_eff, site_loc, n1, n2, a, b, count, seed, first)
            assert np.array_equal(words, want_words) and np.array_equal(c, want_c), (table, a, b, first)
            if hot is not None:                                                                           # sites and kinds, one by one
                words, c = _native.gate_stratum_outcomes_host(hot, site_loc, n1, n2, a, b, count, seed, first)
                assert np.array_equal(words, one_hot_words(site_loc, site, kappa, hot.shape[2])), (table, a, b, first)
                assert np.array_equal(c, want_c)


def test_words_past_ldr_are_left_untouched_and_ranges_join():
    rng = np.random.default_rng(SEED)
    n1, n2 = 9, 8
    site_loc = gsr.synthetic_sites(n1, n2, rng)
    eff = rng.integers(0, 1 << 62, (n1 + 2 * n2, 2, 3), dtype=np.uint64)
    out = np.full((50, 5), 0xDEADBEEF, dtype="<u8")
    two = np.zeros(50, dtype=np.uint8)
    _native.check(_native.lib().gf2_gate_stratum_outcomes_host(eff.ctypes.data, len(eff), 3, site_loc.ctypes.data, n1, n2, 2, 3, 9, 40, 50,
                                                               out.ctypes.data, 5, two.ctypes.data))
    assert (out[:, 3:] == 0xDEADBEEF).all()
    whole, whole_c = _native.gate_stratum_outcomes_host(eff, site_loc, n1, n2, 2, 3, 90, seed=9)
    assert np.array_equal(out[:, :3], whole[40:]) and np.array_equal(two, whole_c[40:])
    head, head_c = _native.gate_stratum_outcomes_host(eff, site_loc, n1, n2, 2, 3, 40, seed=9)
    assert np.array_equal(head, whole[:40]) and np.array_equal(head_c, whole_c[:40])
    assert _native.gate_stratum_outcomes_host(eff, site_loc, n1, n2, 2, 3, 0)[0].shape == (0, 3)


@pytest.mark.parametrize("which", [("cycle", "steane", 2), ("program", "steane", "")], ids=lambda g: "%s-%s-%s" % g)
def test_gadget_counts_are_the_restatement(which):
    """ECCircuit / FTProgram.gate_strata(host=True) against the restated gadget's own tally of the restated draw."""
    code = oracle_code(which[1])
    if which[0] == "cycle":
        native, ref = ec_noise.ECCircuit(code, which[2]), ec_ref.Cycle(code, which[2])
    else:
        native, ref = ft_noise.FTProgram(code, which[2]), ft_ref.Rewritten(code, which[2])
    eff = ger.effect_words(ref)
    site_loc, n1, n2, _ = native.gate_sites()
    strata = [(0, 0), (1, 0), (0, 1), (2, 1), (3, 5), (0, 16)]
    got = native.gate_strata(strata, 3000, seed=SEED, first_sample=77, host=True)
    assert isinstance(got, SampledGateStrata) and (got.n1, got.n2) == (n1, n2) and got.fields == (EC if which[0] == "cycle" else FT)
    assert got.strata.tolist() == [list(s) for s in strata] and got.samples.tolist() == [3000] * len(strata)
    for (a, b), counts in zip(strata, got.counts):
        want = gsr.gate_stratum_counts(ref, eff, site_loc, n1, n2, SEED, 77, 3000, a, b)
        assert np.array_equal(counts, want), (a, b)
        assert not counts[b + 1:].any()
    assert int(got.counts[0, 0, 0]) == 3000 and not got.counts[0, 0, 1:].any()                            # no fault: accepted, nothing wrong
    two = native.gate_strata([(2, 1), (3, 3)], [1000, 0], seed=SEED, first_sample=[77, 5], host=True)
    assert np.array_equal(two.counts[0], native.gate_strata([(2, 1)], 1000, seed=SEED, first_sample=77, host=True).counts[0])
    assert not two.counts[1].any()


# ---- the distribution of the draw ---------------------------------------------------------------------------------------------------

DIST_N1, DIST_N2, DIST_SAMPLES = 7, 5, 10**6
DIST_SITES = np.concatenate((np.arange(DIST_N1), DIST_N1 + 2 * np.arange(DIST_N2))).astype(np.int32)   # L = 17: one word, one-hot


def decode_one_hot(words):
    """(count, n1 + n2) kind masks per site (0: not picked) from the one-hot table's single word over DIST_SITES."""
    word = words[:, 0]
    masks = [(word >> np.uint64(2 * l)) & np.uint64(3) for l in DIST_SITES[:DIST_N1]]
    masks += [(word >> np.uint64(2 * l)) & np.uint64(15) for l in DIST_SITES[DIST_N1:]]
    return np.stack(masks, axis=1).astype(np.int64)


@functools.lru_cache(maxsize=None)
def dist_run(a, b, seed):
    words, c = _native.gate_stratum_outcomes_host(one_hot_table(DIST_N1 + 2 * DIST_N2), DIST_SITES, DIST_N1, DIST_N2, a, b, DIST_SAMPLES, seed)
    masks = decode_one_hot(words)
    assert ((masks[:, :DIST_N1] != 0).sum(axis=1) == a).all() and ((masks[:, DIST_N1:] != 0).sum(axis=1) == b).all()
    cnot = masks[:, DIST_N1:]
    assert np.array_equal(c, (((cnot & 3) != 0) & ((cnot >> 2) != 0)).sum(axis=1))
    return masks


def subset_index(picked):
    """The rank of every row's subset (a boolean (count, n) array with k picks per row) among the C(n, k) subsets, and C(n, k)."""
    n, k = picked.shape[1], int(picked[0].sum())
    table = {subset: rank for rank, subset in enumerate(itertools.combinations(range(n), k))}
    keys = (picked * (1 << np.arange(n))).sum(axis=1)
    rank_of_key = np.full(1 << n, -1, dtype=np.int64)
    for subset, rank in table.items():
        rank_of_key[sum(1 << s for s in subset)] = rank
    return rank_of_key[keys], len(table)


def check_uniform(label, masks, a, b):
    """Subsets uniform per class and jointly; kinds uniform over 3 and over 15 at every site, and independent of the subset's rank."""
    one, two = masks[:, :DIST_N1], masks[:, DIST_N1:]
    ranks, cells = [], []
    for name, part, k in (("one-operand", one, a), ("CNOT", two, b)):
        if k:
            rank, ncells = subset_index(part != 0)
            ed.assert_chi2("%s %s subsets" % (label, name), np.bincount(rank, minlength=ncells), np.full(ncells, 1.0 / ncells), len(masks))
            ranks.append(rank)
            cells.append(ncells)
    if len(ranks) == 2:
        joint = np.bincount(ranks[0] * cells[1] + ranks[1], minlength=cells[0] * cells[1])
        ed.assert_chi2(label + " joint subsets", joint, np.full(len(joint), 1.0 / len(joint)), len(masks))
    for name, part, nkinds in (("one-operand", one, 3), ("CNOT", two, 15)):
        kinds = part[part != 0]
        if len(kinds):
            ed.assert_chi2("%s %s kinds" % (label, name), np.bincount(kinds - 1, minlength=nkinds), np.full(nkinds, 1.0 / nkinds), len(kinds))
            site = np.nonzero(part)[1]
            table = np.bincount(site * nkinds + kinds - 1, minlength=part.shape[1] * nkinds)
            ed.assert_chi2("%s %s (site, kind)" % (label, name), table, np.full(len(table), 1.0 / len(table)), len(kinds))


@pytest.mark.parametrize("case, stratum", list(enumerate([(2, 0), (0, 2), (2, 2), (7, 5)])), ids=lambda v: str(v))
def test_subsets_and_kinds_are_uniform(case, stratum):
    a, b = stratum
    check_uniform("stratum (%d, %d)" % stratum, dist_run(a, b, SEED + case), a, b)


def test_two_strata_of_one_seed_are_independent():
    """Sample i of (2, 2) and sample i of (2, 3) under one seed: their one-operand subsets (21 x 21 cells), their CNOT subsets
    (10 x 10) and the kinds of their lowest picked sites (3 x 3, 15 x 15) against the product of the uniform marginals."""
    first, second = dist_run(2, 2, SEED + 2), dist_run(2, 3, SEED + 2)
    for name, cols in (("one-operand", slice(0, DIST_N1)), ("CNOT", slice(DIST_N1, None))):
        (r_1, c_1), (r_2, c_2) = subset_index(first[:, cols] != 0), subset_index(second[:, cols] != 0)
        table = np.bincount(r_1 * c_2 + r_2, minlength=c_1 * c_2)
        ed.assert_chi2("(2,2) x (2,3) %s subsets" % name, table, np.full(c_1 * c_2, 1.0 / (c_1 * c_2)), DIST_SAMPLES)
        nkinds = 3 if name == "one-operand" else 15
        lowest = lambda masks: masks[:, cols][np.arange(len(masks)), (masks[:, cols] != 0).argmax(axis=1)] - 1
        table = ed.pair_table(lowest(first), lowest(second), nkinds)
        ed.assert_chi2("(2,2) x (2,3) %s kinds" % name, table, np.full(nkinds * nkinds, 1.0 / nkinds**2), DIST_SAMPLES)


def test_the_floyd_mutant_is_rejected():
    """Floyd's t drawn over j instead of j + 1 never picks the last site first: the same chi-square refuses it."""
    for a, b in ((2, 0), (0, 2)):
        n = DIST_N1 if a else DIST_N2
        for plus, ok in ((1, True), (0, False)):
            site, _ = gsr.gate_stratum_draws(SEED, 0, DIST_SAMPLES, DIST_N1, DIST_N2, a, b, floyd_plus=plus)
            picked = np.zeros((DIST_SAMPLES, n), dtype=bool)
            np.put_along_axis(picked, site - (0 if a else DIST_N1), True, axis=1)
            rank, ncells = subset_index(picked)
            chi2, dof = ed.pooled_chi2(np.bincount(rank, minlength=ncells), np.full(ncells, 1.0 / ncells), DIST_SAMPLES)
            assert ed.chi2_verdict(chi2, dof)[2] == ok, (a, b, plus, chi2)


# ---- exactness: the one-round Steane cycle against the exact strata ------------------------------------------------------------------

EXACT_STRATA = ((1, 0), (0, 1), (2, 0), (1, 1), (0, 2))
EXACT_SAMPLES = 1 << 20


@functools.lru_cache(maxsize=None)
def steane_cycle():
    return ec_noise.ECCircuit(oracle_code("steane"), 1)


@functools.lru_cache(maxsize=None)
def steane_sampled():
    return steane_cycle().gate_strata(EXACT_STRATA, EXACT_SAMPLES, seed=SEED, host=True)


@functools.lru_cache(maxsize=None)
def steane_exact(top=2):
    return steane_cycle().enumerate_gate_strata(list(range(top + 1)), host=True)


def check_cells_against_exact(label, sampled, exact, n1, n2, fields):
    """Every [c][field] cell of every indicator field of every sampled stratum against the exact fraction: a binomial z-test (an
    impossible cell must be empty), the rows c > b empty."""
    checked = 0
    for (a, b), n, counts in zip(sampled.strata.tolist(), sampled.samples.tolist(), sampled.counts):
        configs = math.comb(n1, a) * math.comb(n2, b) * 3**a * 15**b
        rows = exact.counts[exact.weights.index(a + b)][b]
        assert not counts[b + 1:].any()
        for c in range(b + 1):
            for col, name in enumerate(fields):
                if name in GateStrata.SUM_FIELDS:
                    continue
                f = int(rows[c, col]) / configs
                ed.assert_z("%s (%d, %d) c = %d %s" % (label, a, b, c, name), int(counts[c, col]), n * f, n * f * (1.0 - f))
                checked += 1
    return checked


def test_sampled_cells_agree_with_the_exact_strata():
    cycle = steane_cycle()
    _, n1, n2, _ = cycle.gate_sites()
    checked = check_cells_against_exact("steane cycle", steane_sampled(), steane_exact(), n1, n2, EC)
    assert checked == (1 + 2 + 1 + 2 + 3) * 6


def test_weight_1_strata_hit_every_site_and_kind():
    """A table whose word 0 is the kind mask and whose word 1 carries the site: chi-square over the 126 x 3 and 102 x 15 cells."""
    cycle = steane_cycle()
    site_loc, n1, n2, _ = cycle.gate_sites()
    assert (n1 * 3, n2 * 15) == (378, 1530)
    eff = np.zeros((cycle.num_locations, 2, 2), dtype="<u8")
    for s, l in enumerate(site_loc.tolist()):
        for t in range(2 if s < n1 else 4):
            eff[l + (t >> 1), t & 1] = (1 << t, (s + 1) << (16 * t))
    for case, (a, b) in enumerate(((1, 0), (0, 1))):
        words, c = _native.gate_stratum_outcomes_host(eff, site_loc, n1, n2, a, b, EXACT_SAMPLES, SEED + case)
        kappa = words[:, 0].astype(np.int64)
        lowest = np.array([0, 0, 1, 0, 2, 0, 1, 0, 3, 0, 1, 0, 2, 0, 1, 0])[kappa]
        site = ((words[:, 1] >> (16 * lowest).astype(np.uint64)) & np.uint64(0xFFFF)).astype(np.int64) - 1
        nkinds, base, n = (3, 0, n1) if a else (15, n1, n2)
        assert kappa.min() >= 1 and kappa.max() <= nkinds and site.min() >= base and site.max() < base + n
        assert np.array_equal(c, ((kappa & 3) != 0) & ((kappa >> 2) != 0))
        table = np.bincount((site - base) * nkinds + kappa - 1, minlength=n * nkinds)
        assert table.min() > 0
        ed.assert_chi2("steane cycle (%d, %d) (site, kind)" % (a, b), table, np.full(n * nkinds, 1.0 / (n * nkinds)), EXACT_SAMPLES)


# ---- the estimator ----------------------------------------------------------------------------------------------------------------

TOY_FIELDS = ('accepted', 'wrong', 'trial_wrong')
TOY_N1, TOY_N2 = 5, 4


def class_size(n1, n2, w, b, c):
    return math.comb(n1, w - b) * math.comb(n2, b) * 3**(w - b) * math.comb(b, c) * 6**(b - c) * 9**c


def toy_exact(top=3):
    """n1 = 5, n2 = 4, weights 0 .. top with made-up counts (accepted >= wrong) inside every class's size."""
    rng = np.random.default_rng(SEED)
    counts = []
    for w in range(top + 1):
        stack = np.zeros((w + 1, w + 1, 3), dtype=np.uint64)
        for b in range(w + 1):
            for c in range(b + 1):
                size = class_size(TOY_N1, TOY_N2, w, b, c)
                acc = int(rng.integers(size // 3, size + 1)) if w else 1
                wrong = int(rng.integers(0, acc // 2 + 1)) if w else 0
                stack[b, c] = (acc, wrong, wrong + int(rng.integers(0, 3)))
        counts.append(stack)
    return GateStrata(TOY_N1, TOY_N2, range(top + 1), counts, TOY_FIELDS)


def sampled_at_exact_fractions(exact, weights, scale=4):
    """N_{a,b} = scale C(n1, a) C(n2, b) 3^a 15^b samples: `scale` times the exact counts are the expected tallies, whole numbers."""
    strata, samples, counts = [], [], []
    for w in weights:
        for b in range(max(0, w - exact.n1), min(w, exact.n2) + 1):
            a = w - b
            strata.append((a, b))
            samples.append(scale * math.comb(exact.n1, a) * math.comb(exact.n2, b) * 3**a * 15**b)
            rows = np.zeros((17, len(exact.fields)), dtype=np.uint64)
            rows[:b + 1] = np.uint64(scale) * exact.counts[exact.weights.index(w)][b, :b + 1]
            counts.append(rows)
    return SampledGateStrata(exact.n1, exact.n2, strata, samples, counts, exact.fields)


ODDS = (GateStrata.depolarising_odds(0.03, 0.05), GateStrata.independent_odds(0.04), GateStrata.depolarising_odds(1e-9, 1e-9))


def close(a, b, rel=1e-12):
    return abs(a - b) <= rel * abs(b)


def test_counts_at_the_exact_fractions_reproduce_the_exact_joint_and_rate():
    exact = toy_exact()
    for head in (0, 1, 3):                                                    # exact weights 0 .. head - 1, the others sampled
        sampled = sampled_at_exact_fractions(exact, range(head, 4))
        part = GateStrata(TOY_N1, TOY_N2, range(head), exact.counts[:head], TOY_FIELDS) if head else None
        merged = part.merged(sampled) if head else MergedGateStrata(None, [sampled])
        assert isinstance(merged, MergedGateStrata)
        for odds in ODDS:
            for field in TOY_FIELDS:
                assert close(merged.joint(odds, field), exact.joint(odds, field)), (head, odds, field)
            got, want = merged.rate(odds, 'wrong'), exact.rate(odds, 'wrong')
            assert isinstance(got, montecarlo.PostSelectedRate)
            assert all(close(g, w) for g, w in zip((got.estimate, got.lower, got.upper), want)), (head, odds)
            assert all(close(g, w) for g, w in zip(merged.acceptance(odds), exact.acceptance(odds)))
            assert merged._missing_mass(odds) == exact._missing_mass(odds)    # the covered set is whole weights
            assert got.stderr > 0
    alone = sampled_at_exact_fractions(exact, range(4)).rate(ODDS[0], 'wrong')                      # SampledGateStrata's own rate
    assert all(close(g, w) for g, w in zip((alone.estimate, alone.lower, alone.upper), exact.rate(ODDS[0], 'wrong')))
    whole = exact.merged(sampled_at_exact_fractions(exact, [2, 3])).rate(ODDS[0], 'wrong')
    assert whole.stderr == 0.0 and (whole.estimate, whole.lower, whole.upper) == exact.rate(ODDS[0], 'wrong')


def test_merged_prefers_the_exact_weight_and_counts_cells_as_covered():
    exact = toy_exact(2)
    fields = exact.fields
    rows = lambda *cells: np.concatenate((np.array(cells, dtype=np.uint64).reshape(-1, 3), np.zeros((17 - len(cells), 3), dtype=np.uint64)))
    three = SampledGateStrata(TOY_N1, TOY_N2, [(2, 1)], [5000], [rows((900, 100, 120), (700, 90, 95))], fields)
    both = SampledGateStrata(TOY_N1, TOY_N2, [(1, 1), (2, 1)], [4000, 5000],
                             [rows((10, 5, 5), (10, 5, 5)), rows((900, 100, 120), (700, 90, 95))], fields)
    odds = ODDS[0]
    assert exact.merged(both).rate(odds, 'wrong') == exact.merged(three).rate(odds, 'wrong')       # (1, 1) has weight 2: the exact one is used
    assert exact.merged(both).strata == [(2, 1)] and exact.merged(three).rate(odds, 'wrong').stderr > 0
    # T: everything but the weights 0 .. 2 and the one cell (2, 1)
    x, y1, y2 = odds
    p_a = montecarlo.binomial_weights(TOY_N1, 3 * x / (1 + 3 * x))
    p_b = montecarlo.binomial_weights(TOY_N2, 15 * y1 / (1 + 15 * y1))
    covered = sum(p_a[a] * p_b[b] for a in range(6) for b in range(5) if a + b <= 2 or (a, b) == (2, 1))
    d, d_t = exact.merged(three).acceptance(odds)
    assert abs((d_t - d) - (1.0 - covered)) < 1e-15
    assert close(exact.merged(three)._missing_mass(odds), exact._missing_mass(odds) - p_a[2] * p_b[1], 1e-12)
    # a stratum without samples covers nothing; one with nothing accepted is covered and contributes nothing
    empty = SampledGateStrata(TOY_N1, TOY_N2, [(2, 1), (3, 0)], [5000, 0], [rows((900, 100, 120), (700, 90, 95)), rows()], fields)
    assert exact.merged(empty).strata == [(2, 1)]
    barren = SampledGateStrata(TOY_N1, TOY_N2, [(3, 0)], [100], [rows()], fields)
    got = exact.merged([three, barren])
    assert got.strata == [(2, 1), (3, 0)] and got.joint(odds) == exact.merged(three).joint(odds)
    assert close(got._missing_mass(odds), exact.merged(three)._missing_mass(odds) - p_a[3] * p_b[0], 1e-12)
    assert got.rate(odds, 'wrong').stderr == exact.merged(three).rate(odds, 'wrong').stderr
    # a whole sampled anti-diagonal covers its weight like an exact stratum
    full = sampled_at_exact_fractions(toy_exact(3), [3])
    assert exact.merged(full)._missing_mass(odds) == toy_exact(3)._missing_mass(odds)


def test_refusals_of_the_merge():
    exact = toy_exact(1)
    rows = np.zeros((17, 3), dtype=np.uint64)
    rows[0] = (100, 20, 25)
    ok = SampledGateStrata(TOY_N1, TOY_N2, [(2, 1)], [500], [rows], TOY_FIELDS)
    with pytest.raises(ValueError, match="sampled twice"):
        exact.merged([ok, SampledGateStrata(TOY_N1, TOY_N2, [(3, 0), (2, 1)], [10, 10], [rows, rows], TOY_FIELDS)])
    with pytest.raises(ValueError, match=r"\(n1, n2\)"):
        exact.merged(SampledGateStrata(TOY_N1 + 1, TOY_N2, [(2, 1)], [500], [rows], TOY_FIELDS))
    with pytest.raises(ValueError, match=r"\(n1, n2\)"):
        exact.merged(SampledGateStrata(TOY_N1, TOY_N2 + 1, [(2, 1)], [500], [rows], TOY_FIELDS))
    with pytest.raises(ValueError, match="fields"):
        exact.merged(SampledGateStrata(TOY_N1, TOY_N2, [(2, 1)], [500], [rows[:, :2]], ('accepted', 'wrong')))
    with pytest.raises(ValueError, match="sum"):
        exact.merged(ok).rate(ODDS[0], 'trial_wrong')
    with pytest.raises(ValueError, match="sum"):
        ok.rate(ODDS[0], 'trial_wrong')
    with pytest.raises(ValueError, match="no field"):
        ok.rate(ODDS[0], 'logical_any')
    with pytest.raises(ValueError, match="distinct"):
        SampledGateStrata(TOY_N1, TOY_N2, [(2, 1), (2, 1)], [1, 1], [rows, rows], TOY_FIELDS)
    with pytest.raises(ValueError, match="accepted"):
        SampledGateStrata(TOY_N1, TOY_N2, [(2, 1)], [1], [rows[:, :2]], ('wrong', 'accepted'))
    with pytest.raises(ValueError, match="a \\+ b <= 16"):
        SampledGateStrata(20, 20, [(9, 8)], [1], [rows], TOY_FIELDS)
    with pytest.raises(ValueError, match="n1 = 5"):
        SampledGateStrata(TOY_N1, TOY_N2, [(6, 0)], [1], [rows], TOY_FIELDS)
    with pytest.raises(ValueError, match="no accepted"):
        SampledGateStrata(TOY_N1, TOY_N2, [(2, 1)], [10], [0 * rows], TOY_FIELDS).rate(ODDS[0], 'wrong')
    with pytest.raises(ValueError, match="no strata"):
        MergedGateStrata(None, [])
    with pytest.raises(ValueError, match="negative"):
        ok.rate((-1.0, 0.1, 0.1), 'wrong')


def test_stderr_of_one_sampled_stratum_is_the_binomial_error_of_the_ratio():
    """y1 = y2: every class of the stratum weighs the same, so the error is sqrt(R (1 - R) / (N a)) with a the accepted fraction."""
    rows = np.zeros((17, 3), dtype=np.uint64)
    rows[:3] = ((1500, 100, 0), (700, 150, 0), (300, 50, 0))
    sampled = SampledGateStrata(50, 40, [(1, 2)], [10000], [rows], TOY_FIELDS)
    for odds in (GateStrata.depolarising_odds(1e-3, 2e-3), GateStrata.depolarising_odds(0.2, 0.1)):
        got = sampled.rate(odds, 'wrong')
        r = 300 / 2500
        assert abs(got.estimate - r) < 1e-15
        assert close(got.stderr, math.sqrt(r * (1 - r) / (10000 * 0.25)))
        assert got.lower <= got.estimate <= got.upper
        x, y, _ = odds
        mass = montecarlo.binomial_weights(50, 3 * x / (1 + 3 * x))[1] * montecarlo.binomial_weights(40, 15 * y / (1 + 15 * y))[2]
        assert close(got.lower, mass * 0.03 / (mass * 0.25 + 1.0 - mass)) and close(got.upper, (mass * 0.03 + 1.0 - mass) / (mass * 0.25 + 1.0 - mass))
    # y1 != y2: the classes weigh differently and the estimate is no longer the pooled ratio
    x = 0.01
    got = sampled.rate((x, x, x * x), 'wrong')
    w = np.array([1.0, x, x * x])
    want = float((w * [100, 150, 50]).sum() / (w * [1500, 700, 300]).sum())
    assert close(got.estimate, want) and abs(want - r) > 1e-3


def test_two_strata_by_hand():
    """n1 = n2 = 1, odds (x, y, y) with 3 x = 1 and 15 y = 1: Z = 1/4, and the strata (1, 0) and (0, 1) both have mass 1/4 -- the
    numbers of test_gadget_strata.test_two_strata_by_hand with B = (1/4, 1/4).  (1, 0): 100 samples, 40 accepted, 10 wrong; (0, 1):
    200 samples, 50 accepted (30 in class 0, 20 in class 1), 20 wrong (12 and 8)."""
    rows_1, rows_2 = np.zeros((17, 2), dtype=np.uint64), np.zeros((17, 2), dtype=np.uint64)
    rows_1[0] = (40, 10)
    rows_2[:2] = ((30, 12), (20, 8))
    sampled = SampledGateStrata(1, 1, [(1, 0), (0, 1)], [100, 200], [rows_1, rows_2], ('accepted', 'wrong'))
    odds = (1.0 / 3.0, 1.0 / 15.0, 1.0 / 15.0)
    got = sampled.rate(odds, 'wrong')
    n, d, t = 0.25 * 0.1 + 0.25 * 0.1, 0.25 * 0.4 + 0.25 * 0.25, 0.5
    r = n / d
    assert close(got.estimate, r) and close(got.lower, n / (d + t)) and close(got.upper, (n + t) / (d + t))
    v_1 = 0.1 * (1 - r)**2 + 0.3 * r**2 - (0.1 - 0.4 * r)**2
    v_2 = 0.1 * (1 - r)**2 + 0.15 * r**2 - (0.1 - 0.25 * r)**2
    assert close(got.stderr, math.sqrt(0.0625 * v_1 / 100 + 0.0625 * v_2 / 200) / d)
    assert all(close(g, w) for g, w in zip(sampled.acceptance(odds), (d, d + t))) and close(sampled.joint(odds, 'wrong'), n)


SPREAD_RUNS, SPREAD_SAMPLES = 200, 4096
SPREAD_STRATA = ((2, 0), (1, 1), (0, 2))


def test_stderr_agrees_with_the_spread_of_the_estimate():
    """200 disjoint first_sample ranges of the host sampler, each merged with the exact weights 0 and 1 of the one-round Steane
    cycle.  The pooled run's stderr predicts each run's variance: sigma^2 = 200 stderr_pooled^2 (the variance goes as 1 / N).  Under
    the delta method (199) S^2 / sigma^2 is chi-square with 199 degrees of freedom; the case fails below 10^-6 in either tail."""
    cycle = steane_cycle()
    exact = steane_exact(1)
    odds = GateStrata.depolarising_odds(1e-2, 1e-2)
    firsts = [r * SPREAD_SAMPLES for r in range(SPREAD_RUNS)]
    estimates, total = [], None
    for first in firsts:
        run = cycle.gate_strata(SPREAD_STRATA, SPREAD_SAMPLES, seed=SEED, first_sample=first, host=True)
        estimates.append(exact.merged(run).rate(odds, 'logical_any').estimate)
        total = run.counts.copy() if total is None else total + run.counts
    pooled = SampledGateStrata(run.n1, run.n2, SPREAD_STRATA, [SPREAD_RUNS * SPREAD_SAMPLES] * 3, total, EC)
    whole = cycle.gate_strata(SPREAD_STRATA, SPREAD_RUNS * SPREAD_SAMPLES, seed=SEED, host=True)
    assert np.array_equal(whole.counts, total)                                # the counts of disjoint ranges add
    rate = exact.merged(pooled).rate(odds, 'logical_any')
    sigma2 = SPREAD_RUNS * rate.stderr**2
    s2 = float(np.var(estimates, ddof=1))
    stat = (SPREAD_RUNS - 1) * s2 / sigma2
    ed.assert_chi2_stat("spread of %d estimates against the delta-method error" % SPREAD_RUNS, stat, SPREAD_RUNS - 1)
    assert abs(float(np.mean(estimates)) - rate.estimate) < 6.0 * rate.stderr   # (the ratio's bias is of order 1 / N)
    assert rate.lower <= rate.estimate <= rate.upper and rate.stderr > 0


def test_merged_rate_of_the_cycle_lies_inside_the_exact_bounds():
    exact = steane_exact(1)
    odds = GateStrata.depolarising_odds(1e-3, 1e-3)
    est, lower, upper = exact.rate(odds, 'logical_any')
    got = exact.merged(steane_sampled()).rate(odds, 'logical_any')
    assert lower <= got.lower <= got.estimate <= got.upper <= upper and got.stderr > 0
    assert got.upper - got.lower < 0.1 * (upper - lower)
    full = steane_exact(2).rate(odds, 'logical_any')
    assert abs(got.estimate - full[0]) < 6.0 * got.stderr


# ---- refused arguments ------------------------------------------------------------------------------------------------------------

def test_refused_arguments_of_the_host_entry_point():
    cycle = steane_cycle()
    site_loc, n1, n2, _ = cycle.gate_sites()
    eff = cycle.effects

    def call(eff=eff, sites=site_loc, n1=n1, n2=n2, a=1, b=1, count=4, first=0, ldw=None):
        return _native.gate_stratum_outcomes_host(eff, sites, n1, n2, a, b, count, 0, first, ldw)

    overlap = site_loc.copy()
    overlap[1] = overlap[0]
    small = (np.zeros((17, 2, 3), dtype="<u8"), np.arange(17, dtype=np.int32), 17, 0)
    mixed = (small[0], np.array([0, 1, 2, 3, 5, 7, 9, 11, 13, 15], dtype=np.int32), 3, 7)          # n1 = 3, n2 = 7 over the same L = 17
    for fn, text in ((lambda: call(a=9, b=8), r"a \+ b <= 16"), (lambda: call(a=17, b=0), r"a \+ b <= 16"), (lambda: call(a=-1), "a, b >= 0"),
                     (lambda: call(*mixed, a=4, b=0), r"a <= n_1 = 3"), (lambda: call(*small, a=3, b=1), r"b <= n_2 = 0"),
                     (lambda: call(sites=overlap), "no partition"), (lambda: call(n1=n1 - 1, sites=site_loc[1:]), "no partition"),
                     (lambda: call(count=-1), "count >= 0"), (lambda: call(first=-1), "first_sample >= 0"), (lambda: call(ldw=2), "ldw"),
                     (lambda: call(np.zeros((4, 2, 17), dtype="<u8"), np.arange(4, dtype=np.int32), 4, 0), "ldr <= 16")):
        with pytest.raises(_native.GF2Error, match=text) as err:
            fn()
        assert err.value.code == _native.GF2_E_ARG and "gf2_gate_stratum_outcomes_host" in err.value.message, text
    assert call(*small, a=16, b=0, count=3)[0].shape == (3, 3)
    lib = _native.lib()
    out, two = np.zeros(3, dtype="<u8"), np.zeros(1, dtype=np.uint8)
    sites = small[1]
    assert lib.gf2_gate_stratum_outcomes_host(None, 17, 3, sites.ctypes.data, 17, 0, 1, 0, 0, 0, 1, out.ctypes.data, 3, two.ctypes.data) == _native.GF2_E_ARG
    assert lib.gf2_gate_stratum_outcomes_host(small[0].ctypes.data, 17, 3, sites.ctypes.data, 17, 0, 1, 0, 0, 0, 1, None, 3, two.ctypes.data) == _native.GF2_E_ARG
    assert b"null buffer" in lib.gf2_last_error()
    assert lib.gf2_gate_stratum_outcomes_host(small[0].ctypes.data, 17, 3, None, 17, 0, 1, 0, 0, 0, 1, out.ctypes.data, 3, two.ctypes.data) == _native.GF2_E_ARG
    assert b"no partition" in lib.gf2_last_error()
    assert lib.gf2_gate_stratum_outcomes_host(small[0].ctypes.data, 17, 3, sites.ctypes.data, 17, 0, 1, 0, 0, 0, 0, None, 3, None) == _native.GF2_OK


def test_refused_requests_of_the_python_entry_points():
    cycle = steane_cycle()
    _, n1, n2, _ = cycle.gate_sites()
    for call, text in ((lambda: cycle.gate_strata([(9, 8)], 10, host=True), r"a \+ b <= 16"),
                       (lambda: cycle.gate_strata([(-1, 2)], 10, host=True), "a, b >= 0"),
                       (lambda: cycle.gate_strata([(1, 1)], -1, host=True), "negative sample count"),
                       (lambda: cycle.gate_strata([(1, 1)], 10, first_sample=-1, host=True), "negative first sample"),
                       (lambda: cycle.gate_strata([(1, 1), (1, 1)], 10, host=True), "distinct")):
        with pytest.raises(ValueError, match=text):
            call()
    assert cycle.gate_strata([(0, 16)], 10, host=True).counts.shape == (1, 17, 8)
    with pytest.raises(ValueError, match="n2 = 2"):
        montecarlo.gate_strata_local(3, 2, FT, [(1, 3)], 1, 0, None)
    with pytest.raises(ValueError, match="n1 = 3"):
        montecarlo.gate_strata_local(3, 9, FT, [(4, 1)], 1, 0, None)


def test_device_entry_points_refuse_null_arguments_without_a_device():
    lib = _native.lib()
    counts = np.zeros(17 * 8, dtype=np.uint64)
    wa, wb, samples, sites = np.array([1], dtype=np.int32), np.array([1], dtype=np.int32), np.array([1], dtype=np.int64), np.zeros(3, dtype=np.int32)
    tail = (sites.ctypes.data, 1, 1, 0, 0, 1, wa.ctypes.data, wb.ctypes.data, samples.ctypes.data, counts.ctypes.data)
    assert lib.gf2_mc_ec_decode_gate_strata(None, None, 1, 3, None, None, 0, 3, None, None, 0, *tail) == _native.GF2_E_ARG
    assert b"gf2_mc_ec_decode_gate_strata: null argument" in lib.gf2_last_error()
    assert lib.gf2_mc_ft_decode_gate_strata(None, None, 7, 0b0010101, 3, None, None, 0, 3, None, None, 0, *tail) == _native.GF2_E_ARG
    assert b"gf2_mc_ft_decode_gate_strata: null argument" in lib.gf2_last_error()
    assert not counts.any()
