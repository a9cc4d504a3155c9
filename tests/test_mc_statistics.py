"""
Is the sampler RIGHT?  (CPU leg; the GPU leg is tests/test_gpu_mc_statistics.py.)

The parity tests prove that the three statements of the sampler (HIP, oracle/gf2_oracle.c, oracle/cpu_ref.py) agree bit for bit.
These tests compare what the definition produces -- through the C oracle -- with exact distributions (oracle/exact_dist.py:
closed forms, no sampling), and the integer count table with the exact binomial in rational arithmetic.

Acceptance: every statistic becomes a p-value and a case fails at p < 10^-6 in EITHER tail (a histogram too regular fails
too).  Seeds are fixed as SEED0 + case index and are not to be changed: a failure is a finding.  Run with -s to see every
p-value.
"""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import c_oracle, cpu_ref, exact_dist as ed
from quantum_css_codes_amd import _native
from quantum_css_codes_amd.circuit_noise import FaultCircuit, fault_locations
from quantum_css_codes_amd.montecarlo import dense_table, packed_word

SEED0 = 20261017
STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
RATES = [(0.01, 0.005, 0.02), (1e-3, 1e-3, 1e-3), (0.2, 0.1, 0.3), (0.01, 0.0, 0.0), (0.0, 0.01, 0.0), (0.0, 0.0, 0.01)]
FIRSTS = [0, (1 << 32) + 12345, (1 << 40) + 777]
G = cpu_ref.GOLDEN
M64 = (1 << 64) - 1


@functools.lru_cache(maxsize=None)
def make_code(name):
    if name == "steane":
        return cpu_ref.CSSCode(STEANE, STEANE)
    cols = np.arange(1, 16)
    h1 = np.array([(cols >> b) & 1 for b in range(4)])
    return cpu_ref.CSSCode(h1, np.vstack([h1] + [h1[a] & h1[b] for a in range(4) for b in range(a + 1, 4)]))


check_chi2, check_stat, check_z, pair_table = ed.assert_chi2, ed.assert_chi2_stat, ed.assert_z, ed.pair_table


# ---- 1: the helpers themselves -----------------------------------------------------------------------------------------

def test_fwht_is_the_sign_matrix_and_the_marginal_is_the_enumeration():
    rng = np.random.default_rng(1)
    a = rng.random(64)
    s = np.arange(64)
    signs = np.array([[(-1.0) ** bin(x & y).count("1") for y in s] for x in s])
    assert np.allclose(ed.fwht(a.copy()), signs @ a, rtol=0, atol=1e-12)
    # Steane, q = 0.1: all 2^7 errors by hand
    q, want = 0.1, np.zeros(8)
    for e in range(128):
        bits = np.array([(e >> j) & 1 for j in range(7)])
        key = int(cpu_ref.vec_to_int(np.mod(STEANE @ bits, 2)))
        want[key] += q ** bits.sum() * (1 - q) ** (7 - bits.sum())
    assert np.allclose(ed.marginal(STEANE, q), want, rtol=0, atol=1e-15)
    assert np.allclose(ed.weight_projection(ed.marginal(STEANE, q), 3),
                       [want[0], want[1] + want[2] + want[4], want[3] + want[5] + want[6], want[7]], rtol=0, atol=1e-15)
    mean, var = ed.syndrome_weight_mean_var(STEANE, q)
    w = np.array([bin(k).count("1") for k in range(8)])
    assert abs(mean - (want * w).sum()) < 1e-14 and abs(var - ((want * w * w).sum() - (want * w).sum() ** 2)) < 1e-14


def test_code_capacity_joint_by_enumeration_and_its_marginals():
    code, p = make_code("steane"), (0.03, 0.02, 0.05)
    joint = ed.code_capacity_joint(code, *p)
    want = np.zeros(256)
    z_op, x_op = code.z_operator_matrix()[0], code.x_operator_matrix()[0]
    for e in range(4 ** 7):
        kinds = [(e >> (2 * j)) & 3 for j in range(7)]                         # 0 none, 1 X, 2 Y, 3 Z
        e_x = np.array([1 if k in (1, 2) else 0 for k in kinds])
        e_z = np.array([1 if k in (2, 3) else 0 for k in kinds])
        prob = math.prod((1 - sum(p), p[0], p[1], p[2])[k] for k in kinds)
        cell = int(cpu_ref.vec_to_int(cpu_ref.syndrome_product(code.parity_check_c2, e_x))) \
            | int(cpu_ref.vec_to_int(cpu_ref.syndrome_product(code.parity_check_c1, e_z))) << 3 \
            | (int(np.dot(z_op, e_x)) & 1) << 6 | (int(np.dot(x_op, e_z)) & 1) << 7
        want[cell] += prob
    assert np.allclose(joint.prob, want, rtol=0, atol=1e-15)
    assert np.allclose(joint.hist_z(), ed.marginal(code.parity_check_c1, p[1] + p[2]), rtol=0, atol=1e-15)
    assert np.allclose(joint.hist_x(), ed.marginal(code.parity_check_c2, p[0] + p[1]), rtol=0, atol=1e-15)


def test_chi2_tails_against_scipy():
    stats = pytest.importorskip("scipy.stats")
    worst = 0.0
    for dof in (1, 2, 7, 48, 255, 1023, 65535, 1 << 20):
        sd = math.sqrt(2.0 * dof)
        for dev in (-7.2, -5.0, -2.0, -0.3, 0.0, 0.4, 2.0, 5.0, 7.5):         # tails down to about 10^-12 on either side
            x = dof + dev * sd if dof > 60 else dof * math.exp(dev / 2.0)
            low, up = ed.chi2_tails(x, dof)
            for got, want in ((low, float(stats.chi2.cdf(x, dof))), (up, float(stats.chi2.sf(x, dof)))):
                if want > 1e-13:
                    worst = max(worst, abs(got / want - 1.0))
    # the prefactor exp(a ln x - x - lgamma a) cancels terms of up to 10^7: 10^7 * 2^-52 = 2 * 10^-9 relative, a few times over
    assert worst < 1e-7, worst
    assert abs(ed.z_to_p(4.891638) / 1e-6 - 1.0) < 1e-3 and ed.z_to_p(0.0) == 1.0
    for z in (0.5, 3.0, 6.0):
        assert abs(ed.z_to_p(z) / (2.0 * float(stats.norm.sf(z))) - 1.0) < 1e-12


def test_pooled_chi2_keeps_every_sample():
    prob = np.array([0.9, 0.0995, 4e-4, 5e-5, 5e-5])
    obs = np.array([9000, 995, 4, 1, 0])
    chi2, dof = ed.pooled_chi2(obs, prob, 10000)
    assert dof == 1                                                            # rest bin expects 5 < 10: joins the smallest kept bin
    assert abs(chi2 - ((9000 - 9000) ** 2 / 9000 + (1000 - 1000) ** 2 / 1000)) < 1e-9
    with pytest.raises(AssertionError, match="rest bin"):
        ed.pooled_chi2([360, 32, 8], [0.9, 0.08, 0.02], 400)
    assert ed.pooled_chi2([10, 0], [1.0, 0.0], 10) == (0.0, 0) and ed.pooled_chi2([9, 1], [1.0, 0.0], 10)[0] == float("inf")


# ---- 2: the count table against the exact binomial -----------------------------------------------------------------------

TABLE_NB = (1, 7, 15, 63, 64, 65, 300, 511, 512)
TABLE_P = (1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 0.01, 0.05, 0.1, 0.3, 0.49, 0.5 - 2.0**-32, 0.5, 0.5 + 2.0**-32, 0.51, 0.7, 0.9,
           0.99, 1 - 1e-3, 1 - 1e-4, 1 - 1e-5, 1 - 1e-6)
# Half a unit of 2^-32 is the rounding of the table's entries.  The float64 error of the recurrence (at most 512 steps of a few
# ulp each on values below 1: about 10^-13, 5 * 10^-4 units) could push an entry over a rounding boundary; measured on this whole
# grid against exact rationals it never does: the worst excess over half a unit is zero (DESIGN.md section 5 "Distribution").
TABLE_MEASURED_EXCESS = 0


def table_error_units(t_any, nb):
    """max over k of |table[k] - 2^32 P(Bin(nb, t_any / 2^32) <= k)| in units of 2^-32, exact integers until the last step."""
    table = cpu_ref.binomial_cdf_table(t_any, nb)
    other, shift, cum, worst = (1 << 32) - t_any, 32 * (nb - 1), 0, Fraction(0)
    for k in range(nb):
        cum += math.comb(nb, k) * t_any**k * other**(nb - k)                   # 2^(32 nb) P(K <= k)
        worst = max(worst, Fraction(abs((table[k] << shift) - cum), 1 << shift))
    return worst


@pytest.mark.parametrize("nb", TABLE_NB)
def test_count_table_against_the_exact_binomial(nb):
    worst = Fraction(0)
    for p_t in TABLE_P:
        t_any = cpu_ref.quantise_probability(p_t)
        assert abs(Fraction(t_any, 1 << 32) - Fraction(p_t)) <= Fraction(1, 1 << 33)     # gf2_quantise: to nearest
        err = table_error_units(t_any, nb)
        worst = max(worst, err)
        assert err <= Fraction(1, 2) + Fraction(TABLE_MEASURED_EXCESS), (nb, p_t, float(err))
    print("COUNT-TABLE nb %3d: worst |table - exact| = %.6f units of 2^-32 (excess over 1/2: %.3g)"
          % (nb, float(worst), max(0.0, float(worst) - 0.5)))
    assert float(worst) - 0.5 <= TABLE_MEASURED_EXCESS + 1e-12, float(worst)     # the figure DESIGN.md states is the figure measured


def test_quantisation_floor_of_the_steane_logical_error_rate():
    """Designed distribution (K from the integer table, a uniform subset, i.i.d. kinds from the integer thresholds) against the
    ideal i.i.d. one, exactly by enumeration of the 4^7 Pauli errors grouped by (weight, kinds).  Only the direction and the
    table's own bound are asserted; the four figures are in DESIGN.md section 5 "Distribution"."""
    code = make_code("steane")
    z_op, x_op = code.z_operator_matrix()[0], code.x_operator_matrix()[0]
    fails = []                                                                 # (weight, #X, #Y, #Z) of every error that ends in a logical flip
    for e in range(4 ** 7):
        kinds = [(e >> (2 * j)) & 3 for j in range(7)]
        e_x = np.array([1 if k in (1, 2) else 0 for k in kinds])
        e_z = np.array([1 if k in (2, 3) else 0 for k in kinds])
        flips = []
        for err, check, table, op in ((e_x, code.parity_check_c2, code._c2_syndromes, z_op),
                                      (e_z, code.parity_check_c1, code._c1_syndromes, x_op)):
            key = int(cpu_ref.vec_to_int(cpu_ref.syndrome_product(check, err)))
            corr = table[key] if key in table else np.zeros(7, dtype=int)
            flips.append(int(np.dot(op, np.mod(err + corr, 2))) & 1)
        if flips[0] or flips[1]:
            fails.append((kinds.count(1), kinds.count(2), kinds.count(3)))
    rel, lines = [], []
    for p in (1e-3, 1e-4, 1e-5, 1e-6):
        p_x = p_y = p_z = p / 3
        t_any, t_1, t_2 = cpu_ref.pauli_thresholds(p_x, p_y, p_z)
        table = cpu_ref.binomial_cdf_table(t_any, 7)
        p_k = [Fraction(table[k] - (table[k - 1] if k else 0), 1 << 32) for k in range(8)]
        kind = (Fraction(t_1, 1 << 32), Fraction(t_2 - t_1, 1 << 32), Fraction((1 << 32) - t_2, 1 << 32))
        designed = sum(p_k[a + b + c] / math.comb(7, a + b + c) * kind[0]**a * kind[1]**b * kind[2]**c for a, b, c in fails)
        fx, fy, fz, rest = Fraction(p_x), Fraction(p_y), Fraction(p_z), 1 - Fraction(p_x) - Fraction(p_y) - Fraction(p_z)
        ideal = sum(fx**a * fy**b * fz**c * rest**(7 - a - b - c) for a, b, c in fails)
        rel.append(float((designed - ideal) / ideal))
        lines.append("QUANTISATION p = %g: ideal %.6e designed %.6e relative error %+.3e" % (p, float(ideal), float(designed), rel[-1]))
        # bound: each P(K = k) is off by at most two table entries' errors (1/2 + excess units each), the rate by 2^-33 (an
        # event of 7 qubits moves by at most 7 times that), each of at most 7 kinds by three thresholds' 2^-33 relative to >= 1/4
        bound = (8 * (1 + 2 * TABLE_MEASURED_EXCESS) + 3.5) * 2.0**-32 + float(ideal) * 7 * 3 * 4 * 2.0**-33
        assert abs(float(designed - ideal)) <= bound, (p, float(designed), float(ideal), bound)
    print("\n".join(lines))
    assert abs(rel[0]) < abs(rel[1]) < abs(rel[2]) <= abs(rel[3]), rel             # the error grows as p falls
    assert abs(rel[0]) < 1e-3 and abs(rel[3]) > 0.1                             # trustworthy at 10^-3, not at 10^-6


# ---- 3: the definition through the C oracle ------------------------------------------------------------------------------

MARGINAL_CASES = [(name, rates) for name in ("steane", "rm15") for rates in RATES]


@pytest.mark.parametrize("case", range(len(MARGINAL_CASES)))
def test_oracle_marginal_histograms(case):
    name, p = MARGINAL_CASES[case]
    code, count, first = make_code(name), 10**7, FIRSTS[case % 3]
    h1, h2 = code.parity_check_c1, code.parity_check_c2
    hz, hx = c_oracle.mc(c_oracle.pack_rows(h1), code.r_1, c_oracle.pack_rows(h2), code.r_2, code.n, SEED0 + case, first, count, *p, 0)
    label = "oracle mc %s p=%s first=%d" % (name, p, first)
    check_chi2(label + " hist_z", hz, ed.marginal(h1, p[1] + p[2]), count)
    check_chi2(label + " hist_x", hx, ed.marginal(h2, p[0] + p[1]), count)


def checks_of_64_qubits():
    rng = np.random.default_rng(64)
    return rng.integers(0, 2, (10, 64)), rng.integers(0, 2, (9, 64))


def test_oracle_rates_close_to_one_on_64_qubits():
    """(1 - q)^64 underflows from q = 1 - 2^-17 on: the direct form of the count table then made every qubit err with certainty
    (found by test_count_table_against_the_exact_binomial; the complementary form now serves every segment length)."""
    hm1, hm2 = checks_of_64_qubits()
    count = 4 * 10**6
    for k, p in enumerate(((1 - 1e-5, 0.0, 0.0), (0.0, 1 - 1e-6, 0.0), (2e-6, 0.0, 1 - 3e-6))):
        hz, hx = c_oracle.mc(c_oracle.pack_rows(hm1), 10, c_oracle.pack_rows(hm2), 9, 64, SEED0 + 15 + k, FIRSTS[k], count, *p, 0)
        check_chi2("oracle mc n=64 p=%s hist_z" % (p,), hz, ed.marginal(hm1, p[1] + p[2]), count)
        check_chi2("oracle mc n=64 p=%s hist_x" % (p,), hx, ed.marginal(hm2, p[0] + p[1]), count)
        assert int(hz.max()) < count or p[1] + p[2] == 0.0                     # some sample has a qubit without a Z component


def oracle_decode(code, seed, first, count, p):
    return c_oracle.mc_decode(c_oracle.pack_rows(code.parity_check_c1), code.r_1, c_oracle.pack_rows(code.parity_check_c2), code.r_2,
                              code.n, dense_table(code._c1_syndromes, code.r_1, code.n), dense_table(code._c2_syndromes, code.r_2, code.n),
                              packed_word(code.x_operator_matrix()[0]), packed_word(code.z_operator_matrix()[0]), seed, first, count, *p)


def exact_decode(code, p, count):
    joint = ed.code_capacity_joint(code, *p)
    return ed.expected_decode_counts(joint, code._c1_syndromes, code._c2_syndromes,
                                     (code.x_operator_matrix()[0], code.z_operator_matrix()[0]), count)


DECODE_CASES = [(name, rates) for name in ("steane", "rm15") for rates in RATES[:3]]
FIELDS = ('logical_x', 'logical_z', 'logical_any', 'uncorrectable_x', 'uncorrectable_z')


@pytest.mark.parametrize("case", range(len(DECODE_CASES)))
def test_oracle_decode_counts(case):
    name, p = DECODE_CASES[case]
    code, count, first = make_code(name), 10**7, FIRSTS[(case + 1) % 3]
    got = oracle_decode(code, SEED0 + 20 + case, first, count, p)
    mean, var = exact_decode(code, p, count)
    for f in range(5):
        check_z("oracle decode %s p=%s %s" % (name, p, FIELDS[f]), int(got[f]), mean[f], var[f])


def segments_of(n):
    return [(lo, min(n, lo + 512)) for lo in range(0, n, 512)]


def gather_position_statistics(n, seed, first, count, p, chunk=100000):
    """Per-qubit error counts; per (segment, K in 1..3) the number of such segments and their per-position counts; the (kind,
    position parity) table of every erroneous qubit."""
    per_qubit = np.zeros(n, dtype=np.int64)
    cond = {(s, k): [0, np.zeros(hi - lo, dtype=np.int64)] for s, (lo, hi) in enumerate(segments_of(n)) for k in (1, 2, 3)}
    kinds = np.zeros((3, 2), dtype=np.int64)
    for start in range(0, count, chunk):
        now = min(chunk, count - start)
        ex, ez = c_oracle.sample_errors(n, seed, first + start, now, *p)
        bx, bz = c_oracle.unpack_rows(ex, n, dtype=np.uint8), c_oracle.unpack_rows(ez, n, dtype=np.uint8)
        hit = bx | bz
        per_qubit += hit.sum(axis=0, dtype=np.int64)
        for s, (lo, hi) in enumerate(segments_of(n)):
            seg = hit[:, lo:hi]
            k_seg = seg.sum(axis=1, dtype=np.int64)
            for k in (1, 2, 3):
                rows = k_seg == k
                cond[(s, k)][0] += int(rows.sum())
                cond[(s, k)][1] += seg[rows].sum(axis=0, dtype=np.int64)
        for row, bits in enumerate((bx & (1 - bz), bx & bz, (1 - bx) & bz)):
            kinds[row, 0] += int(bits[:, 0::2].sum(dtype=np.int64))
            kinds[row, 1] += int(bits[:, 1::2].sum(dtype=np.int64))
    return per_qubit, cond, kinds


def conditioned_position_chi2(counts, segments, k):
    """Positions of the k erroneous qubits of `segments` segments of nb qubits are a uniform k-subset: per-position counts have
    mean M k / nb, variance M p (1 - p) and covariance -M p (1 - p) / (nb - 1), so sum (c - M p)^2 / (M p (1 - p)) (nb - 1) / nb
    is a chi-square on nb - 1 degrees of freedom."""
    nb = counts.size
    p = k / nb
    return float(((counts - segments * p) ** 2).sum() / (segments * p * (1 - p)) * (nb - 1) / nb), nb - 1


# (n, p_t): the rate puts K = 1..3 errors into the segments of 512; n = 1030 also at a rate that puts them into its last 6 qubits
# (the last segment of n = 513 is one qubit: nothing to choose)
POSITION_CASES = [(7, 0.2), (64, 0.03), (65, 0.03), (512, 0.004), (513, 0.004), (1030, 0.004), (1030, 0.3)]


@pytest.mark.parametrize("case", range(len(POSITION_CASES)))
def test_oracle_position_uniformity_and_floyd(case):
    n, p_t = POSITION_CASES[case]
    p, count, first = (0.5 * p_t, 0.2 * p_t, 0.3 * p_t), 10**6, FIRSTS[case % 3]
    per_qubit, cond, kinds = gather_position_statistics(n, SEED0 + 30 + case, first, count, p)
    label = "oracle positions n=%d p_t=%g" % (n, p_t)
    # every qubit errs independently at rate p_t: n independent binomials
    check_stat(label + " per-qubit", float(((per_qubit - count * p_t) ** 2).sum() / (count * p_t * (1 - p_t))), n)
    tested = 0
    for (s, k), (segs, counts) in sorted(cond.items()):
        nb = counts.size
        if k < nb and segs * k / nb >= ed.MIN_EXPECTED:                        # (k = nb leaves nothing to choose; too few: no statistic)
            check_stat(label + " segment %d given K=%d (%d segments)" % (s, k, segs), *conditioned_position_chi2(counts, segs, k))
            tested += 1
    assert tested >= (3 if n > 1 else 0)
    total = int(kinds.sum())
    assert total == int(per_qubit.sum())
    even = (n + 1) // 2
    prob = np.outer(np.array(p) / p_t, [even / n, (n - even) / n])
    check_chi2(label + " (kind, position parity)", kinds.reshape(-1), prob.reshape(-1), total)


def binomial_pmf(nb, q):
    return np.array([math.comb(nb, k) * q**k * (1 - q)**(nb - k) for k in range(nb + 1)])


def capped(pmf, cap):
    return np.append(pmf[:cap], pmf[cap:].sum())


def segment_counts(n, seed, first, count, p):
    ex, ez = c_oracle.sample_errors(n, seed, first, count, *p)
    hit = c_oracle.unpack_rows(ex | ez, n, dtype=np.uint8)
    return np.stack([hit[:, lo:hi].sum(axis=1, dtype=np.int64) for lo, hi in segments_of(n)], axis=1)


def test_oracle_independence_of_segments_samples_and_seeds():
    p_t, count, cap = 0.004, 10**6, 6
    p = (0.5 * p_t, 0.2 * p_t, 0.3 * p_t)
    k_dist = capped(binomial_pmf(512, p_t), cap)
    both = np.outer(k_dist, k_dist).reshape(-1)
    k = np.minimum(segment_counts(1024, SEED0 + 40, FIRSTS[1], count, p), cap)
    check_chi2("oracle independence (K_s, K_s+1) n=1024", pair_table(k[:, 0], k[:, 1], cap + 1), both, count)
    for start in (0, 1):                                                       # disjoint pairs (2m, 2m+1), then (2m+1, 2m+2)
        a, b = k[start:count - 1:2, 0], k[start + 1:count:2, 0]
        pairs = min(a.size, b.size)
        check_chi2("oracle independence (K_i, K_i+1) pairs from %d" % start, pair_table(a[:pairs], b[:pairs], cap + 1), both, pairs)
    other = np.minimum(segment_counts(1024, SEED0 + 41, FIRSTS[1], count, p), cap)       # the next seed, the same samples
    check_chi2("oracle independence (K under seed s, K under s+1)", pair_table(k[:, 0], other[:, 0], cap + 1), both, count)
    # Steane Z syndromes of consecutive samples, 64 bins
    ps = (0.03, 0.02, 0.05)
    _, ez = c_oracle.sample_errors(7, SEED0 + 42, FIRSTS[2], count, *ps)
    synd = np.mod(c_oracle.unpack_rows(ez, 7, dtype=np.int64) @ STEANE.T, 2)
    key = synd[:, 0] * 4 + synd[:, 1] * 2 + synd[:, 2]
    dist = ed.marginal(STEANE, ps[1] + ps[2])
    for start in (0, 1):
        a, b = key[start:count - 1:2], key[start + 1:count:2]
        pairs = min(a.size, b.size)
        check_chi2("oracle independence Steane (sigma_i, sigma_i+1) pairs from %d" % start, pair_table(a[:pairs], b[:pairs], 8),
                   np.outer(dist, dist).reshape(-1), pairs)


def test_seed_plus_golden_is_the_stream_shifted_by_one_sample():
    """Known property of the key mix64(seed + G (i + 1)): seed s + G gives sample i what seed s gives sample i + 1.  Callers
    vary first_sample, not the seed by arithmetic."""
    for n, seed in ((7, 5), (600, SEED0), (70, M64 - 3)):
        a = c_oracle.sample_errors(n, (seed + G) & M64, 10, 500, 0.02, 0.01, 0.03)
        b = c_oracle.sample_errors(n, seed, 11, 500, 0.02, 0.01, 0.03)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].any()
    e1 = cpu_ref.sample_pauli_error((9 + G) & M64, 4, 70, 0.1, 0.05, 0.1)
    e2 = cpu_ref.sample_pauli_error(9, 5, 70, 0.1, 0.05, 0.1)
    assert np.array_equal(e1[0], e2[0]) and np.array_equal(e1[1], e2[1])


# ---- circuit faults on the CPU: faults from the oracle's sampler, outcomes as ONE matrix product ----------------------------

def padded_encoder(code, total):
    gates = cpu_ref.encode_zero_gates(code)
    pad = total - len(fault_locations(gates))
    idle = np.array([(2, q % code.n, 0) for q in range(pad)], dtype=np.int32).reshape(-1, 3)
    return np.concatenate((idle[:pad // 2], gates, idle[pad // 2:]))


def circuit_cases():
    steane, rm = make_code("steane"), make_code("rm15")
    return [("steane encode_zero", steane, cpu_ref.encode_zero_gates(steane), (0.004, 0.003, 0.005)),
            ("steane encode_plus", steane, cpu_ref.encode_plus_gates(steane), (0.004, 0.003, 0.005)),
            ("rm15 encode_zero", rm, cpu_ref.encode_zero_gates(rm), (0.0006, 0.0003, 0.0006)),
            ("steane padded L=1025", steane, padded_encoder(steane, 1025), (0.001, 0.0005, 0.0015))]


def cells_by_matrix_product(effects, r_1, r_2, seed, first, count, p, chunk=100000):
    """Cell index of every sample: (f_x @ E_x + f_z @ E_z) mod 2 over the outcome bits."""
    total, m = effects.shape[0], r_1 + r_2 + 2
    cell = ed.pack_outcome_words(effects, r_1, r_2)                            # (L, 2)
    bits = [((cell[:, c, None] >> np.arange(m)) & 1).astype(np.float32) for c in (0, 1)]
    out = np.zeros(count, dtype=np.int64)
    for start in range(0, count, chunk):
        now = min(chunk, count - start)
        ex, ez = c_oracle.sample_errors(total, seed, first + start, now, *p)
        f_x, f_z = (c_oracle.unpack_rows(w, total, dtype=np.float32) for w in (ex, ez))
        got = (f_x @ bits[0] + f_z @ bits[1]).astype(np.int64) & 1
        out[start:start + now] = (got << np.arange(m)).sum(axis=1)
    return out


@pytest.mark.parametrize("case", range(4))
def test_oracle_circuit_faults_full_joint(case):
    name, code, gates, p = circuit_cases()[case]
    circ = FaultCircuit.for_code(code, gates)
    assert circ.num_locations == (21, 26, circ.num_locations, 1025)[case] and circ.ldr == 3
    count, first = 10**6, FIRSTS[case % 3]
    joint = ed.circuit_joint(circ.effects, *p, code.r_1, code.r_2)
    cells = cells_by_matrix_product(circ.effects, code.r_1, code.r_2, SEED0 + 50 + case, first, count, p)
    check_chi2("oracle circuit %s L=%d joint" % (name, circ.num_locations), np.bincount(cells, minlength=joint.prob.size), joint.prob, count)


def test_idle_circuit_joint_is_the_code_capacity_joint():
    for name in ("steane", "rm15"):
        code = make_code(name)
        circ = FaultCircuit.for_code(code, np.array([(2, q, 0) for q in range(code.n)], dtype=np.int32))
        p = (0.02, 0.01, 0.03)
        assert np.allclose(ed.circuit_joint(circ.effects, *p, code.r_1, code.r_2).prob, ed.code_capacity_joint(code, *p).prob,
                           rtol=0, atol=1e-15)


# ---- 6: the tests can fail --------------------------------------------------------------------------------------------------

def np_mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def numpy_segment(seed, first, count, nb, p_t, floyd_plus=1, index_and=M64):
    """NumPy copy of the sampler's first segment (count and positions, no kinds): (K, positions (count, max K), -1 = none).
    floyd_plus = 0 is the mutant that draws Floyd's t over j instead of j + 1; index_and masks bits of the sample index."""
    with np.errstate(over="ignore"):
        i = (np.arange(count, dtype=np.uint64) + np.uint64(first)) & np.uint64(index_and)
        ks = np_mix64(np.uint64(seed) + np.uint64(G) * (i + np.uint64(1)))
        d = np_mix64(ks + np.uint64(cpu_ref.STREAM_MULT))
        table = np.array(cpu_ref.binomial_cdf_table(cpu_ref.quantise_probability(p_t), nb)[:nb], dtype=np.uint64)
        k_err = np.searchsorted(table, d >> np.uint64(32), side="right").astype(np.int64)
        pos = np.full((count, int(k_err.max())), -1, dtype=np.int64)
        for k in range(pos.shape[1]):
            act = np.flatnonzero(k_err > k)
            v = np_mix64(d[act] + np.uint64(G) * np.uint64(k + 1))
            j = nb - k_err[act] + k
            t = (((v >> np.uint64(32)) * (j + floyd_plus).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
            taken = (pos[act, :k] == t[:, None]).any(axis=1)
            pos[act, k] = np.where(taken, j, t)
    return k_err, pos


def position_counts(k_err, pos, nb, k):
    rows = k_err == k
    return np.bincount(pos[rows, :k].reshape(-1), minlength=nb), int(rows.sum())


def smallest_rejected(reject, low=1e-6, high=1.0):
    """Smallest eps in [low, high] with reject(eps), by bisection on a geometric scale (reject is monotone here)."""
    assert reject(high) and not reject(low)
    for _ in range(40):
        mid = math.sqrt(low * high)
        low, high = (low, mid) if reject(mid) else (mid, high)
    return high


def test_numpy_copy_is_the_sampler():
    for nb, p_t in ((7, 0.2), (64, 0.05), (512, 0.004)):
        k_err, pos = numpy_segment(77, 1000, 20000, nb, p_t)
        ex, ez = c_oracle.sample_errors(nb, 77, 1000, 20000, 0.5 * p_t, 0.2 * p_t, 0.3 * p_t)
        hit = c_oracle.unpack_rows(ex | ez, nb, dtype=np.uint8)
        mine = np.zeros_like(hit)
        rows, cols = np.nonzero(pos >= 0)
        mine[rows, pos[rows, cols]] = 1
        assert np.array_equal(mine, hit) and np.array_equal(k_err, hit.sum(axis=1))


def test_mutants_are_rejected_and_resolving_power():
    """Each family of statistics on a deliberately wrong reference or sampler.  The smallest rate error (1 + eps) each rejects
    at p < 10^-6 is printed (RESOLVING lines) and recorded in DESIGN.md section 5 "Distribution"."""
    out = []
    # marginal family: Steane, N = 10^7 (the histograms of test_oracle_marginal_histograms case 0)
    code, p, count = make_code("steane"), RATES[0], 10**7
    h1, h2 = code.parity_check_c1, code.parity_check_c2
    hz, hx = c_oracle.mc(c_oracle.pack_rows(h1), 3, c_oracle.pack_rows(h2), 3, 7, SEED0, FIRSTS[0], count, *p, 0)

    def rejects(hist, prob, n):
        return not ed.chi2_verdict(*ed.pooled_chi2(hist, prob, n))[2]
    assert not rejects(hz, ed.marginal(h1, p[1] + p[2]), count)
    assert rejects(hz, ed.marginal(h1, p[0] + p[1]), count)                    # hist_z against hist_x's rate
    assert rejects(hx, ed.marginal(h2, p[1] + p[2]), count)
    eps = smallest_rejected(lambda e: rejects(hz, ed.marginal(h1, (p[1] + p[2]) * (1 + e)), count))
    mass = 1.0 - ed.marginal(h1, p[1] + p[2])[0]
    out.append("RESOLVING marginal: Steane hist_z N=1e7, rates x (1 + eps): eps >= %.2e rejected (5 / sqrt(N p_bin) = %.2e)"
               % (eps, 5 / math.sqrt(count * mass)))
    assert eps <= 10 / math.sqrt(count * mass)            # a shift of 10 standard deviations of the non-zero bins' mass cannot hide
    # decode family: z of logical_any under scaled rates
    got = oracle_decode(code, SEED0 + 20, FIRSTS[1], count, p)

    def decode_rejects(e):
        mean, var = exact_decode(code, tuple(v * (1 + e) for v in p), count)
        return any(not ed.z_verdict(int(got[f]), mean[f], var[f])[2] for f in range(3))
    assert not decode_rejects(0.0)
    eps = smallest_rejected(decode_rejects)
    mean, _ = exact_decode(code, p, count)
    out.append("RESOLVING decode counts: Steane N=1e7, rates x (1 + eps): eps >= %.2e rejected (5 / sqrt(N p_bin) / 2 = %.2e; "
               "the counts go as p^2)" % (eps, 2.5 / math.sqrt(mean[2])))
    assert eps <= 10 / math.sqrt(mean[2])
    # position family: Floyd's t drawn over j instead of j + 1 -- visible only given K >= 2
    for nb, p_t in ((7, 0.2), (512, 0.004)):
        good, bad = numpy_segment(SEED0 + 60, 0, 10**6, nb, p_t), numpy_segment(SEED0 + 60, 0, 10**6, nb, p_t, floyd_plus=0)
        for k in (2, 3):
            for tag, (k_err, pos) in (("sampler", good), ("Floyd mutant", bad)):
                counts, segs = position_counts(k_err, pos, nb, k)
                chi2, dof = conditioned_position_chi2(counts, segs, k)
                low, up, ok = ed.chi2_verdict(chi2, dof)
                out.append("RESOLVING positions: %s nb=%d K=%d: chi2 %.1f on %d, upper p %.2e" % (tag, nb, k, chi2, dof, up))
                assert ok == (tag == "sampler"), (tag, nb, k, chi2, dof)
        counts, segs = position_counts(*bad, nb, 1)                             # K = 1: j = nb - 1, the mutant never picks the last position
        assert counts[nb - 1] == 0 and segs > 1000
    # a sample key that ignores the top bit of i (of 2^20 samples): the second half repeats the first; every count doubles its
    # variance, which a chi-square with many degrees of freedom sees
    nb, p_t, count = 512, 0.004, 1 << 20
    for tag, mask in (("sampler", M64), ("top-bit mutant", (1 << 19) - 1)):
        k_err, pos = numpy_segment(SEED0 + 61, 0, count, nb, p_t, index_and=mask)
        per_qubit = np.bincount(pos[pos >= 0], minlength=nb)
        chi2 = float(((per_qubit - count * p_t) ** 2).sum() / (count * p_t * (1 - p_t)))
        low, up, ok = ed.chi2_verdict(chi2, nb)
        out.append("RESOLVING per-qubit: %s nb=512 N=2^20: chi2 %.1f on %d, upper p %.2e" % (tag, chi2, nb, up))
        assert ok == (tag == "sampler")
    # independence family: a key that ignores the LOW bit of i makes samples 2m and 2m + 1 equal
    k_dist = capped(binomial_pmf(nb, p_t), 6)
    for tag, mask in (("sampler", M64), ("low-bit mutant", M64 - 1)):
        k_err = np.minimum(numpy_segment(SEED0 + 62, 0, count, nb, p_t, index_and=mask)[0], 6)
        verdicts = []
        for start in (0, 1):
            a, b = k_err[start:count - 1:2], k_err[start + 1:count:2]
            pairs = min(a.size, b.size)
            verdicts.append(ed.chi2_verdict(*ed.pooled_chi2(pair_table(a[:pairs], b[:pairs], 7), np.outer(k_dist, k_dist).reshape(-1), pairs))[2])
        out.append("RESOLVING independence: %s lag-1 (K_i, K_i+1): accepted = %s" % (tag, verdicts))
        assert all(verdicts) == (tag == "sampler") and (tag == "sampler" or not verdicts[0])
    print("\n".join(out))
