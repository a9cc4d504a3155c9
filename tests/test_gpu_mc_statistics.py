"""
Is the sampler RIGHT, on the device?  The GPU leg of tests/test_mc_statistics.py: the Monte-Carlo entry points against the exact
distributions of oracle/exact_dist.py (closed forms, no sampling) at sample counts only the device reaches.  A chi-square at
N = 10^10 resolves relative deviations of about 5 / sqrt(N p_bin) per bin: 10^-4 and below.

Acceptance as on the CPU: every statistic becomes a p-value, a case fails at p < 10^-6 in either tail, seeds are fixed as
SEED0 + case index and never changed.  Run with -s to see every p-value.

Which route got which kind of test (routes as the parity tests of test_gpu_parity.py force them):
  small-code fused kernel (Steane, RM15; CSSCode.monte_carlo)   full histograms, chi-square against the exact marginals, N = 10^10,
                                                                first_sample 0 and 2^40, 8 shards summed = the whole
  GF2_MC_PIPELINE (small codes: sampler -> syndromes -> bins)   full histograms, chi-square, N = 10^8
  lane kernel, n = 127 / 255 / 511, checks of 20 rows           weight histograms (the route has no full mode), chi-square against the
                                                                weight projection of the exact marginal, N = 10^9
  GF2_MC_FUSED (sampler fused into the column gather), n = 127  the same, N = 10^9
  GF2_MC_UNFUSED (sampler -> column gather), n = 127            the same, N = 10^8
  GF2_MC_DENSE (sampler -> table kernel -> bins), n = 4096      full histograms of checks of 12 and 10 rows, chi-square, N = 10^8
  column gather at n = 4096, checks of 12 and 10 rows (default) weight histograms, chi-square against the projection, N = 10^8
  slab pipeline at n = 4096 (record sampler: default; and       needs tall checks: z-score of the mean syndrome weight against
  GF2_MC_ROWS), the configs[4] code                             syndrome_weight_mean_var, N = 10^8, p = 0.01
  table decode: gf2_mc_decode (Steane, RM15), gf2_mc_decode_    z-scores of the five counts against expected_decode_counts; at n = 47
  hashed (Steane; 47 qubits, checks cut down to 10 rows each)   r_1 + r_2 + 2 = 48 is too wide for the joint, hence the cut
  circuit kernels (gf2_circuit.hip): histograms, tally, stored  marginals and z-scores at N = 10^9 (10^8 for L = 1025), the full joint
  outcome words, four circuits                                  and lag-1 independence from 2 * 10^7 stored words
"""
import functools
import time

import numpy as np
import pytest

from oracle import cpu_ref, exact_dist as ed
from quantum_css_codes_amd import _native, bin_matrix, circuit_noise, montecarlo
from quantum_css_codes_amd.css_code import CSSCode

pytestmark = pytest.mark.gpu

SEED0 = 20261017 + 100                       # (the CPU leg holds indices 0 .. 99)
STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
RATES = [(0.01, 0.005, 0.02), (1e-3, 1e-3, 1e-3), (0.2, 0.1, 0.3), (0.01, 0.0, 0.0), (0.0, 0.01, 0.0), (0.0, 0.0, 0.01)]
FIELDS = montecarlo.DECODE_FIELDS
N_BIG = 10**10


@functools.lru_cache(maxsize=None)
def make_code(name):
    if name == "steane":
        return CSSCode(STEANE, STEANE)
    cols = np.arange(1, 16)
    h1 = np.array([(cols >> b) & 1 for b in range(4)])
    return CSSCode(h1, np.vstack([h1] + [h1[a] & h1[b] for a in range(4) for b in range(a + 1, 4)]))


@pytest.fixture
def route():
    context = _native.default_context()

    class Route(object):
        def force(self, name):
            context.set_flags(context.get_flags() | getattr(_native, "F_" + name[4:]))

        def release(self, name):
            context.set_flags(context.get_flags() & ~getattr(_native, "F_" + name[4:]))
    yield Route()
    context.set_flags(0)


@pytest.fixture(scope="module", autouse=True)
def module_time():
    start = time.time()
    yield
    print("\nMODULE-TIME test_gpu_mc_statistics.py: %.1f s" % (time.time() - start))


# ---- CSSCode.monte_carlo: the small-code kernel ---------------------------------------------------------------------------

MC_CASES = [(name, rates, first) for name in ("steane", "rm15") for rates in RATES for first in (0, 1 << 40)]


@pytest.mark.parametrize("case", range(len(MC_CASES)))
def test_monte_carlo_full_histograms(case):
    name, p, first = MC_CASES[case]
    code = make_code(name)
    got = code.monte_carlo(N_BIG, *p, seed=SEED0 + case, first_sample=first, mode='full')
    label = "monte_carlo %s p=%s first=%d N=%.0e" % (name, p, first, N_BIG)
    ed.assert_chi2(label + " hist_z", got['hist_z'], ed.marginal(code.parity_check_c1, p[1] + p[2]), N_BIG)
    ed.assert_chi2(label + " hist_x", got['hist_x'], ed.marginal(code.parity_check_c2, p[0] + p[1]), N_BIG)


@pytest.mark.parametrize("name", ["steane", "rm15"])
def test_monte_carlo_eight_shards_sum_to_the_whole(name):
    code, p, case = make_code(name), RATES[0], MC_CASES.index((name, RATES[0], 1 << 40))
    whole = code.monte_carlo(N_BIG, *p, seed=SEED0 + case, first_sample=1 << 40, mode='full')
    sum_z, sum_x = 0, 0
    for rank in range(8):
        start, mine = montecarlo.shard_range(1 << 40, N_BIG, rank, 8)
        part = code.monte_carlo(mine, *p, seed=SEED0 + case, first_sample=start, mode='full')
        sum_z, sum_x = sum_z + part['hist_z'], sum_x + part['hist_x']
    assert np.array_equal(sum_z, whole['hist_z']) and np.array_equal(sum_x, whole['hist_x'])


@pytest.mark.parametrize("name", ["steane", "rm15"])
def test_small_code_pipeline_route(name, route):
    code, p, count = make_code(name), RATES[0], 10**8
    seed = SEED0 + 30 + ("steane", "rm15").index(name)
    route.force("GF2_MC_PIPELINE")
    got = code.monte_carlo(count, *p, seed=seed, first_sample=(1 << 32) + 5, mode='full')
    route.release("GF2_MC_PIPELINE")
    ed.assert_chi2("GF2_MC_PIPELINE %s hist_z" % name, got['hist_z'], ed.marginal(code.parity_check_c1, p[1] + p[2]), count)
    ed.assert_chi2("GF2_MC_PIPELINE %s hist_x" % name, got['hist_x'], ed.marginal(code.parity_check_c2, p[0] + p[1]), count)


def test_rates_close_to_one_on_64_qubits():
    """The count table at q -> 1 on one-word segments ((1 - q)^64 underflows; see the CPU leg's test of the same name)."""
    rng = np.random.default_rng(64)
    hm1, hm2 = rng.integers(0, 2, (10, 64)), rng.integers(0, 2, (9, 64))
    count = 10**9
    for k, p in enumerate(((1 - 1e-5, 0.0, 0.0), (0.0, 1 - 1e-6, 0.0), (2e-6, 0.0, 1 - 3e-6))):
        got = run_checks(hm1, hm2, SEED0 + 35 + k, (0, (1 << 32) + 1, 1 << 40)[k], count, p, _native.HIST_FULL)
        assert_marginals("gf2_mc_run n=64 p=%s N=%.0e" % (p, count), hm1, hm2, got, p, count, False)


# ---- table decode ---------------------------------------------------------------------------------------------------------

def exact_counts(code, tables, p, count):
    joint = ed.code_capacity_joint(code, *p)
    return ed.expected_decode_counts(joint, tables[0], tables[1], (code.x_operator_matrix()[0], code.z_operator_matrix()[0]), count)


DECODE_CASES = [(name, rates, hashed) for name in ("steane", "rm15") for rates in RATES[:3] for hashed in (False,)] + \
    [("steane", RATES[0], True)]


@pytest.mark.parametrize("case", range(len(DECODE_CASES)))
def test_logical_error_rates_counts(case):
    name, p, hashed = DECODE_CASES[case]
    code, count = make_code(name), 10**9
    first = (0, (1 << 32) + 99, 1 << 40)[case % 3]
    if hashed:
        got = montecarlo.decode_local(code, count, *p, seed=SEED0 + 40 + case, first_sample=first, hashed=True)
    else:
        got = code.logical_error_rates(count, *p, seed=SEED0 + 40 + case, first_sample=first)
    assert got['samples'] == count
    mean, var = exact_counts(code, (code._c1_syndromes, code._c2_syndromes), p, count)
    for f in range(5):
        ed.assert_z("logical_error_rates %s%s p=%s %s" % (name, " hashed" if hashed else "", p, FIELDS[f]), got[FIELDS[f]], mean[f], var[f])


class CutCode(object):
    """The first rows of a code's two checks with its logical operators: what code_capacity_joint reads."""

    def __init__(self, code, rows):
        self.parity_check_c1, self.parity_check_c2 = code.parity_check_c1[:rows], code.parity_check_c2[:rows]
        self.n, self.r_1, self.r_2 = code.n, rows, rows
        self._x, self._z = code.x_operator_matrix(), code.z_operator_matrix()

    def x_operator_matrix(self):
        return self._x

    def z_operator_matrix(self):
        return self._z


def first_seen_table(check, n):
    """The zero error and every single-qubit error whose syndrome no earlier entry has (a 10-row check of 47 columns has
    colliding columns, which the reference's syndrome_table answers with the zero error alone)."""
    table = {0: np.zeros(n, dtype=int)}
    for j in range(n):
        e = np.zeros(n, dtype=int)
        e[j] = 1
        table.setdefault(int(cpu_ref.vec_to_int(cpu_ref.syndrome_product(check, e))), e)
    return table


def test_hashed_decode_of_47_qubits_with_checks_cut_to_ten_rows():
    rng = np.random.default_rng(47 + 23)
    while True:
        h1 = rng.integers(0, 2, (23, 47))
        if bin_matrix.rank(h1) == 23:
            break
    null = bin_matrix.nullspace(h1)
    full = CSSCode(h1, null[: null.shape[0] - 1], max_table_weight=1)          # k = 1: the normalised checks and the operators
    code = CutCode(full, 10)
    tables = (first_seen_table(code.parity_check_c1, 47), first_seen_table(code.parity_check_c2, 47))
    (keys1, corr1), (keys2, corr2) = (montecarlo.table_entries(t, 10, 47) for t in tables)
    two = lambda vec: np.pad(_native.pack_rows(np.asarray(vec).reshape(1, -1))[0], (0, 2))[:2]
    p, count = (0.004, 0.002, 0.006), 10**9
    got = _native.default_context().mc_decode_hashed(
        47, _native.pack_rows(code.parity_check_c1), 10, keys1, corr1, _native.pack_rows(code.parity_check_c2), 10, keys2, corr2,
        two(code.x_operator_matrix()[0]), two(code.z_operator_matrix()[0]), SEED0 + 50, (1 << 33) + 1, count, *p)
    mean, var = exact_counts(code, tables, p, count)
    for f in range(5):
        ed.assert_z("gf2_mc_decode_hashed n=47 cut to 10+10 rows p=%s %s" % (p, FIELDS[f]), int(got[f]), mean[f], var[f])


# ---- gf2_mc_run beyond 64 qubits: one case per route -----------------------------------------------------------------------

def sparse_checks(n, r1, r2, per_row, seed):
    """Checks with an identity block (H1 in front, H2 at the end) and `per_row` further ones per row: informative syndromes."""
    rng = np.random.default_rng(seed)
    hm1, hm2 = np.zeros((r1, n), dtype=int), np.zeros((r2, n), dtype=int)
    for hm, r, lo, hi in ((hm1, r1, r1, n), (hm2, r2, 0, n - r2)):
        for i in range(r):
            hm[i, rng.choice(np.arange(lo, hi), per_row, replace=False)] = 1
    hm1[:, :r1] = np.identity(r1, dtype=int)
    hm2[:, n - r2:] = np.identity(r2, dtype=int)
    return hm1, hm2


def run_checks(hm1, hm2, seed, first, count, p, mode):
    ctx = _native.default_context()
    n = hm1.shape[1]
    c1 = ctx.check_create(_native.pack_rows(hm1), hm1.shape[0], n)
    c2 = ctx.check_create(_native.pack_rows(hm2), hm2.shape[0], n)
    return ctx.mc_run(c1, c2, seed, first, count, *p, mode)


def assert_marginals(label, hm1, hm2, got, p, count, weight):
    for tag, hist, hm, q in (("hist_z", got[0], hm1, p[1] + p[2]), ("hist_x", got[1], hm2, p[0] + p[1])):
        dist = ed.marginal(hm, q)
        ed.assert_chi2("%s %s" % (label, tag), hist, ed.weight_projection(dist, hm.shape[0]) if weight else dist, count)


MID_CASES = [(127, None, 10**9), (255, None, 10**9), (511, None, 10**9), (127, "GF2_MC_FUSED", 10**9), (127, "GF2_MC_UNFUSED", 10**8)]


@pytest.mark.parametrize("case", range(len(MID_CASES)))
def test_mid_size_routes_weight_histograms(case, route):
    n, flag, count = MID_CASES[case]
    hm1, hm2 = sparse_checks(n, 20, 20, 6, n)
    p = (0.004, 0.003, 0.005)
    if flag:
        route.force(flag)
    got = run_checks(hm1, hm2, SEED0 + 60 + case, (1 << 32) + 7, count, p, _native.HIST_WEIGHT)
    if flag:
        route.release(flag)
    assert_marginals("gf2_mc_run n=%d r=20 %s N=%.0e" % (n, flag or "lane kernel", count), hm1, hm2, got, p, count, True)


@pytest.mark.parametrize("flag", ["GF2_MC_DENSE", None])
def test_n4096_short_checks(flag, route):
    hm1, hm2 = sparse_checks(4096, 12, 10, 40, 4096)
    p, count = (0.004, 0.003, 0.002), 10**8
    if flag:
        route.force(flag)
    got = run_checks(hm1, hm2, SEED0 + 70 + (1 if flag else 0), 1 << 40, count, p, _native.HIST_FULL if flag else _native.HIST_WEIGHT)
    if flag:
        route.release(flag)
    assert_marginals("gf2_mc_run n=4096 r=12/10 %s N=%.0e" % (flag or "default (column gather)", count), hm1, hm2, got, p, count, not flag)


@pytest.mark.parametrize("flag", [None, "GF2_MC_ROWS"])
def test_slab_pipeline_mean_syndrome_weight_on_the_config4_code(flag, route):
    import bench
    code, h1, h2 = bench.build_code()
    ctx = _native.default_context()
    c1, c2 = ctx.check_create(h1, bench.R1, bench.N_QUBITS), ctx.check_create(h2, bench.R2, bench.N_QUBITS)
    count, p = 10**8, bench.P_TOTAL / 3
    if flag:
        route.force(flag)
    got = ctx.mc_run(c1, c2, SEED0 + 80 + (1 if flag else 0), 5 * 10**11, count, p, p, p, _native.HIST_WEIGHT)
    if flag:
        route.release(flag)
    from oracle import c_oracle
    for tag, hist, hm in (("hist_z", got[0], c_oracle.unpack_rows(h1, bench.N_QUBITS)), ("hist_x", got[1], c_oracle.unpack_rows(h2, bench.N_QUBITS))):
        assert int(hist.sum()) == count
        mean, var = ed.syndrome_weight_mean_var(hm, 2 * p)
        total = int((hist.astype(object) * np.arange(hist.size).astype(object)).sum())
        ed.assert_z("slab pipeline (%s) config4 mean syndrome weight %s" % (flag or "record sampler", tag), total, count * mean, count * var)


# ---- circuit faults: gf2_circuit.hip -----------------------------------------------------------------------------------------

def padded_encoder(code, total):
    gates = code.encode_zero_gates()
    pad = total - len(circuit_noise.fault_locations(gates))
    idle = np.array([(2, q % code.n, 0) for q in range(pad)], dtype=np.int32).reshape(-1, 3)
    return np.concatenate((idle[:pad // 2], gates, idle[pad // 2:]))


def circuit_cases():
    steane, rm = make_code("steane"), make_code("rm15")
    return [("steane encode_zero", steane, steane.encode_zero_gates(), (0.004, 0.003, 0.005), 10**9),
            ("steane encode_plus", steane, steane.encode_plus_gates(), (0.004, 0.003, 0.005), 10**9),
            ("rm15 encode_zero", rm, rm.encode_zero_gates(), (0.0006, 0.0003, 0.0006), 10**9),
            ("steane padded L=1025", steane, padded_encoder(steane, 1025), (0.001, 0.0005, 0.0015), 10**8)]


@pytest.mark.parametrize("case", range(4))
def test_circuit_histograms_and_tallies(case):
    name, code, gates, p, count = circuit_cases()[case]
    circ = circuit_noise.circuit_for(code, gates)
    joint = ed.circuit_joint(circ.effects, *p, code.r_1, code.r_2)
    first = (0, (1 << 32) + 3, 1 << 40, 12345)[case]
    got = code.circuit_monte_carlo(gates, count, *p, seed=SEED0 + 90 + case, first_sample=first, mode='full')
    label = "circuit_monte_carlo %s L=%d N=%.0e" % (name, circ.num_locations, count)
    ed.assert_chi2(label + " hist_z", got['hist_z'], joint.hist_z(), count)
    ed.assert_chi2(label + " hist_x", got['hist_x'], joint.hist_x(), count)
    tally = code.circuit_logical_error_rates(gates, count, *p, seed=SEED0 + 94 + case, first_sample=first)
    mean, var = ed.expected_decode_counts(joint, code._c1_syndromes, code._c2_syndromes,
                                          (code.x_operator_matrix()[0], code.z_operator_matrix()[0]), count)
    for f in range(5):
        ed.assert_z("circuit_logical_error_rates %s %s" % (name, FIELDS[f]), tally[FIELDS[f]], mean[f], var[f])


@pytest.mark.parametrize("case", range(4))
def test_circuit_stored_outcomes_joint_and_lag_one(case):
    name, code, gates, p, _ = circuit_cases()[case]
    circ = circuit_noise.circuit_for(code, gates)
    count = 2 * 10**7
    words = circ.outcomes(count, *p, seed=SEED0 + 98 + case, first_sample=(1 << 40) + case)
    joint = ed.circuit_joint(circ.effects, *p, code.r_1, code.r_2)
    cells = ed.pack_outcome_words(words, code.r_1, code.r_2)
    assert np.array_equal(words[:, 0] >> np.uint64(code.r_2), np.zeros(count, dtype=np.uint64)) and not (words[:, 2] >> np.uint64(2)).any()
    ed.assert_chi2("FaultCircuit.outcomes %s joint N=%.0e" % (name, count), np.bincount(cells, minlength=joint.prob.size), joint.prob, count)
    key_z = (cells >> code.r_2) & ((1 << code.r_1) - 1)
    dist, bins = joint.hist_z(), 1 << code.r_1
    for start in (0, 1):                                                       # disjoint pairs (2m, 2m+1), then (2m+1, 2m+2)
        a, b = key_z[start:count - 1:2], key_z[start + 1:count:2]
        pairs = min(a.size, b.size)
        ed.assert_chi2("FaultCircuit.outcomes %s lag-1 (key_z_i, key_z_i+1) pairs from %d" % (name, start),
                       ed.pair_table(a[:pairs], b[:pairs], bins), np.outer(dist, dist).reshape(-1), pairs)
