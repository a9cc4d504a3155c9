"""
Weight-stratified Monte-Carlo on the GPU (DESIGN.md section 5 "Strata"): decode_strata_kernel (csrc/gf2_table.hip) and the
stratum mode of circuit_kernel (csrc/gf2_circuit.hip) through CSSCode.logical_error_strata, circuit_logical_error_strata and
encoder_logical_error_strata.

  exact     all five counts against tests/strata_ref.py (NumPy sampler, syndromes, vec_to_int keys, the code's own table dicts,
            operator parities; circuits: forward Pauli-frame propagation written here)
  zeros     Steane strata 0 and 1 never flip
  z-tests   counts against exact fractions by enumeration, binomial variance; every statistic a p-value through
            oracle/exact_dist.py, a case fails below 10^-6 in either tail; seeds 20261017 + 300 + case index
  the point rate(1e-6) and rate(1e-9) of the Steane code, where logical_error_rates returns 0 flips
"""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import exact_dist as ed
from quantum_css_codes_amd import _native, bin_matrix, circuit_noise, montecarlo
from quantum_css_codes_amd.css_code import CSSCode
from tests import strata_ref as ref

pytestmark = pytest.mark.gpu

SEED0 = 20261017 + 300
H, CNOT, IDLE = 0, 1, 2
STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
FIRST = (1 << 40) + 777
KINDS = [(1, 1, 1), (0.5, 0.2, 0.3)]
FIELDS = montecarlo.DECODE_FIELDS
N_BIG = 10**9


def dual_pair(rng, n, r1):
    """H1 (r1 x n, full rank) and all but one row of a basis of its dual: a k = 1 CSS pair."""
    while True:
        h1 = rng.integers(0, 2, (r1, n))
        if bin_matrix.rank(h1) == r1:
            break
    null = bin_matrix.nullspace(h1)
    return h1, null[: null.shape[0] - 1]


@functools.lru_cache(maxsize=None)
def make_code(name):
    if name == "steane":
        return CSSCode(STEANE, STEANE)
    if name == "rm15":
        cols = np.arange(1, 16)
        h1 = np.array([(cols >> b) & 1 for b in range(4)])
        return CSSCode(h1, np.vstack([h1] + [h1[a] & h1[b] for a in range(4) for b in range(a + 1, 4)]))
    n, r1, cap = name
    h1, h2 = dual_pair(np.random.default_rng(n + r1), n, r1)
    return CSSCode(h1, h2, max_table_weight=cap)


# ---- 1: exact against the NumPy restatement ------------------------------------------------------------------------------

# (100, 25, 3): r_2 = 74 checks, two-word keys, a table only max_table_weight makes finite
@pytest.mark.parametrize("case", enumerate(["steane", "rm15", (47, 23, None), (100, 25, 3)]), ids=lambda c: str(c[1]))
def test_strata_counts_are_the_restatement(case):
    index, name = case
    code = make_code(name)
    if name == (100, 25, 3):
        assert code.r_2 > 63 and code.r_1 <= 63
    weights, count, seed, kinds = list(range(min(code.n, 8) + 1)), 1 << 16, SEED0 + index, KINDS[index % 2]
    got = code.logical_error_strata(weights, count, kinds=kinds, seed=seed, first_sample=FIRST)
    want = ref.strata_counts(code, weights, count, kinds, seed, FIRST)
    for s, w in enumerate(weights):
        print("STRATA %s w=%d counts %s" % (name, w, got.counts[s].tolist()))
    assert np.array_equal(got.counts, want)
    assert got.nb == code.n and list(got.weights) == weights and list(got.samples) == [count] * len(weights)
    assert not got.counts[0].any()
    # eight shards of every stratum sum to the whole (sample ranges of their own, uneven counts)
    samples = [count - 13 * s for s in range(len(weights))]
    whole = code.logical_error_strata(weights, samples, kinds=kinds, seed=seed, first_sample=FIRST)
    total = np.zeros_like(whole.counts)
    for rank in range(8):
        shards = [montecarlo.shard_range(FIRST, c, rank, 8) for c in samples]
        total += code.logical_error_strata(weights, [c for _, c in shards], kinds=kinds, seed=seed, first_sample=[f for f, _ in shards]).counts
    assert np.array_equal(total, whole.counts)
    assert np.array_equal(whole.counts, ref.strata_counts(code, weights, samples, kinds, seed, FIRST))
    # and strata_sharded without a process group is strata_local
    alone = montecarlo.strata_sharded(code, weights, samples, kinds=kinds, seed=seed, first_sample=FIRST)
    assert np.array_equal(alone.counts, whole.counts)


# ---- 2: exact zeros --------------------------------------------------------------------------------------------------------

def test_steane_strata_0_and_1_never_flip():
    got = make_code("steane").logical_error_strata([0, 1], 10**8, seed=SEED0 + 10)
    assert got.counts.shape == (2, 5) and not got.counts.any()
    assert got.rate(1e-3) == (0.0, 0.0, got.rate(1e-3).truncation) and got.rate(1e-3).truncation > 2e-5


# ---- 3: distribution -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def steane_run(kind_index):
    """Strata 0 .. 7 of the Steane code: 10^9 samples each from weight 2 on."""
    samples = [10**6, 10**8] + [N_BIG] * 6
    return make_code("steane").logical_error_strata(range(8), samples, kinds=KINDS[kind_index], seed=SEED0 + 20 + kind_index,
                                                    first_sample=FIRST)


@functools.lru_cache(maxsize=None)
def steane_fails():
    return ref.steane_failures(make_code("steane"))                  # (any, x, z): (#X, #Y, #Z) of every failing error


def exact_fraction(fails, w, q):
    """P(flip | weight w) with kind probabilities q: a uniform w-subset, i.i.d. kinds."""
    return sum(q[0]**a * q[1]**b * q[2]**c for a, b, c in fails if a + b + c == w) / math.comb(7, w)


@pytest.mark.parametrize("kind_index", (0, 1))
def test_steane_strata_follow_the_exact_fractions(kind_index):
    got = steane_run(kind_index)
    q = ref.kind_probabilities(KINDS[kind_index])
    f_any, f_x, f_z = steane_fails()
    assert not got.counts[:2].any() and not got.counts[:, 3:].any()          # the Steane tables hold every syndrome
    for w in range(2, 8):
        for name, fails in (('logical_x', f_x), ('logical_z', f_z), ('logical_any', f_any)):
            f = exact_fraction(fails, w, q)
            ed.assert_z("steane stratum %d %s kinds %s" % (w, name, KINDS[kind_index]), int(got.counts[w, FIELDS.index(name)]),
                        N_BIG * f, N_BIG * f * (1 - f))


def side_fractions(check, table, op, n):
    """Per number m of erroneous qubits of ONE component: the fractions of the C(n, m) patterns that end in a logical flip and
    that have no table entry, by enumeration of all 2^n patterns."""
    patterns = ((np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1).astype(np.uint8)
    op = np.asarray(op).astype(np.int64) & 1
    of_entry = {int(key): int(np.dot(op, np.asarray(corr).astype(np.int64))) & 1 for key, corr in table.items()}
    found = [of_entry.get(key) for key in ref.keys_of(check, patterns)]
    miss = np.array([f is None for f in found])
    flip = ((patterns.astype(np.int64) @ op) & 1) ^ np.array([f or 0 for f in found])
    m = patterns.sum(axis=1)
    total = np.bincount(m, minlength=n + 1)
    return np.bincount(m, weights=flip, minlength=n + 1) / total, np.bincount(m, weights=miss, minlength=n + 1) / total


def test_rm15_strata_follow_the_exact_per_side_fractions():
    """A stratum of weight w has Bin(w, q_x + q_y) qubits with an X component, a uniform subset given their number (and
    likewise Z with q_y + q_z): the per-side counts are mixtures of the per-weight fractions of the 2^15 patterns of a side."""
    code, kinds, count = make_code("rm15"), KINDS[1], 10**8
    weights = [1, 2, 3, 4, 5, 6]
    got = code.logical_error_strata(weights, count, kinds=kinds, seed=SEED0 + 30, first_sample=FIRST)
    q = ref.kind_probabilities(kinds)
    sides = (("x", q[0] + q[1], side_fractions(code.parity_check_c2, code._c2_syndromes, code.z_operator_matrix()[0], 15)),
             ("z", q[1] + q[2], side_fractions(code.parity_check_c1, code._c1_syndromes, code.x_operator_matrix()[0], 15)))
    for s, w in enumerate(weights):
        for tag, q_side, (flip, miss) in sides:
            mix = [math.comb(w, m) * q_side**m * (1 - q_side)**(w - m) for m in range(w + 1)]
            for name, frac in (("logical_" + tag, flip), ("uncorrectable_" + tag, miss)):
                f = sum(b * frac[m] for m, b in enumerate(mix))
                ed.assert_z("rm15 stratum %d %s" % (w, name), int(got.counts[s, FIELDS.index(name)]), count * f, count * f * (1 - f))


# ---- 4: the point of the feature ---------------------------------------------------------------------------------------------

def test_rates_below_the_quantisation_floor():
    got = steane_run(0)
    f_any = steane_fails()[0]
    for p, quoted in ((1e-6, 1.633328e-11), (1e-9, None)):
        each, rest = Fraction(p) / 3, 1 - Fraction(p)
        exact = float(sum(each ** sum(f) * rest ** (7 - sum(f)) for f in f_any))
        rate = got.rate(p)
        print("STRATA steane rate(%g) = %.6e +- %.2e (exact %.6e, truncation %g)" % (p, rate.estimate, rate.stderr, exact, rate.truncation))
        assert quoted is None or abs(exact / quoted - 1) < 1e-6
        assert rate.truncation == 0.0 and 0 < rate.stderr < 1e-4 * rate.estimate
        assert abs(rate.estimate - exact) <= 5 * rate.stderr
    # the direct sampler at the same rate, side by side: unchanged, and blind
    direct = make_code("steane").logical_error_rates(10**8, 1e-6 / 3, 1e-6 / 3, 1e-6 / 3, seed=SEED0 + 40)
    assert direct['logical_any'] == 0 and direct['logical_x'] == 0 and direct['logical_z'] == 0 and direct['samples'] == 10**8


# ---- 5: circuits -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", enumerate(["steane", (47, 23, None)]), ids=lambda c: str(c[1]))
def test_idle_circuit_strata_are_the_code_capacity_strata(case):
    index, name = case
    code = make_code(name)
    weights, samples = list(range(9 if code.n > 8 else 8)), [10**6 - 7 * s for s in range(9)][:9 if code.n > 8 else 8]
    idle = np.array([(IDLE, q, 0) for q in range(code.n)], dtype=np.int32)
    for kinds in KINDS:
        want = code.logical_error_strata(weights, samples, kinds=kinds, seed=SEED0 + 50 + index, first_sample=FIRST)
        got = code.circuit_logical_error_strata(idle, weights, samples, kinds=kinds, seed=SEED0 + 50 + index, first_sample=FIRST)
        assert np.array_equal(got.counts, want.counts) and got.nb == code.n
        # (no error, no flip; a random pair need not correct every single error -- the Steane code does)
        assert want.counts[-1, 2] > 0 and not want.counts[0].any() and (code.n != 7 or not want.counts[1].any())


def propagate(gates, n, f_x, f_z):
    """Final frames (n x count each): every gate acts, then its locations' faults (L x count) are XOR-ed in."""
    count = f_x.shape[1]
    e_x, e_z, loc = np.zeros((n, count), dtype=np.uint8), np.zeros((n, count), dtype=np.uint8), 0
    for kind, a, b in gates.tolist():
        if kind == H:
            e_x[a], e_z[a] = e_z[a].copy(), e_x[a].copy()
        elif kind == CNOT:
            e_x[b] ^= e_x[a]
            e_z[a] ^= e_z[b]
        for q in ((a, b) if kind == CNOT else (a,)):
            e_x[q] ^= f_x[loc]
            e_z[q] ^= f_z[loc]
            loc += 1
    assert loc == f_x.shape[0]
    return e_x, e_z


def circuit_strata_restated(code, gates, weights, count, kinds, seed, first):
    total = len(circuit_noise.fault_locations(gates))
    out = np.zeros((len(weights), 5), dtype=np.uint64)
    for s, w in enumerate(weights):
        f_x, f_z = ref.stratum_bits(seed, first, count, total, w, kinds)
        e_x, e_z = propagate(gates, code.n, np.ascontiguousarray(f_x.T), np.ascontiguousarray(f_z.T))
        out[s] = ref.decode_counts(code, np.ascontiguousarray(e_x.T), np.ascontiguousarray(e_z.T))
    return out


@pytest.mark.parametrize("case", enumerate([("steane", "zero"), ("steane", "plus"), ("rm15", "zero")]), ids=lambda c: "%s-%s" % c[1])
def test_encoder_strata_against_forward_propagation(case):
    index, (name, state) = case
    code = make_code(name)
    gates = np.asarray(circuit_noise.encoder_gates(code, state), dtype=np.int32)
    weights, count, kinds, seed = [0, 1, 2, 3, 4], 1 << 14, KINDS[index % 2], SEED0 + 60 + index
    got = code.encoder_logical_error_strata(state, weights, count, kinds=kinds, seed=seed, first_sample=FIRST)
    want = circuit_strata_restated(code, gates, weights, count, kinds, seed, FIRST)
    print("STRATA encoder %s %s L=%d counts %s" % (name, state, got.nb, got.counts.tolist()))
    assert np.array_equal(got.counts, want)
    assert got.nb == len(circuit_noise.fault_locations(gates)) and not got.counts[0].any()


def test_one_segment_of_1025_locations_and_sixteen_picks():
    """L = 1025 (no 512-location segments here: one segment over all of L, the effects read through L2) and every weight up to
    the 16 picks the register list holds."""
    code = make_code("steane")
    rng = np.random.default_rng(5)
    rows = []
    for g in range(525):                                                     # 500 CNOTs (two locations each) among 25 IDLEs
        a, b = rng.choice(7, 2, replace=False)
        rows.append((IDLE, a, 0) if g % 21 == 0 else (CNOT, a, b))
    gates = np.array(rows, dtype=np.int32)
    assert len(circuit_noise.fault_locations(gates)) == 1025
    weights, count, seed = list(range(17)), 1 << 13, SEED0 + 70
    got = code.circuit_logical_error_strata(gates, weights, count, kinds=KINDS[1], seed=seed, first_sample=FIRST)
    assert np.array_equal(got.counts, circuit_strata_restated(code, gates, weights, count, KINDS[1], seed, FIRST))
    assert got.nb == 1025 and got.counts[1:, 2].all()


def test_one_fault_in_the_steane_encoder_can_flip_the_logical_qubit():
    """f_1 of encode_zero, exact by enumeration of the 3 L single faults through the effect table; the encoder is not fault
    tolerant (f_1 > 0) where the code itself corrects every single error (f_1 = 0)."""
    code, kinds, count = make_code("steane"), KINDS[1], 10**8
    circ = circuit_noise.circuit_for(code, circuit_noise.encoder_gates(code, 'zero'))
    total, q = circ.num_locations, ref.kind_probabilities(kinds)
    z_op, x_op = np.asarray(code.z_operator_matrix()[0]), np.asarray(code.x_operator_matrix()[0])
    of_x = {int(k): int(np.dot(z_op, v)) & 1 for k, v in code._c2_syndromes.items()}
    of_z = {int(k): int(np.dot(x_op, v)) & 1 for k, v in code._c1_syndromes.items()}
    exact = np.zeros(3)
    for l in range(total):
        for kind, words in enumerate((circ.effects[l, 0], circ.effects[l, 0] ^ circ.effects[l, 1], circ.effects[l, 1])):
            key_x, key_z, parity = (int(v) for v in words)
            flip_x, flip_z = (parity & 1) ^ of_x[key_x], ((parity >> 1) & 1) ^ of_z[key_z]           # (every Steane syndrome has its entry)
            exact += q[kind] / total * np.array([flip_x, flip_z, flip_x | flip_z])
    got = code.encoder_logical_error_strata('zero', [1], count, kinds=kinds, seed=SEED0 + 80, first_sample=FIRST)
    for k, name in enumerate(FIELDS[:3]):
        print("STRATA steane encode_zero f_1 %s exact %.6f measured %.6f" % (name, exact[k], int(got.counts[0, k]) / count))
        ed.assert_z("steane encode_zero one fault " + name, int(got.counts[0, k]), count * exact[k], count * exact[k] * (1 - exact[k]))
    assert exact[2] > 0 and got.counts[0, 2] > 0 and not got.counts[0, 3:].any()
    assert not code.logical_error_strata([1], count, kinds=kinds, seed=SEED0 + 80, first_sample=FIRST).counts.any()
    assert got.rate(1e-6).estimate > 1e-7                                                           # first order in p, not second


def test_refused_strata():
    code = make_code("steane")
    circ = circuit_noise.circuit_for(code, circuit_noise.encoder_gates(code, 'zero'))             # L = 21
    short = circuit_noise.circuit_for(code, np.array([(IDLE, q, 0) for q in range(7)], dtype=np.int32))
    ctx = _native.default_context()
    keys1, flips1, keys2, flips2 = circ._tables()
    for circuit, w, text in ((circ, 17, "outside"), (short, 8, "outside"), (circ, -1, "outside")):
        with pytest.raises(_native.GF2Error, match=text) as err:
            ctx.mc_circuit_decode_strata(circuit.device(), 3, keys1, flips1, 3, keys2, flips2, 1, 0, [w], [10], 1.0, 1.0, 1.0)
        assert err.value.code == _native.GF2_E_ARG
        with pytest.raises(ValueError):
            circuit.logical_error_strata([w], 10)
    for counts, kinds, text in (([-1], (1, 1, 1), "negative"), ([10], (0, 0, 0), "kind weights"), ([10], (1, -1, 1), "kind weights")):
        with pytest.raises(_native.GF2Error, match=text):
            ctx.mc_circuit_decode_strata(circ.device(), 3, keys1, flips1, 3, keys2, flips2, 1, 0, [1], counts, *kinds)
    two = lambda vec: np.pad(_native.pack_rows(np.asarray(vec).reshape(1, -1))[0], (0, 2))[:2]
    (k1, c1), (k2, c2) = (montecarlo.table_entries(t, 3, 7) for t in (code._c1_syndromes, code._c2_syndromes))
    args = (7, _native.pack_rows(code.parity_check_c1), 3, k1, c1, _native.pack_rows(code.parity_check_c2), 3, k2, c2,
            two(code.x_operator_matrix()[0]), two(code.z_operator_matrix()[0]), 1, 0)
    for weights, counts, kinds, text in (([8], [10], (1, 1, 1), "outside"), ([-1], [10], (1, 1, 1), "outside"), ([1], [-1], (1, 1, 1), "negative"),
                                         ([1], [10], (0, 0, 0), "kind weights")):
        with pytest.raises(_native.GF2Error, match=text) as err:
            ctx.mc_decode_strata(*args, weights, counts, *kinds)
        assert err.value.code == _native.GF2_E_ARG
    with pytest.raises(_native.GF2Error, match="nstrata"):
        ctx.mc_decode_strata(*args, [1] * 257, [1] * 257, 1.0, 1.0, 1.0)
    assert ctx.mc_decode_strata(*args, [], [], 1.0, 1.0, 1.0).shape == (0, 5)
    assert not ctx.mc_decode_strata(*args, [2, 3], [0, 0], 1.0, 1.0, 1.0).any()
