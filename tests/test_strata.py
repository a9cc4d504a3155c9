"""
Weight-stratified Monte-Carlo on the CPU (DESIGN.md section 5 "Strata"): the host statement of the definition
(gf2_stratum_errors, csrc/gf2_host.cpp) against the NumPy restatement of tests/strata_ref.py bit for bit, its distribution by
the project's convention (every statistic a p-value through oracle/exact_dist.py, a case fails below 10^-6 in either tail, seeds
20261017 + 200 + case index: the legs before this one hold the indices below 200), a mutant that must be rejected, the estimator
against exact rationals, the sharding under gloo and the argument errors.
"""
import math
import os
import socket
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch.multiprocessing as mp

from oracle import cpu_ref, exact_dist as ed
from quantum_css_codes_amd import _native, montecarlo
from tests import strata_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED0 = 20261017 + 200
STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
FIRSTS = [0, (1 << 32) + 12345, (1 << 40) + 777]
KINDS = [(1, 1, 1), (0.5, 0.2, 0.3), (2, 0, 5)]
NBS = (1, 7, 64, 65, 128, 513, 1030)


def weights_of(nb):
    ws = {0, 1, 2, 3, min(nb, 16)} | ({nb} if nb <= 128 else set())
    return sorted(w for w in ws if w <= nb)


# ---- 1, 2: the two statements agree bit for bit; every sample has w distinct positions -----------------------------------

@pytest.mark.parametrize("nb", NBS)
def test_host_statement_is_the_numpy_restatement(nb):
    count = 257
    for w in weights_of(nb):
        for first in FIRSTS:
            for case, kinds in enumerate(KINDS):
                seed = SEED0 + case
                ex, ez = _native.stratum_errors(nb, w, count, kinds, seed=seed, first=first)
                assert ex.shape == ez.shape == (count, (nb + 63) // 64)
                want_x, want_z = ref.stratum_bits(seed, first, count, nb, w, kinds)
                assert np.array_equal(ex, ref.pack(want_x)) and np.array_equal(ez, ref.pack(want_z)), (nb, w, first, kinds)
                hit = ref.unpack(ex | ez, nb)
                assert np.all(hit.sum(axis=1) == w)                               # exactly w distinct positions, pad bits zero
                assert np.all(ref.unpack(ex | ez, ex.shape[1] * 64).sum(axis=1) == w)
                pos, _ = ref.stratum_draws(seed, first, count, nb, w, kinds)
                assert np.all((pos >= 0) & (pos < nb)) and all(len(set(row)) == w for row in pos.tolist())
                if kinds[1] == 0:                                                 # no Y: never both components on one position
                    assert not np.any(ref.unpack(ex & ez, nb))


def test_a_shifted_range_is_the_same_stream():
    ex, ez = _native.stratum_errors(65, 3, 100, seed=SEED0 + 3, first=FIRSTS[2])
    ex2, ez2 = _native.stratum_errors(65, 3, 40, seed=SEED0 + 3, first=FIRSTS[2] + 60)
    assert np.array_equal(ex[60:], ex2) and np.array_equal(ez[60:], ez2)
    assert _native.stratum_errors(65, 3, 0)[0].shape == (0, 2)


# ---- 3: distribution of the host statement ------------------------------------------------------------------------------

N_DIST = 10**6


def subset_position_chi2(counts, samples, k):
    """Per-position counts of `samples` uniform k-subsets of nb positions: mean M k / nb, variance M p (1 - p), covariance
    -M p (1 - p) / (nb - 1), so sum (c - M p)^2 / (M p (1 - p)) (nb - 1) / nb is a chi-square on nb - 1 degrees of freedom."""
    nb = counts.size
    p = k / nb
    return float(((counts - samples * p) ** 2).sum() / (samples * p * (1 - p)) * (nb - 1) / nb), nb - 1


def host_statistics(nb, w, kinds, seed, first, count, chunk=100000):
    """Per-position counts and the (X, Y, Z) counts of `count` samples of the host statement."""
    per_pos, per_kind = np.zeros(nb, dtype=np.int64), np.zeros(3, dtype=np.int64)
    for done in range(0, count, chunk):
        now = min(chunk, count - done)
        ex, ez = _native.stratum_errors(nb, w, now, kinds, seed=seed, first=first + done)
        x, z = ref.unpack(ex, nb), ref.unpack(ez, nb)
        per_pos += (x | z).sum(axis=0, dtype=np.int64)
        per_kind += np.array([(x & ~z & 1).sum(), (x & z).sum(), (z & ~x & 1).sum()], dtype=np.int64)
    return per_pos, per_kind


POSITION_CASES = [(nb, w) for nb in (7, 512, 1030) for w in (1, 2, 3)]


@pytest.mark.parametrize("case", range(len(POSITION_CASES)))
def test_positions_are_a_uniform_subset_and_kinds_follow_the_thresholds(case):
    nb, w = POSITION_CASES[case]
    kinds = KINDS[case % 3]
    per_pos, per_kind = host_statistics(nb, w, kinds, SEED0 + 10 + case, FIRSTS[case % 3], N_DIST)
    assert int(per_pos.sum()) == w * N_DIST == int(per_kind.sum())
    ed.assert_chi2_stat("strata positions nb=%d w=%d" % (nb, w), *subset_position_chi2(per_pos, N_DIST, w))
    ed.assert_chi2("strata kinds nb=%d w=%d kinds=%s" % (nb, w, kinds), per_kind, ref.kind_probabilities(kinds), w * N_DIST)
    if kinds[1] == 0:
        assert per_kind[1] == 0


def lowest_position_pmf(nb, w):
    """P(min of a uniform w-subset of nb positions = m), padded to nb entries."""
    return np.array([math.comb(nb - 1 - m, w - 1) / math.comb(nb, w) if nb - 1 - m >= w - 1 else 0.0 for m in range(nb)])


@pytest.mark.parametrize("w", (1, 2))
def test_neighbouring_strata_of_one_seed_are_independent(w):
    """Sample i of stratum w and sample i of stratum w + 1 share (seed, i) and differ in the segment slot alone.  Projection:
    the lowest position of each, on 7 positions; the pair table against the product of the two exact marginals."""
    nb, seed = 7, SEED0 + 30 + w
    low = []
    for weight in (w, w + 1):
        ex, ez = _native.stratum_errors(nb, weight, N_DIST, seed=seed, first=FIRSTS[1])
        low.append(np.argmax(ref.unpack(ex | ez, nb), axis=1))
    prob = np.outer(lowest_position_pmf(nb, w), lowest_position_pmf(nb, w + 1)).reshape(-1)
    ed.assert_chi2("strata %d and %d of one seed, lowest positions" % (w, w + 1), ed.pair_table(low[0], low[1], nb), prob, N_DIST)
    # (and the projection can see dependence: a stratum against itself is rejected)
    same = np.outer(lowest_position_pmf(nb, w), lowest_position_pmf(nb, w)).reshape(-1)
    assert not ed.chi2_verdict(*ed.pooled_chi2(ed.pair_table(low[0], low[0], nb), same, N_DIST))[2]


# ---- 4: the tests can fail -------------------------------------------------------------------------------------------------

def test_floyd_mutant_is_rejected():
    """Floyd's t drawn over j instead of j + 1: the last position is only ever reached through a collision."""
    for nb in (7, 512):
        for w in (2, 3):
            for tag, plus in (("definition", 1), ("Floyd mutant", 0)):
                pos, _ = ref.stratum_draws(SEED0 + 40, 0, N_DIST, nb, w, floyd_plus=plus)
                chi2, dof = subset_position_chi2(np.bincount(pos.reshape(-1), minlength=nb), N_DIST, w)
                low, up, ok = ed.chi2_verdict(chi2, dof)
                print("RESOLVING strata positions: %s nb=%d w=%d: chi2 %.1f on %d, upper p %.2e" % (tag, nb, w, chi2, dof, up))
                assert ok == (tag == "definition"), (tag, nb, w, chi2, dof)
        pos, _ = ref.stratum_draws(SEED0 + 40, 0, 10000, nb, 1, floyd_plus=0)
        assert not np.any(pos == nb - 1)


# ---- 5, 6: the estimator ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def steane_exact():
    """Exact f_w of the Steane code with uniform kinds as a Strata (N_w = C(7, w) 3^w errors, all of them), and the failing
    errors' (#X, #Y, #Z)."""
    code = cpu_ref.CSSCode(STEANE, STEANE)
    fails = ref.steane_failures(code)[0]
    per_weight = np.bincount([sum(f) for f in fails], minlength=8)
    counts = np.zeros((8, 5), dtype=np.uint64)
    counts[:, 2] = per_weight
    return montecarlo.Strata(7, range(8), [math.comb(7, w) * 3**w for w in range(8)], counts), fails, per_weight


def exact_rate(fails, p):
    each, rest = Fraction(p) / 3, 1 - Fraction(p)
    return sum(each ** sum(f) * rest ** (7 - sum(f)) for f in fails)


def test_steane_fractions_are_the_issue_figures(steane_exact):
    strata, _, per_weight = steane_exact
    assert per_weight[0] == 0 and per_weight[1] == 0
    assert Fraction(int(per_weight[2]), math.comb(7, 2) * 9) == Fraction(7, 9)
    assert np.allclose(strata.fractions(), [0, 0, 0.7778, 0.7333, 0.7852, 0.7490, 0.7202, 0.7888], atol=5e-5)


@pytest.mark.parametrize("p", (1e-3, 1e-4, 1e-5, 1e-6, 1e-9, 1e-12))
def test_rate_is_the_exact_rational(steane_exact, p):
    strata, fails, _ = steane_exact
    exact = exact_rate(fails, p)
    got = strata.rate(p)
    print("STRATA rate(%g) = %.15e exact %.15e truncation %.3e" % (p, got.estimate, float(exact), got.truncation))
    assert abs(Fraction(got.estimate) - exact) <= Fraction(1, 10**12) * exact
    assert got.truncation == 0.0 and got.stderr >= 0.0
    est, err, trunc = strata.curve([p, 2 * p])
    assert est[0] == got.estimate and err[0] == got.stderr and trunc[0] == 0.0 and est[1] > est[0]


def test_the_rates_design_md_quotes(steane_exact):
    strata = steane_exact[0]
    for p, want in ((1e-3, 1.627742e-5), (1e-4, 1.632773e-7), (1e-5, 1.633277e-9), (1e-6, 1.633328e-11), (1e-12, 1.633333e-23)):
        assert abs(strata.rate(p).estimate / want - 1) < 1e-6


def test_binomial_weights_sum_to_one_and_hold_at_tiny_rates():
    for nb in (1, 7, 128, 5000):
        for p in (0.0, 1e-12, 1e-6, 0.01, 0.5, 0.99, 1.0):
            b = montecarlo.binomial_weights(nb, p)
            assert b.shape == (nb + 1,) and abs(math.fsum(b) - 1.0) < 1e-9
    b = montecarlo.binomial_weights(128, 1e-12)
    for w in (0, 1, 2, 5):
        exact = math.comb(128, w) * Fraction(1e-12) ** w * (1 - Fraction(1e-12)) ** (128 - w)
        assert abs(Fraction(float(b[w])) - exact) <= Fraction(1, 10**12) * exact
    with pytest.raises(ValueError):
        montecarlo.binomial_weights(7, 1.5)


@pytest.mark.parametrize("p", (1e-2, 1e-3, 1e-6, 1e-9))
def test_truncation_is_the_unsampled_mass_and_an_upper_bound(steane_exact, p):
    whole, fails, _ = steane_exact
    part = montecarlo.Strata(7, whole.weights[:3], whole.samples[:3], whole.counts[:3])
    got = part.rate(p)
    fp = Fraction(p)
    tail = sum(math.comb(7, w) * fp**w * (1 - fp)**(7 - w) for w in range(3, 8))
    assert abs(Fraction(got.truncation) - tail) <= Fraction(1, 10**12) * tail
    exact = exact_rate(fails, p)
    assert Fraction(got.estimate) <= exact <= Fraction(got.estimate) + Fraction(got.truncation)
    # a stratum without samples is not sampled: its mass goes to the truncation
    empty = montecarlo.Strata(7, [0, 1, 2, 3], [1, 1, 567, 0], [[0] * 5, [0] * 5, [0, 0, 441, 0, 0], [0] * 5])
    assert abs(empty.rate(p).truncation - got.truncation) <= 1e-15 * got.truncation
    assert abs(empty.rate(p).estimate - got.estimate) <= 1e-15 * got.estimate


def test_standard_error_formula():
    strata = montecarlo.Strata(7, [2, 3], [1000, 4000], [[0, 0, 780, 0, 0], [0, 0, 2900, 0, 0]])
    b = montecarlo.binomial_weights(7, 0.01)
    f2, f3 = 0.78, 0.725
    got = strata.rate(0.01)
    assert math.isclose(got.estimate, b[2] * f2 + b[3] * f3, rel_tol=1e-14)
    assert math.isclose(got.stderr, math.sqrt(b[2]**2 * f2 * (1 - f2) / 1000 + b[3]**2 * f3 * (1 - f3) / 4000), rel_tol=1e-14)
    assert strata.rate(0.01, 'logical_x').estimate == 0.0
    with pytest.raises(ValueError):
        montecarlo.Strata(7, [2, 2], [1, 1], np.zeros((2, 5)))
    with pytest.raises(ValueError):
        montecarlo.Strata(7, [8], [1], np.zeros((1, 5)))


# ---- 7: sharding ------------------------------------------------------------------------------------------------------------

SHARD_WEIGHTS, SHARD_SAMPLES = [0, 1, 2, 3, 7], [100, 3001, 1000, 777, 5]


def _host_strata_local(code, weights, samples, kinds=(1, 1, 1), seed=0, first_sample=0):
    """strata_local's signature on the CPU: errors from the host statement, the decode from tests/strata_ref.py."""
    from quantum_css_codes_amd import _native, montecarlo
    from tests import strata_ref
    samples = np.broadcast_to(np.asarray(samples, dtype=np.int64), (len(weights),))
    firsts = np.broadcast_to(np.asarray(first_sample, dtype=np.int64), (len(weights),))
    counts = np.zeros((len(weights), 5), dtype=np.uint64)
    for s, w in enumerate(weights):
        ex, ez = _native.stratum_errors(code.n, w, int(samples[s]), kinds, seed=seed, first=int(firsts[s]))
        counts[s] = strata_ref.decode_counts(code, strata_ref.unpack(ex, code.n), strata_ref.unpack(ez, code.n))
    return montecarlo.Strata(code.n, weights, samples, counts, kinds)


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from oracle import cpu_ref
    from quantum_css_codes_amd import montecarlo
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    res = montecarlo.strata_sharded(cpu_ref.CSSCode(STEANE, STEANE), SHARD_WEIGHTS, SHARD_SAMPLES, kinds=(0.5, 0.2, 0.3), seed=SEED0 + 50,
                                    first_sample=FIRSTS[2], local_fn=_host_strata_local)
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), counts=res.counts, samples=res.samples, weights=res.weights)
    dist.destroy_process_group()


@pytest.mark.parametrize("world", (2, 8))
def test_strata_sharded_gives_the_counts_of_one_rank(tmp_path, world):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    code = cpu_ref.CSSCode(STEANE, STEANE)
    whole = _host_strata_local(code, SHARD_WEIGHTS, SHARD_SAMPLES, kinds=(0.5, 0.2, 0.3), seed=SEED0 + 50, first_sample=FIRSTS[2])
    assert np.array_equal(whole.counts, ref.strata_counts(code, SHARD_WEIGHTS, SHARD_SAMPLES, (0.5, 0.2, 0.3), SEED0 + 50, FIRSTS[2]))
    assert whole.counts[:2].sum() == 0 and whole.counts[2:, 2].all()               # weights 0 and 1 never flip, the others do
    for rank in range(world):
        r = np.load(tmp_path / ("rank%d.npz" % rank))
        assert np.array_equal(r["counts"], whole.counts) and list(r["samples"]) == SHARD_SAMPLES and list(r["weights"]) == SHARD_WEIGHTS
    # without a process group: the one shard is the whole
    alone = montecarlo.strata_sharded(code, SHARD_WEIGHTS, SHARD_SAMPLES, kinds=(0.5, 0.2, 0.3), seed=SEED0 + 50, first_sample=FIRSTS[2],
                                      local_fn=_host_strata_local)
    assert np.array_equal(alone.counts, whole.counts)


# ---- 8: argument errors -----------------------------------------------------------------------------------------------------

def test_argument_errors():
    for args, text in (((7, 8, 10), "outside"), ((7, -1, 10), "outside"), ((0, 0, 10), "positions"), (((1 << 20) + 1, 0, 10), "positions"),
                       ((7, 2, -1), "negative range")):
        with pytest.raises(_native.GF2Error, match=text) as err:
            _native.stratum_errors(*args)
        assert err.value.code == _native.GF2_E_ARG
    for kinds in ((0, 0, 0), (1, -1, 1), (float("nan"), 1, 1), (float("inf"), 1, 1)):
        with pytest.raises(_native.GF2Error, match="kind weights") as err:
            _native.stratum_errors(7, 2, 10, kinds)
        assert err.value.code == _native.GF2_E_ARG
    with pytest.raises(_native.GF2Error, match="negative range"):
        _native.stratum_errors(7, 2, 10, first=-1)
    ex = np.zeros((4, 1), dtype="<u8")
    assert _native.lib().gf2_stratum_errors(65, 1, 0, 0, 4, 1.0, 1.0, 1.0, ex.ctypes.data, ex.ctypes.data, 1) == _native.GF2_E_ARG   # lde too small
    assert _native.lib().gf2_stratum_errors(7, 1, 0, 0, 4, 1.0, 1.0, 1.0, None, None, 1) == _native.GF2_E_ARG
    assert b"null" in _native.lib().gf2_last_error()
    # the Python layer refuses before it touches a device
    code = cpu_ref.CSSCode(STEANE, STEANE)
    for call in (lambda: montecarlo.strata_local(code, [8], 10), lambda: montecarlo.strata_local(code, [-1], 10),
                 lambda: montecarlo.strata_local(code, [1], -5), lambda: montecarlo.strata_local(code, [1], 10, kinds=(0, 0, 0)),
                 lambda: montecarlo.strata_local(code, [1], 10, kinds=(1, -1, 1)), lambda: montecarlo.strata_local(code, [1, 2], [10]*3)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        steane = montecarlo.Strata(7, [2], [10], np.zeros((1, 5)))
        steane.rate(-0.1)
