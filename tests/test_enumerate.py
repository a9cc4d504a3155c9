"""
Exact strata on the CPU (DESIGN.md section 5 "Exact strata"): gf2_subset_unrank and gf2_circuit_enumerate_host
(csrc/gf2_host.cpp), FaultCircuit.enumerate_strata(host=True), montecarlo.ExactStrata / MergedStrata / enumerate_sharded.

  unrank      ranks 0 .. C(nb, w) - 1 are the combinations in colexicographic order; Python integers at nb = 2^20; refusals
  restated    the host statement against tests/enumerate_ref.py, count for count, per composition [n_x][n_y][field]
  truth       counts that share no code with the effect table: the 4^7 errors of the Steane code through oracle.cpu_ref, and
              every single fault of the Steane encoders by forward frame propagation
  additive    three unequal rank ranges sum to the whole
  arithmetic  ExactStrata.rate against the exact rational, truncation, merged, leading_order
  sharding    enumerate_sharded over gloo worlds of 2 and 8 ranks
"""
import itertools
import math
import os
import socket
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch.multiprocessing as mp

from oracle import cpu_ref
from quantum_css_codes_amd import _native, circuit_noise, montecarlo
from tests import enumerate_ref as eref
from tests import strata_ref as sref
from tests.test_circuit_effects import propagate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, CNOT, IDLE = 0, 1, 2
STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
FIELDS = montecarlo.DECODE_FIELDS


def rm15_checks():
    cols = np.arange(1, 16)
    h1 = np.array([(cols >> b) & 1 for b in range(4)])
    return h1, np.vstack([h1] + [h1[a] & h1[b] for a in range(4) for b in range(a + 1, 4)])


def long_gates():
    """The 1025-location circuit of tests/test_gpu_strata.py: 500 CNOTs (two locations each) among 25 IDLEs on 7 qubits."""
    rng = np.random.default_rng(5)
    rows = []
    for g in range(525):
        a, b = rng.choice(7, 2, replace=False)
        rows.append((IDLE, a, 0) if g % 21 == 0 else (CNOT, a, b))
    return np.array(rows, dtype=np.int32)


def gates_of(code, name):
    if name == "idle":
        return circuit_noise.idle_gates(code.n)
    if name == "long":
        return long_gates()
    return np.asarray(cpu_ref.encode_zero_gates(code) if name == "zero" else cpu_ref.encode_plus_gates(code), dtype=np.int32)


_CACHE = {}


def circuit(code_name, gates_name):
    """(oracle code, FaultCircuit) -- the tables come from oracle.cpu_ref, nothing here needs a GPU."""
    key = (code_name, gates_name)
    if key not in _CACHE:
        if code_name not in _CACHE:
            _CACHE[code_name] = cpu_ref.CSSCode(STEANE, STEANE) if code_name == "steane" else cpu_ref.CSSCode(*rm15_checks())
        code = _CACHE[code_name]
        _CACHE[key] = (code, circuit_noise.FaultCircuit.for_code(code, gates_of(code, gates_name)))
    return _CACHE[key]


def host_counts(circ, w, first_rank=None, count=None):
    return circ.enumerate_strata([w], first_rank=first_rank, count=count, host=True).counts[0]


# ---- 1: unrank -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nb", (1, 7, 21, 64, 65))
def test_ranks_are_the_combinations_in_colexicographic_order(nb):
    for w in range(min(nb, 8) + 1):
        total = math.comb(nb, w)
        if total <= 20000:
            ranks, want = range(total), sorted(itertools.combinations(range(nb), w), key=lambda s: s[::-1])
        else:                                                                # the first and the last 10^4
            ranks = list(range(10**4)) + list(range(total - 10**4, total))
            want = [tuple(eref.unrank(nb, w, r)) for r in ranks]
        for rank, subset in zip(ranks, want):
            got = _native.subset_unrank(nb, w, rank)
            assert tuple(got.tolist()) == tuple(subset), (nb, w, rank)
        assert eref.rank_of(want[-1]) == total - 1 and tuple(want[-1]) == tuple(range(nb - w, nb))


@pytest.mark.parametrize("w", (3, 8))
def test_unrank_of_2_to_20_positions_agrees_with_python_integers(w):
    nb = 1 << 20
    top = min(math.comb(nb, w), 1 << 63)
    rng = np.random.default_rng(w)
    ranks = [0, 1, top - 1, top // 2, math.comb(nb - 1, w) - 1 if w == 3 else (1 << 62) + 12345] + [int(v) % top for v in rng.integers(0, 1 << 62, 200)]
    for rank in ranks:
        got = _native.subset_unrank(nb, w, rank).tolist()
        assert got == eref.unrank(nb, w, rank) and eref.rank_of(got) == rank, (w, rank)


def test_unrank_refusals():
    for args, text in (((7, 3, 35), "rank"), ((7, 3, -1), "rank"), ((7, 8, 0), "weight"), ((7, -1, 0), "weight"), ((21, 9, 0), "weight"),
                       ((0, 0, 0), "positions"), (((1 << 20) + 1, 1, 0), "positions"), ((7, 0, 1), "rank")):
        with pytest.raises(_native.GF2Error, match=text) as err:
            _native.subset_unrank(*args)
        assert err.value.code == _native.GF2_E_ARG
    with pytest.raises(_native.GF2Error):
        _native.subset_unrank(1 << 20, 8, 1 << 63)                           # does not fit 63 bits
    assert _native.lib().gf2_subset_unrank(7, 3, 0, None) == _native.GF2_E_ARG
    assert _native.subset_unrank(7, 0, 0).shape == (0,)


# ---- 2: the host statement against the NumPy restatement -------------------------------------------------------------------

CASES = [("steane", "idle", (0, 1, 2, 3, 4, 7)), ("steane", "zero", (0, 1, 2, 3)), ("steane", "plus", (0, 1, 2)), ("rm15", "zero", (0, 1, 2))]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s" % c[:2])
def test_host_statement_is_the_restatement(case):
    code, circ = circuit(*case[:2])
    for w in case[2]:
        got, want = host_counts(circ, w), eref.counts(code, circ.effects, w)
        print("ENUMERATE %s %s L=%d w=%d any %d of %d" % (case[0], case[1], circ.num_locations, w, int(got[:, :, 2].sum()), 3**w * math.comb(circ.num_locations, w)))
        assert got.shape == (w + 1, w + 1, 5) and np.array_equal(got, want), (case, w)
        assert all(not got[n_x, n_y].any() for n_x in range(w + 1) for n_y in range(w + 1) if n_x + n_y > w)


def test_host_statement_on_1025_locations():
    code, circ = circuit("steane", "long")
    assert circ.num_locations == 1025 and circ.effects.nbytes > 20480        # the device reads these effects through L2
    assert np.array_equal(host_counts(circ, 1), eref.counts(code, circ.effects, 1))
    first, count = math.comb(1025, 2) - 3000, 2500                           # a window deep inside the range of weight 2
    got = host_counts(circ, 2, first, count)
    assert np.array_equal(got, eref.counts(code, circ.effects, 2, first, count)) and int(got[:, :, 2].sum()) > 0


# ---- 3: ground truth that shares no code with the effect table --------------------------------------------------------------

def test_steane_code_capacity_counts_are_the_walk_of_all_4_to_7_errors():
    code, circ = circuit("steane", "idle")
    fails = sref.steane_failures(code)                                       # [any, x, z] -> (#X, #Y, #Z) of every failing error
    exact = circ.enumerate_strata(range(8), host=True)
    for w, got in zip(exact.weights, exact.counts):
        want = np.zeros((w + 1, w + 1, 5), dtype=np.uint64)
        for col, triples in ((2, fails[0]), (0, fails[1]), (1, fails[2])):
            for n_x, n_y, n_z in triples:
                if n_x + n_y + n_z == w:
                    want[n_x, n_y, col] += 1
        assert np.array_equal(got, want), w
    f = exact.fractions()
    assert f[0] == 0 and f[1] == 0 and f[2] == Fraction(7, 9) and all(isinstance(v, Fraction) for v in f)
    assert np.allclose([float(v) for v in f], [0, 0, 0.7778, 0.7333, 0.7852, 0.7490, 0.7202, 0.7888], atol=5e-5)   # DESIGN.md "Strata"
    assert exact.configurations() == [3**w * math.comb(7, w) for w in range(8)] and sum(exact.configurations()) == 4**7


@pytest.mark.parametrize("state", ("zero", "plus"))
def test_single_faults_of_the_steane_encoders_by_forward_propagation(state):
    code, circ = circuit("steane", state)
    gates, total = gates_of(code, state), circ.num_locations
    want = np.zeros((2, 2, 5), dtype=np.uint64)
    one = np.identity(total, dtype=np.uint8)
    none = np.zeros_like(one)
    for (n_x, n_y), (f_x, f_z) in (((1, 0), (one, none)), ((0, 1), (one, one)), ((0, 0), (none, one))):
        want[n_x, n_y] = sref.decode_counts(code, *propagate(gates.tolist(), code.n, f_x, f_z))
    got = host_counts(circ, 1)
    assert np.array_equal(got, want) and got[:, :, 2].sum() > 0              # the encoders are not fault tolerant


# ---- 4: range additivity -------------------------------------------------------------------------------------------------------

def test_three_unequal_ranges_sum_to_the_whole():
    _, circ = circuit("steane", "zero")
    for w in (2, 3):
        total = math.comb(21, w)
        cuts = [0, 1, total // 3 + 7, total]
        parts = [host_counts(circ, w, lo, hi - lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(parts[0] + parts[1] + parts[2], host_counts(circ, w))
        assert not host_counts(circ, w, total, 0).any() and not host_counts(circ, w, 5, 0).any()


# ---- 5: ExactStrata arithmetic -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def steane_exact():
    code, circ = circuit("steane", "idle")
    return circ.enumerate_strata(range(8), host=True), sref.steane_failures(code)[0]


def exact_rate(fails, p):
    each, rest = Fraction(p) / 3, 1 - Fraction(p)
    return sum(each ** sum(f) * rest ** (7 - sum(f)) for f in fails)


@pytest.mark.parametrize("p", (1e-3, 1e-6, 1e-9, 1e-12))
def test_rate_is_the_exact_rational(steane_exact, p):
    strata, fails = steane_exact
    got, exact = strata.rate(p), exact_rate(fails, p)
    print("ENUMERATE rate(%g) = %.15e exact %.15e" % (p, got.estimate, float(exact)))
    assert abs(Fraction(got.estimate) - exact) <= Fraction(1, 10**12) * exact
    assert got.stderr == 0.0 and got.truncation == 0.0
    # weights 0 .. 2 only: the truncation is the binomial mass of 3 .. 7 and bounds the deficit
    part = montecarlo.ExactStrata(7, strata.weights[:3], strata.counts[:3]).rate(p)
    fp = Fraction(p)
    tail = sum(math.comb(7, w) * fp**w * (1 - fp)**(7 - w) for w in range(3, 8))
    assert abs(Fraction(part.truncation) - tail) <= Fraction(1, 10**12) * tail and part.stderr == 0.0
    assert Fraction(part.estimate) <= exact <= Fraction(part.estimate) + Fraction(part.truncation) * (1 + Fraction(1, 10**12))


def test_kind_ratios_come_from_one_enumeration(steane_exact):
    strata, _ = steane_exact
    code, _ = circuit("steane", "idle")
    _, by_x, _ = sref.steane_failures(code)
    kinds = (Fraction(1, 2), Fraction(1, 5), Fraction(3, 10))
    want = [sum(kinds[0]**a * kinds[1]**b * kinds[2]**c for a, b, c in by_x if a + b + c == w) / math.comb(7, w) for w in range(8)]
    assert strata.fractions(kinds, 'logical_x') == want
    assert np.allclose(strata.fractions((0.5, 0.2, 0.3), 'logical_x'), [float(v) for v in want], rtol=1e-13, atol=0)
    assert strata.fractions((5, 2, 3), 'logical_x') == want                  # only the ratio counts
    assert strata.fractions((0, 0, 1), 'logical_x') == [0] * 8               # Z errors never flip the Z measurement
    with pytest.raises(ValueError):
        strata.fractions((0, 0, 0))


def test_leading_order(steane_exact):
    strata, _ = steane_exact
    assert strata.leading_order() == (2, Fraction(21 * 7, 9))
    assert montecarlo.ExactStrata(7, strata.weights[:2], strata.counts[:2]).leading_order() is None
    _, enc = circuit("steane", "zero")
    w, c = enc.enumerate_strata([0, 1, 2], host=True).leading_order(field='logical_x')
    assert w == 1 and c > 0                                                  # first order in p: the encoder is not fault tolerant


def test_merged_uses_exact_fractions_where_it_has_them(steane_exact):
    strata, fails = steane_exact
    low = montecarlo.ExactStrata(7, strata.weights[:3], strata.counts[:3])
    per_weight = np.bincount([sum(f) for f in fails], minlength=8)
    samples = [1000 * (w + 1) for w in range(3, 8)]
    counts = np.zeros((5, 5), dtype=np.uint64)
    counts[:, 2] = [7 * n // 10 for n in samples]
    sampled = montecarlo.Strata(7, range(3, 8), samples, counts, kinds=(2, 2, 2))
    both = low.merged(sampled)
    for p in (1e-2, 1e-6):
        got, alone = both.rate(p), sampled.rate(p)
        b = montecarlo.binomial_weights(7, p)
        assert got.stderr == alone.stderr > 0 and got.truncation == 0.0
        assert math.isclose(got.estimate, alone.estimate + b[2] * per_weight[2] / (9 * 21), rel_tol=1e-13)
        assert math.isclose(alone.truncation, b[0] + b[1] + b[2], rel_tol=1e-13)
    assert list(both.weights) == list(range(8)) and np.allclose(both.fractions()[:4], [0, 0, 7 / 9, 0.7])
    # an exact stratum replaces a sampled one of the same weight: no variance from it
    wide = montecarlo.Strata(7, range(2, 8), [500] + samples, np.vstack(([0, 0, 400, 0, 0], counts)), kinds=(1, 1, 1))
    assert low.merged(wide).rate(1e-2) == both.rate(1e-2)
    est, err, trunc = both.curve([1e-3, 2e-3])
    assert est[1] > est[0] > 0 and err[0] > 0 and trunc[0] == 0
    for call in (lambda: low.merged([sampled, montecarlo.Strata(7, [3], [10], np.zeros((1, 5)), kinds=(1, 2, 1))]),   # mismatched kinds
                 lambda: low.merged(sampled, kinds=(1, 0, 0)),
                 lambda: low.merged(montecarlo.Strata(8, [3], [10], np.zeros((1, 5)))),
                 lambda: low.merged([sampled, sampled])):
        with pytest.raises(ValueError):
            call()
    # Strata itself keeps its behaviour
    assert sampled.rate(1e-2).truncation > 0 and sampled.kinds == (2.0, 2.0, 2.0)


def test_python_layer_refusals():
    _, circ = circuit("steane", "zero")
    with pytest.raises(ValueError, match="%d fault configurations" % (27 * 1330)):
        circ.enumerate_strata([3], max_configurations=27 * 1330 - 1, host=True)
    assert circ.enumerate_strata([3], max_configurations=27 * 1330, host=True).counts[0].shape == (4, 4, 5)
    assert circuit_noise.ENUMERATE_BUDGET >= 1 << 32
    for call in (lambda: circ.enumerate_strata([9], host=True), lambda: circ.enumerate_strata([-1], host=True),
                 lambda: circ.enumerate_strata([2], first_rank=200, count=11, host=True), lambda: circ.enumerate_strata([2], first_rank=-1, host=True),
                 lambda: circuit("steane", "idle")[1].enumerate_strata([8], host=True),
                 lambda: circuit_noise.FaultCircuit(circ.gates, 7, np.ones((3, 7), dtype=np.uint8), np.ones((3, 7), dtype=np.uint8)).enumerate_strata([1], host=True)):
        with pytest.raises(ValueError):
            call()
    keys1, flips1, keys2, flips2 = circ._tables()
    for w, first, count, text in ((9, 0, 1, "weight"), (22, 0, 1, "weight"), (2, 0, 211, "leave"), (2, 210, 1, "leave"), (2, -1, 1, "leave"), (2, 0, -1, "leave")):
        with pytest.raises(_native.GF2Error, match=text) as err:
            _native.circuit_enumerate_host(circ.effects, 3, keys1, flips1, 3, keys2, flips2, w, first, count)
        assert err.value.code == _native.GF2_E_ARG
    with pytest.raises(_native.GF2Error, match="twice"):
        _native.circuit_enumerate_host(circ.effects, 3, np.vstack((keys1, keys1[:1])), np.append(flips1, 0), 3, keys2, flips2, 1, 0, 1)
    with pytest.raises(_native.GF2Error, match="words"):
        _native.circuit_enumerate_host(circ.effects, 64, keys1, flips1, 3, keys2, flips2, 1, 0, 1)


# ---- 6: sharding ---------------------------------------------------------------------------------------------------------------

SHARD_WEIGHTS = [0, 1, 2, 3]


def _host_local(circ, weights, first_rank, count):
    return circ.enumerate_strata(weights, first_rank=first_rank, count=count, host=True)


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from quantum_css_codes_amd import montecarlo
    from tests import test_enumerate
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    res = montecarlo.enumerate_sharded(test_enumerate.circuit("steane", "zero")[1], SHARD_WEIGHTS, local_fn=_host_local)
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **{"w%d" % w: c for w, c in zip(res.weights, res.counts)})
    dist.destroy_process_group()


@pytest.mark.parametrize("world", (2, 8))
def test_enumerate_sharded_gives_the_counts_of_one_rank(tmp_path, world):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    _, circ = circuit("steane", "zero")
    whole = circ.enumerate_strata(SHARD_WEIGHTS, host=True)
    for rank in range(world):
        r = np.load(tmp_path / ("rank%d.npz" % rank))
        for w, want in zip(whole.weights, whole.counts):
            assert np.array_equal(r["w%d" % w], want), (rank, w)
    alone = montecarlo.enumerate_sharded(circ, SHARD_WEIGHTS, local_fn=_host_local)      # no process group: the one shard is the whole
    assert all(np.array_equal(a, b) for a, b in zip(alone.counts, whole.counts)) and alone.nb == 21
