"""
Exact strata on the GPU (DESIGN.md section 5 "Exact strata"): enumerate_kernel (csrc/gf2_enumerate.hip) through
gf2_circuit_enumerate, FaultCircuit.enumerate_strata and CSSCode.*_strata_exact.

  exact     the device against the host statement gf2_circuit_enumerate_host, count for count per composition: the cases of
            tests/test_enumerate.py, the 1025-location circuit at full weight 2 and on a window of 2^20 ranks of weight 3, the
            ldr = 3, 4 and 5 layouts, counts that are no multiple of the workgroup, ranges that span several launches
  sampler   ONE full weight-3 enumeration of the 1025-location circuit (4.8 x 10^9 configurations) against
            logical_error_strata([3], 10^8): every field within the suite's two-sided bound (oracle/exact_dist.py, p >= 10^-6)
  refusals  weight above 8 or L, ranges outside [0, C(L, w)), a circuit without a code, n > 128

Every test runs under a time limit of its own (a watchdog that ends the process), none provokes a fault.
"""
import faulthandler
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import exact_dist as ed
from quantum_css_codes_amd import _native, circuit_noise, montecarlo
from tests import strata_ref as sref
from tests.test_enumerate import long_gates
from tests.test_gpu_strata import make_code

pytestmark = pytest.mark.gpu

SEED0 = 20261017 + 400
FIELDS = montecarlo.DECODE_FIELDS
TIME_LIMIT = 600                                                             # seconds per test


@pytest.fixture(autouse=True)
def own_time_limit():
    faulthandler.dump_traceback_later(TIME_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def circuit(code_name, gates_name):
    code = make_code(code_name)
    gates = {"idle": lambda: circuit_noise.idle_gates(code.n), "long": long_gates}.get(gates_name, lambda: circuit_noise.encoder_gates(code, gates_name))()
    return circuit_noise.circuit_for(code, gates)


def both(circ, w, first_rank=None, count=None):
    """(device, host) counts of one weight."""
    budget = 1 << 40
    got = circ.enumerate_strata([w], first_rank=first_rank, count=count, max_configurations=budget).counts[0]
    want = circ.enumerate_strata([w], first_rank=first_rank, count=count, max_configurations=budget, host=True).counts[0]
    return got, want


# ---- 1: the device against the host statement ------------------------------------------------------------------------------

CASES = [("steane", "idle", (0, 1, 2, 3, 4, 5, 6, 7)), ("steane", "zero", (0, 1, 2, 3, 4)), ("steane", "plus", (0, 1, 2)), ("rm15", "zero", (0, 1, 2)),
         ("steane", "long", (0, 1, 2)), ((100, 25, 3), "idle", (0, 1, 2, 3))]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s" % c[:2])
def test_device_counts_are_the_host_statement(case):
    circ = circuit(*case[:2])
    if case[0] == (100, 25, 3):
        assert circ.ldr == 4 and circ.code.r_2 > 63                          # two-word key_x
    for w in case[2]:
        got, want = both(circ, w)
        print("ENUMERATE %s %s L=%d w=%d any %d of %d" % (case[0], case[1], circ.num_locations, w, int(got[:, :, 2].sum()), 3**w * math.comb(circ.num_locations, w)))
        assert np.array_equal(got, want), (case, w)


def test_public_entry_points_agree():
    code = make_code("steane")
    exact = code.logical_error_strata_exact(range(8))
    assert exact.nb == 7 and exact.fractions()[:3] == [0, 0, Fraction(7, 9)] and exact.leading_order() == (2, Fraction(49, 3))
    assert np.allclose([float(f) for f in exact.fractions()], [0, 0, 0.7778, 0.7333, 0.7852, 0.7490, 0.7202, 0.7888], atol=5e-5)
    enc = code.encoder_logical_error_strata_exact('zero', [0, 1, 2])
    same = code.circuit_logical_error_strata_exact(circuit_noise.encoder_gates(code, 'zero'), [0, 1, 2])
    assert enc.nb == 21 and all(np.array_equal(a, b) for a, b in zip(enc.counts, same.counts))
    assert enc.leading_order(field='logical_x')[0] == 1                      # one fault in the encoder can flip the logical qubit
    alone = montecarlo.enumerate_sharded(circuit("steane", "zero"), [0, 1, 2])           # no process group: the one shard is the whole
    assert all(np.array_equal(a, b) for a, b in zip(alone.counts, enc.counts))


def test_windows_odd_counts_and_a_deep_window_of_weight_3():
    circ = circuit("steane", "long")
    total = math.comb(1025, 3)
    for first, count in ((0, 1), (12345, 255), (77, 257), (total - 1000, 1000), (total // 2 + 13, 100003)):   # no multiples of 256
        got, want = both(circ, 3, first, count)
        assert np.array_equal(got, want) and int(got.sum(axis=(0, 1))[2]) <= 27 * count, (first, count)
    first = total // 2 + 987654321 % 1000003                                 # 2^20 ranks deep inside the range
    got, want = both(circ, 3, first, 1 << 20)
    assert np.array_equal(got, want) and got[:, :, 2].sum() > 0
    enc = circuit("steane", "zero")
    whole, _ = both(enc, 3)
    parts = [both(enc, 3, lo, hi - lo)[0] for lo, hi in ((0, 1), (1, 450), (450, 1330))]
    assert np.array_equal(parts[0] + parts[1] + parts[2], whole)


def synthetic(rng, r1, r2, locations):
    """A random effect table in the Monte-Carlo layout and tables that hold half of the keys single faults produce."""
    kwx, kwz = (1 if r2 <= 63 else 2), (1 if r1 <= 63 else 2)
    ldr = kwx + kwz + 1
    eff = np.zeros((locations, 2, ldr), dtype="<u8")
    for first, kw, r in ((0, kwx, r2), (kwx, kwz, r1)):
        bits = rng.integers(0, 2, (locations, 2, 64 * kw), dtype=np.uint8)
        bits[:, :, r:] = 0
        eff[:, :, first:first + kw] = np.packbits(bits, axis=2, bitorder="little").view("<u8")
    eff[:, :, ldr - 1] = rng.integers(0, 4, (locations, 2))
    tables = []
    for first, kw in ((kwx, kwz), (0, kwx)):                                 # table 1 (key_z), table 2 (key_x)
        keys = np.ascontiguousarray(np.unique(eff[:, :, first:first + kw].reshape(-1, kw), axis=0)[::2])
        tables += [keys, rng.integers(0, 2, len(keys), dtype=np.uint8)]
    return eff, tables


@pytest.mark.parametrize("case", [(3, 3, 3), (64, 63, 4), (40, 70, 4), (70, 70, 5)], ids=lambda c: "ldr%d-%d-%d" % (c[2], c[0], c[1]))
def test_every_layout_staged_and_through_l2(case):
    r1, r2, ldr = case
    ctx = _native.default_context()
    rng = np.random.default_rng(SEED0 + r1)
    for locations in (1, 60, 700):                                           # 700 x 2 x ldr words are beyond the 20 KiB staged in LDS
        eff, (keys1, flips1, keys2, flips2) = synthetic(rng, r1, r2, locations)
        assert eff.shape[2] == ldr and (eff.nbytes > 20480) == (locations == 700)
        circ = ctx.circuit_create(eff)
        for w in range(min(locations, 3 if locations < 700 else 2) + 1):
            total = math.comb(locations, w)
            for first, count in ((0, total), (total // 3, total - total // 3)):
                got = ctx.circuit_enumerate(circ, r1, keys1, flips1, r2, keys2, flips2, w, first, count)
                want = _native.circuit_enumerate_host(eff, r1, keys1, flips1, r2, keys2, flips2, w, first, count)
                assert np.array_equal(got, want), (case, locations, w, first)
            assert got[:, :, 3:].sum() > 0 or w == 0 or locations == 1      # half of the keys are missing: uncorrectable counts


def test_a_range_of_several_launches_is_the_sum_of_its_parts():
    """3^8 C(21, 8) = 1.3 x 10^9 configurations of the Steane encoder are two launches; three unequal parts of one launch each
    (163 659 subsets at most) must add up to them, and a part is the host statement's."""
    circ = circuit("steane", "zero")
    total, budget = math.comb(21, 8), 1 << 40
    assert 3**8 * total > 1 << 30 and 80001 * 3**8 < 1 << 30
    whole = circ.enumerate_strata([8], max_configurations=budget).counts[0]
    cuts = [0, 70000, 150001, total]
    parts = [circ.enumerate_strata([8], first_rank=lo, count=hi - lo, max_configurations=budget).counts[0] for lo, hi in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(parts[0] + parts[1] + parts[2], whole)
    assert int(whole.sum(axis=(0, 1))[3:].sum()) == 0 and 0 < int(whole[:, :, 2].sum()) < 3**8 * total
    got, want = both(circ, 8, 150001 - 300, 700)                             # across the cut, 4.6 x 10^6 configurations on the host
    assert np.array_equal(got, want)


# ---- 2: one full enumeration of weight 3 against the sampler ------------------------------------------------------------------

def test_full_weight_3_of_1025_locations_against_the_sampler():
    circ = circuit("steane", "long")
    count, kinds = 10**8, (1, 1, 1)
    exact = circ.enumerate_strata([3], max_configurations=1 << 40)
    assert exact.configurations() == [27 * math.comb(1025, 3)] and exact.configurations()[0] > 4.8e9
    t_1, t_2 = sref.thresholds(kinds)                                        # the sampler's kinds are quantised to 2^-32
    q = (Fraction(t_1, 1 << 32), Fraction(t_2 - t_1, 1 << 32), Fraction((1 << 32) - t_2, 1 << 32))
    sampled = circ.logical_error_strata([3], count, kinds=kinds, seed=SEED0 + 1)
    for k, name in enumerate(FIELDS):
        f = float(exact.fractions(q, name)[0])
        print("ENUMERATE 1025 locations f_3 %s exact %.9f sampled %.9f" % (name, f, int(sampled.counts[0, k]) / count))
        ed.assert_z("1025 locations stratum 3 " + name, int(sampled.counts[0, k]), count * f, count * f * (1 - f))
    assert exact.fractions(q, 'logical_any')[0] > 0
    merged = exact.merged(circ.logical_error_strata([4], 10**6, kinds=kinds, seed=SEED0 + 2))
    assert merged.rate(1e-6).stderr < 1e-3 * merged.rate(1e-6).estimate


# ---- 3: refused arguments -----------------------------------------------------------------------------------------------------

def test_refused_enumerations():
    code = make_code("steane")
    circ, short = circuit("steane", "zero"), circuit("steane", "idle")       # L = 21, L = 7
    ctx = _native.default_context()
    keys1, flips1, keys2, flips2 = circ._tables()
    for circuit_, w, first, count, text in ((circ, 9, 0, 1, "weight"), (short, 8, 0, 1, "weight"), (circ, -1, 0, 1, "weight"),
                                            (circ, 2, 0, 211, "leave"), (circ, 2, 210, 1, "leave"), (circ, 2, -1, 1, "leave"), (circ, 2, 5, -1, "leave")):
        with pytest.raises(_native.GF2Error, match=text) as err:
            ctx.circuit_enumerate(circuit_.device(), 3, keys1, flips1, 3, keys2, flips2, w, first, count)
        assert err.value.code == _native.GF2_E_ARG
    for call in (lambda: circ.enumerate_strata([9]), lambda: short.enumerate_strata([8]), lambda: circ.enumerate_strata([2], first_rank=200, count=11),
                 lambda: circ.enumerate_strata([3], max_configurations=100)):
        with pytest.raises(ValueError):
            call()
    assert not ctx.circuit_enumerate(circ.device(), 3, keys1, flips1, 3, keys2, flips2, 2, 210, 0).any()
    with pytest.raises(_native.GF2Error, match="twice"):
        ctx.circuit_enumerate(circ.device(), 3, np.vstack((keys1, keys1[:1])), np.append(flips1, 0), 3, keys2, flips2, 1, 0, 1)
    with pytest.raises(_native.GF2Error, match="words"):
        ctx.circuit_enumerate(circ.device(), 64, keys1, flips1, 3, keys2, flips2, 1, 0, 1)
    # a circuit that was not made by for_code has no tables to decode with
    bare = circuit_noise.FaultCircuit(circ.gates, 7, np.ones((3, 7), dtype=np.uint8), np.ones((3, 7), dtype=np.uint8))
    with pytest.raises(ValueError, match="for_code"):
        bare.enumerate_strata([1])
    # n > 128: no syndrome tables to look the frame up in
    class Wide(object):
        n, r_1, r_2 = 129, 3, 3
    wide = circuit_noise.FaultCircuit(circuit_noise.idle_gates(129), 129, np.ones((3, 129), dtype=np.uint8), np.ones((3, 129), dtype=np.uint8), code=Wide())
    with pytest.raises(ValueError, match="n <= 128"):
        wide.enumerate_strata([1])
    assert code.logical_error_strata_exact([1]).counts[0].sum() == 0
