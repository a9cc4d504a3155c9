"""
Exact strata under gate-level faults on the GPU: gate_enumerate_kernel (csrc/gf2_gate_enumerate.hip) through
gf2_ec_gate_enumerate / gf2_ft_gate_enumerate, ECCircuit / FTProgram.enumerate_gate_range and enumerate_gate_strata, and
CSSCode.*_gate_strata_exact.  Every comparison is exact.

  whole strata    the device against the host statements gf2_ec_gate_enumerate_host / gf2_ft_gate_enumerate_host, count for count per c,
                  and against the census literals of tests/test_gate_enumerate.py (derived with the NumPy restatement)
  identity        T_w = sum_c sum_b N[w - c][b][c]: the device's site counts against the device's location counts of enumerate_strata
                  (the parent's counting kernel) on whole strata, and against the committed PAIR_COUNTS of tests/test_gadget_enumerate.py
  instantiations  every (LDR, rule, staged) of the kernel on synthetic effect tables with a mixed site table
  windows         odd counts, first ranks off every boundary, a wrap of the one-operand part inside a run, the last ranks, weight 4
  launches        a range of two launches is the sum of its parts; runs of several ranks per lane
  entry points    CSSCode.*_gate_strata_exact; refusals; count 0

The host statement is serial; a large range is handed to it in pieces on a few threads (ctypes releases the interpreter lock, the
counts of disjoint ranges add), so that no test waits for it.  Every test runs under a time limit of its own, none provokes a fault.
"""
import faulthandler
import math
from fractions import Fraction

import numpy as np
import pytest

from quantum_css_codes_amd import _native, ec_noise, ft_noise, montecarlo
from tests.test_gadget_enumerate import PAIR_COUNTS
from tests.test_gate_enumerate import CENSUS, census_of, location_totals, site_totals
from tests.test_gpu_gadget_enumerate import CYCLE_CASES, PROGRAM_CASES, in_pieces, synthetic_cycle, synthetic_program
from tests.test_gpu_strata import make_code

pytestmark = pytest.mark.gpu

SEED0 = 20261018 + 900
BUDGET = 1 << 40
TIME_LIMIT = 300                                                             # seconds per test
EC, FT = ec_noise.EC_FIELDS, ft_noise.FT_FIELDS


@pytest.fixture(autouse=True)
def own_time_limit():
    faulthandler.dump_traceback_later(TIME_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def total(gadget, w, b):
    _, n1, n2, _ = gadget.gate_sites()
    return math.comb(n1, w - b) * math.comb(n2, b)


def host(gadget, w, b, first, count):
    return in_pieces(lambda f, n: gadget.enumerate_gate_range(w, b, f, n, host=True), first, count)


def device(gadget, w, b, first=0, count=None):
    return gadget.enumerate_gate_range(w, b, first, total(gadget, w, b) - first if count is None else count)


def cycle(rounds):
    return ec_noise.circuit_for(make_code("steane"), rounds)


def program(name, ops):
    return ft_noise.program_for(make_code(name), ops)


# ---- 1: whole strata of the one-round cycle against the host statement ---------------------------------------------------------------

def test_one_round_of_the_steane_cycle_whole_to_weight_2():
    circ = cycle(1)
    assert circ.ldr == 3 and circ.effects.nbytes <= 20480                   # staged in LDS
    assert circ.gate_sites()[1:3] == (126, 102)
    for w in (0, 1, 2):
        for b in range(w + 1):
            got = device(circ, w, b)
            assert got.shape == (b + 1, len(EC))
            assert np.array_equal(got, host(circ, w, b, 0, total(circ, w, b))), (w, b)
    strata = circ.enumerate_gate_strata([0, 1])
    assert census_of(strata.counts[1], 1) == CENSUS[("cycle", "steane", 1)][3]


# ---- 2: the identity with the location strata, device against device ---------------------------------------------------------------------

def test_identity_with_the_location_strata_of_the_cycle():
    circ = cycle(1)
    sites = circ.enumerate_gate_strata([0, 1, 2, 3], max_configurations=BUDGET)      # weight 3: 1.1 x 10^9 configurations
    assert sites.configurations()[3] == sum(math.comb(126, 3 - b) * math.comb(102, b) * 3**(3 - b) * 15**b for b in range(4))
    locations = circ.enumerate_strata([2, 3], max_configurations=BUDGET)             # weight 3: 1.6 x 10^8, the parent's kernel
    for w in (2, 3):
        got, want = site_totals(sites, w).tolist(), location_totals(locations, w).tolist()
        print("GATE cycle identity w=%d accepted %d logical_any %d" % (w, got[0], got[3]))
        assert got == want, w
    assert location_totals(locations, 2)[:4].tolist() == [81161, 7821, 2652, 10263]
    c = sites.counts[3].astype(object)
    assert all(int(c[b, k, 0]) == 0 for b in range(4) for k in range(b + 1, 4)) and int(c[3, 3, 0]) > 0


# ---- 3: five rounds, through L2 ------------------------------------------------------------------------------------------------------

def test_five_rounds_of_the_steane_cycle():
    circ = cycle(5)
    assert circ.ldr == 8 and circ.effects.nbytes > 20480                    # through L2
    for w in (0, 1):
        for b in range(w + 1):
            got = device(circ, w, b)
            assert np.array_equal(got, host(circ, w, b, 0, total(circ, w, b))) and got[:, 0].sum() > 0, (w, b)
    for b, first, count in ((1, total(circ, 2, 1) // 2 + 17, 50001), (2, total(circ, 2, 2) - 20001, 20001)):
        assert np.array_equal(device(circ, 2, b, first, count), host(circ, 2, b, first, count)), b


# ---- 4: the programs ------------------------------------------------------------------------------------------------------------------

def test_gate_free_steane_program():
    prog = program("steane", "")
    assert prog.ldr == 8 and prog.gate_sites()[1:3] == (603, 491)
    sites = prog.enumerate_gate_strata([0, 1, 2])                            # weight 2: 4.2 x 10^7 configurations
    assert census_of(sites.counts[1], 1) == CENSUS[("program", "steane", "")][3]
    totals = site_totals(sites, 2)
    for name, want in PAIR_COUNTS["steane"].items():
        assert int(totals[FT.index(name)]) == sum(sum(row) for row in want), name
    for b in range(3):
        first, count = total(prog, 2, b) // 3 + 5, 30001
        assert np.array_equal(device(prog, 2, b, first, count), host(prog, 2, b, first, count)), b
    assert sites.series('independent', 'wrong') == [0, 2, Fraction(8701, 3)]
    assert sites.series(('depolarising', 1), 'wrong')[1] == Fraction(6, 5)


def test_gate_free_rm15_program_weight_1():
    prog = program("rm15", "")
    assert prog.ldr == 9 and prog.gate_sites()[1:3] == (1209, 1329)
    sites = prog.enumerate_gate_strata([0, 1])
    assert census_of(sites.counts[1], 1) == CENSUS[("program", "rm15", "")][3]
    for b in (0, 1):
        assert np.array_equal(sites.counts[1][b, :b + 1], host(prog, 1, b, 0, total(prog, 1, b))), b


# ---- 5: every instantiation on synthetic effect tables --------------------------------------------------------------------------------

def mixed_sites(rng, locations):
    """A random partition of [0, locations) into one- and two-location sites: (site_loc, n1, n2)."""
    one, two, l = [], [], 0
    while l < locations:
        if l + 1 < locations and rng.random() < 0.5:
            two.append(l)
            l += 2
        else:
            one.append(l)
            l += 1
    return np.array(one + two, dtype=np.int32), len(one), len(two)


def check_synthetic(device_fn, host_fn, sites, fields):
    """Weight 2, every b, whole: device against host.  Returns (accepted, rejected)."""
    _, n1, n2 = sites
    seen = np.zeros(2, dtype=np.int64)
    for b in range(3):
        count = math.comb(n1, 2 - b) * math.comb(n2, b)
        got = device_fn(2, b, 0, count)
        assert got.shape == (b + 1, fields)
        assert np.array_equal(got, in_pieces(lambda f, n: host_fn(2, b, f, n), 0, count)), (n1, n2, b)
        seen += (int(got[:, 0].sum()), count * 3**(2 - b) * 15**b - int(got[:, 0].sum()))
    return seen


@pytest.mark.parametrize("case", CYCLE_CASES, ids=lambda c: "rounds%d-ldr%d" % (c[0], 1 + c[0] + c[1]))
def test_every_cycle_instantiation(case):
    rounds, nflag = case
    ctx = _native.default_context()
    rng = np.random.default_rng(SEED0 + 16 * rounds + nflag)
    r1, r2 = 5, 4
    for locations in (40, 500):                                              # staged in LDS, and through L2 (test_gpu_gadget_enumerate.py)
        assert (2 * locations * (1 + rounds + nflag) * 8 <= 20480) == (locations == 40)
        eff, tables = synthetic_cycle(rng, r1, r2, rounds, nflag, locations)
        sites = mixed_sites(rng, locations)
        assert min(sites[1:]) >= 2
        circ = ctx.circuit_create(eff)
        args = (rounds, r1, tables[0], tables[1], r2, tables[2], tables[3]) + sites
        accepted, rejected = check_synthetic(lambda w, b, f, n: ctx.ec_gate_enumerate(circ, *args, w, b, f, n),
                                             lambda w, b, f, n: _native.ec_gate_enumerate_host(eff, *args, w, b, f, n), sites, len(EC))
        assert accepted > 1 and rejected > 0, (case, locations)
        circ.free()


@pytest.mark.parametrize("case", PROGRAM_CASES, ids=lambda c: "steps%d-ldr%d" % (c[0], c[0] + c[2]))
def test_every_measurement_instantiation(case):
    nsteps, mask, nflag = case
    ctx = _native.default_context()
    rng = np.random.default_rng(SEED0 + 32 * nsteps + nflag)
    r1, r2 = 4, 5
    eff, tables = synthetic_program(rng, r1, r2, nsteps, mask, nflag, 40)
    sites = mixed_sites(rng, 40)
    assert min(sites[1:]) >= 2
    circ = ctx.ft_circuit_create(eff)
    args = (nsteps, mask, r1, tables[0], tables[1], r2, tables[2], tables[3]) + sites
    accepted, rejected = check_synthetic(lambda w, b, f, n: ctx.ft_gate_enumerate(circ, *args, w, b, f, n),
                                         lambda w, b, f, n: _native.ft_gate_enumerate_host(eff, *args, w, b, f, n), sites, len(FT))
    assert accepted > 1 and rejected > 0, case
    circ.free()


def test_cases_cover_the_kernel_instantiations():
    assert {1 + r + f for r, f in CYCLE_CASES} == set(range(3, 9)) and {s + f for s, _, f in PROGRAM_CASES} == set(range(8, ft_noise.MAX_LDR + 1))


# ---- 6: windows ------------------------------------------------------------------------------------------------------------------------

def test_windows_of_the_measurement():
    prog = program("steane", "XXX")
    _, n1, n2, _ = prog.gate_sites()
    assert (n1, n2, prog.ldr) == (990, 797, 11)
    c1 = n1                                                                  # (2, 1): C(n_1, 1) one-operand subsets per CNOT
    for first, count in ((0, 1), (12345, 4097), (77, 257), (33, 31), (5 * c1 - 3, 7), (7 * c1 - 1, 2), (total(prog, 2, 1) - 1000, 1000)):
        assert np.array_equal(device(prog, 2, 1, first, count), host(prog, 2, 1, first, count)), (first, count)
    for b, first, count in ((0, total(prog, 2, 0) - 777, 777), (2, 99, 10001), (2, total(prog, 2, 2) - 1, 1)):
        assert np.array_equal(device(prog, 2, b, first, count), host(prog, 2, b, first, count)), (b, first, count)
    # runs of two ranks per lane, the one-operand part wrapping inside runs: 2^20 + 4097 subsets of (3, 1) from just below a wrap
    c1 = math.comb(n1, 2)
    first, count = 5 * c1 - 1001, (1 << 20) + 4097
    assert count // (2048 * 256) == 2 and count > 2 * c1
    got = device(prog, 3, 1, first, count)
    assert np.array_equal(got, host(prog, 3, 1, first, count)) and got[:, 0].sum() > 0
    # weight 4: 2 001 subsets of (4, 2) across a wrap, 2 025 kinds each
    first = 3 * c1 - 1000
    assert np.array_equal(device(prog, 4, 2, first, 2001), host(prog, 4, 2, first, 2001))
    first = total(prog, 4, 4) - 40
    assert np.array_equal(device(prog, 4, 4, first, 40), host(prog, 4, 4, first, 40))


# ---- 7: two launches --------------------------------------------------------------------------------------------------------------------

def test_a_range_of_two_launches_is_the_sum_of_its_parts():
    """A launch covers 2^28 configurations.  (w, b) = (3, 2) of the one-round cycle is 126 C(102, 2) = 649 026 subsets of 675 kinds
    each: two launches.  Three unequal parts must add up to the whole, and the two edge parts are the host statement's."""
    circ = cycle(1)
    all_ = total(circ, 3, 2)
    per_launch = (1 << 28) // 675
    assert all_ == 649026 and per_launch < all_ <= 2 * per_launch
    whole = device(circ, 3, 2)
    cuts = [0, 30001, all_ - 29999, all_]
    parts = [device(circ, 3, 2, lo, hi - lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(parts[0] + parts[1] + parts[2], whole)
    assert 0 < int(whole[:, 0].sum()) < 675 * all_
    for part, (lo, hi) in ((parts[0], cuts[:2]), (parts[2], cuts[2:])):
        assert np.array_equal(part, host(circ, 3, 2, lo, hi - lo))
    got = device(circ, 3, 2, per_launch - 300, 700)                          # across the cut
    assert np.array_equal(got, host(circ, 3, 2, per_launch - 300, 700))


# ---- 8: runs longer than one rank ---------------------------------------------------------------------------------------------------------

def test_runs_of_several_ranks_per_lane():
    prog = program("steane", "XXX")
    count = (1 << 21) + 12345                                                # b = 0, a = 3: 27 kinds, one launch, runs of four ranks
    first = total(prog, 3, 0) // 2 + 54321
    assert count * 27 < (1 << 28) and count // (2048 * 256) == 4 and first + count < total(prog, 3, 0)
    got = device(prog, 3, 0, first, count)
    assert np.array_equal(got, host(prog, 3, 0, first, count)) and got[0, 0] > 0


# ---- 9: public entry points and refusals ---------------------------------------------------------------------------------------------------

def test_public_entry_points():
    code = make_code("steane")
    ec = code.error_correct_gate_strata_exact([0, 1, 2])
    assert isinstance(ec, montecarlo.GateStrata) and ec.fields == EC and (ec.n1, ec.n2) == (126, 102)
    assert ec.leading_order(('depolarising', 1), 'logical_x') == (1, Fraction(3, 5))
    assert ec.series('independent', 'logical_any') == code.error_correct_strata_exact([0, 1, 2]).series((1, 1, 1), 'logical_any')
    host_strata = ec_noise.circuit_for(code, 1).enumerate_gate_strata([0, 1, 2], host=True)
    assert all(np.array_equal(a, b) for a, b in zip(ec.counts, host_strata.counts))
    classes, flipping = code.error_correct_gate_single_faults()
    assert int((classes & 1 != 0).sum()) == int(ec.counts[1][:, :, 0].sum()) == 652 and len(flipping) == int(ec.counts[1][:, :, 3].sum())
    ft = code.logical_program_gate_strata_exact('XXX', [0, 1])
    assert ft.fields == FT and census_of(ft.counts[1], 1) == CENSUS[("program", "steane", "XXX")][3]
    assert ft.series(('depolarising', 1), 'wrong') == [0, 3] and len(code.logical_program_gate_single_faults('XXX')[1]) == 45
    estimate, lower, upper = ec.rate(montecarlo.GateStrata.depolarising_odds(1e-4, 1e-4), 'logical_any')
    assert lower <= estimate <= upper and abs(estimate - 0.6e-4) < 1e-5


def test_refusals():
    code = make_code("steane")
    ctx = _native.default_context()
    circ, prog = ec_noise.circuit_for(code, 1), ft_noise.program_for(code, "")
    tables = circ._tables()
    ec_sites, ft_sites = circ.gate_sites()[:3], prog.gate_sites()[:3]
    ec = lambda device=None, rounds=1, sites=ec_sites, w=1, b=0, first=0, count=1: \
        ctx.ec_gate_enumerate(circ.device() if device is None else device, rounds, *tables, *sites, w, b, first, count)
    ft = lambda device=None, nsteps=prog.nsteps, mask=prog.measure_mask, sites=ft_sites, w=1, b=0, first=0, count=1: \
        ctx.ft_gate_enumerate(prog.device() if device is None else device, nsteps, mask, *tables, *sites, w, b, first, count)
    rng = np.random.default_rng(SEED0 + 9)
    five = rng.integers(0, 1 << 62, (30, 2, 5)).astype("<u8")                # the Monte-Carlo layout is no cycle: its effects leave the layout
    five[:, :, 4] &= np.uint64(3)
    five_dev = ctx.circuit_create(five)
    thirty = (np.arange(30, dtype=np.int32), 30, 0)
    twice = ec_sites[0].copy()
    twice[5] = twice[6]
    for call, text in ((lambda: ec(five_dev, sites=thirty), "beyond"), (lambda: ft(five_dev, nsteps=4, mask=1, sites=thirty), "8 <= ldr"),
                       (lambda: ft(circ.device(), nsteps=2, mask=1, sites=ec_sites), "8 <= ldr"),
                       (lambda: ec(ft_noise.program_for(code, "XXX").device(), rounds=6), "ldr <= 8"), (lambda: ec(rounds=2), "rounds need"),
                       (lambda: ec(w=5), "weight"), (lambda: ec(w=2, b=3), "CNOT picks"), (lambda: ec(w=2, b=1, count=126 * 102 + 1), "leave"),
                       (lambda: ec(first=-1), "leave"), (lambda: ec(sites=(twice, 126, 102)), "partition"),
                       (lambda: ec(sites=(ec_sites[0][:-1], 126, 101)), "partition"), (lambda: ft(sites=ec_sites), "partition"),
                       (lambda: ft(w=2, b=1, first=603 * 491, count=1), "leave")):
        with pytest.raises(_native.GF2Error, match=text) as err:
            call()
        assert err.value.code == _native.GF2_E_ARG, text
    five_dev.free()
    for call in (lambda: circ.enumerate_gate_strata([3], max_configurations=100), lambda: prog.enumerate_gate_strata([3]),
                 lambda: circ.enumerate_gate_strata([5])):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match=r"\d+ gate-fault configurations to enumerate, more than max_configurations"):
        prog.enumerate_gate_strata([3])                                      # 3.6 x 10^10 configurations: beyond the default budget
    assert not ec(w=2, b=1, first=100, count=0).any() and ec(w=2, b=1, first=100, count=0).shape == (2, 8)
    assert not ft(w=2, b=2, first=100, count=0).any() and ft(w=2, b=2, first=100, count=0).shape == (3, 7)
