"""
Exact strata of the two post-selected gadgets on the GPU (DESIGN.md sections 5b "Exact strata of the cycle" and 5c "Exact strata of the
measurement"): gadget_enumerate_kernel (csrc/gf2_gadget_enumerate.hip) through gf2_ec_enumerate / gf2_ft_enumerate,
ECCircuit / FTProgram.enumerate_strata and CSSCode.*_strata_exact.  Every comparison is exact.

  whole strata    the device against the host statements gf2_ec_enumerate_host / gf2_ft_enumerate_host, count for count per
                  composition, and against the literals of tests/test_gadget_enumerate.py (re-derived with the NumPy restatement)
  instantiations  every (LDR, rule, staged) of the kernel on synthetic effect tables
  windows         odd counts, first ranks off every boundary, one rank, the last ranks, 2^20 ranks deep inside weight 3, parts
  launches        a range of several launches is the sum of single-launch parts; a window across a cut
  entry points    CSSCode.logical_program_strata_exact / error_correct_strata_exact, montecarlo.enumerate_sharded
  refusals        layouts, ldr, budget; count 0

The host statement is serial; a large range is handed to it in pieces on a few threads (ctypes releases the interpreter lock, the
counts of disjoint ranges add), so that no test waits for it.  Every test runs under a time limit of its own, none provokes a fault.
"""
import concurrent.futures
import faulthandler
import math

import numpy as np
import pytest

from quantum_css_codes_amd import _native, circuit_noise, ec_noise, ft_noise, montecarlo
from tests.test_gadget_enumerate import PAIR_COUNTS, SINGLE_COUNTS
from tests.test_gpu_strata import make_code

pytestmark = pytest.mark.gpu

SEED0 = 20261018 + 500
BUDGET = 1 << 40
TIME_LIMIT = 600                                                             # seconds per test
HOST_THREADS = 16
EC, FT = ec_noise.EC_FIELDS, ft_noise.FT_FIELDS


@pytest.fixture(autouse=True)
def own_time_limit():
    faulthandler.dump_traceback_later(TIME_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def in_pieces(host_fn, first, count):
    """host_fn(first, count) summed over up to HOST_THREADS pieces of the range, one thread each."""
    if count < 4096:
        return host_fn(first, count)
    cuts = [first + count * k // HOST_THREADS for k in range(HOST_THREADS + 1)]
    with concurrent.futures.ThreadPoolExecutor(HOST_THREADS) as pool:
        parts = list(pool.map(lambda lo_hi: host_fn(lo_hi[0], lo_hi[1] - lo_hi[0]), zip(cuts[:-1], cuts[1:])))
    return sum(parts[1:], parts[0])


def gadget_host(gadget, w, first, count):
    one = lambda f, n: gadget.enumerate_strata([w], first_rank=f, count=n, max_configurations=BUDGET, host=True).counts[0]
    return in_pieces(one, first, count)


def gadget_device(gadget, w, first=None, count=None):
    return gadget.enumerate_strata([w], first_rank=first, count=count, max_configurations=BUDGET).counts[0]


def cycle(rounds):
    return ec_noise.circuit_for(make_code("steane"), rounds)


def program(name, ops):
    return ft_noise.program_for(make_code(name), ops)


# ---- 1: whole strata against the host statement ----------------------------------------------------------------------------------

def test_one_round_of_the_steane_cycle_whole_to_weight_3():
    circ = cycle(1)
    assert circ.ldr == 3 and circ.effects.nbytes <= 20480                   # staged in LDS
    L = circ.num_locations
    for w in (0, 1, 2):
        got = gadget_device(circ, w)
        assert np.array_equal(got, gadget_host(circ, w, 0, math.comb(L, w))), w
    whole = gadget_device(circ, 3)                                           # 1.6 x 10^8 configurations
    total = math.comb(L, 3)
    print("GADGET cycle L=%d w=3 accepted %d logical_any %d of %d" % (L, int(whole[:, :, 0].sum()), int(whole[:, :, 3].sum()), 27 * total))
    cuts = [0, 70001, total - 99999, total]
    parts = [gadget_device(circ, 3, lo, hi - lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(parts[0] + parts[1] + parts[2], whole)
    for part, (lo, hi) in ((parts[0], cuts[:2]), (parts[2], cuts[2:])):      # two windows of it on the host
        assert np.array_equal(part, gadget_host(circ, 3, lo, hi - lo))
    assert 0 < int(whole[:, :, 3].sum()) < int(whole[:, :, 0].sum()) < 27 * total


def test_five_rounds_of_the_steane_cycle():
    circ = cycle(5)
    assert circ.ldr == 8 and circ.effects.nbytes > 20480                    # through L2
    for w in (0, 1, 2):
        got = gadget_device(circ, w)
        assert np.array_equal(got, gadget_host(circ, w, 0, math.comb(circ.num_locations, w))), w
        assert got[:, :, 0].sum() > 0


@pytest.mark.parametrize("name, ldr", [("steane", 8), ("rm15", 9)])
def test_gate_free_programs_to_weight_1(name, ldr):
    prog = program(name, "")
    assert prog.ldr == ldr
    for w in (0, 1):
        got = gadget_device(prog, w)
        assert np.array_equal(got, gadget_host(prog, w, 0, math.comb(prog.num_locations, w))), w
    assert got[:, :, :2].tolist() == SINGLE_COUNTS[name]                     # accepted and wrong by kind: the census


# ---- 2: the whole weight-2 strata against the committed literals -------------------------------------------------------------------

@pytest.mark.parametrize("name", ["steane", "rm15"])
def test_weight_2_of_the_gate_free_programs_is_the_committed_table(name):
    prog = program(name, "")
    got = gadget_device(prog, 2)                                             # 11.3 and 67.3 million configurations
    want = PAIR_COUNTS[name]
    assert got[:, :, 0].tolist() == want['accepted'] and got[:, :, 1].tolist() == want['wrong']
    if name == "rm15":
        assert int(got[:, :, 5].sum()) > 0                                   # unmatched x keys occur


# ---- 3: every instantiation on synthetic effect tables -----------------------------------------------------------------------------

def synthetic_tables(rng, keys_x, keys_z):
    """Tables 1 (key_z) and 2 (key_x) holding half of the keys that occur."""
    out = []
    for keys in (keys_z, keys_x):
        half = np.ascontiguousarray(np.unique(keys)[::2]).astype("<u8")
        out += [half, rng.integers(0, 2, len(half), dtype=np.uint8)]
    return out


def flag_words(rng, locations, nflag):
    """Sparse flag bits: about a third of the effects trip one of two verifications, so that configurations are accepted and
    rejected, and two faults can hide each other.  The 500-location tables trip five times in six, with one of 63 patterns: the real
    gadgets reject most configurations too, and the serial host statement, whose time goes into the accepted ones, stays within
    seconds at weight 3."""
    words = np.zeros((locations, 2, nflag), dtype="<u8")
    small = locations <= 40
    hit = rng.random((locations, 2)) < (0.35 if small else 0.85)
    words[hit, rng.integers(0, nflag, int(hit.sum()))] = rng.integers(1, 3 if small else 64, int(hit.sum())).astype(np.uint64)
    return words


def synthetic_cycle(rng, r1, r2, rounds, nflag, locations):
    ldr = 1 + rounds + nflag
    eff = np.zeros((locations, 2, ldr), dtype="<u8")
    key_x = rng.integers(0, 1 << r2, (locations, 2, 1 + rounds)).astype(np.uint64)
    key_z = rng.integers(0, 1 << r1, (locations, 2, 1 + rounds)).astype(np.uint64)
    eff[:, :, :1 + rounds] = key_x | key_z << np.uint64(32)
    eff[:, :, 0] |= rng.integers(0, 2, (locations, 2)).astype(np.uint64) << np.uint64(31) | rng.integers(0, 2, (locations, 2)).astype(np.uint64) << np.uint64(63)
    eff[:, :, 1 + rounds:] = flag_words(rng, locations, nflag)
    return eff, synthetic_tables(rng, key_x, key_z)


def synthetic_program(rng, r1, r2, nsteps, mask, nflag, locations):
    eff = np.zeros((locations, 2, nsteps + nflag), dtype="<u8")
    key_x = rng.integers(0, 1 << r2, (locations, 2, nsteps)).astype(np.uint64)
    key_z = rng.integers(0, 1 << r1, (locations, 2, nsteps)).astype(np.uint64)
    for s in range(nsteps):
        if (mask >> s) & 1:
            eff[:, :, s] = key_x[:, :, s] | rng.integers(0, 2, (locations, 2)).astype(np.uint64) << np.uint64(31)
        else:
            eff[:, :, s] = key_x[:, :, s] | key_z[:, :, s] << np.uint64(32)
    eff[:, :, nsteps:] = flag_words(rng, locations, nflag)
    return eff, synthetic_tables(rng, key_x, key_z)


#              rounds, flag words -> LDR 3 .. 8
CYCLE_CASES = [(1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1), (1, 3), (2, 5)]
#                nsteps, measure_mask, flag words -> LDR 8 .. 16
PROGRAM_CASES = [(7, 0b0010101, 1), (7, 0b1000000, 2), (9, 0b001010100, 1), (8, 0b00101010, 3), (11, 0b00101010101, 1), (12, 0b000000010101, 1),
                 (13, 0b0101010000000, 1), (13, 0b1010101010101, 2), (15, 0b001010101010101, 1)]
CYCLE_LOCATIONS, PROGRAM_LOCATIONS = (1, 40, 500), (1, 40)


def test_cases_cover_the_kernel_instantiations():
    staged = {(1 + r + f, 2 * loc * (1 + r + f) * 8 <= 20480) for r, f in CYCLE_CASES for loc in CYCLE_LOCATIONS}
    assert staged == {(ldr, s) for ldr in range(3, 9) for s in (True, False)}
    assert {r for r, _ in CYCLE_CASES} == set(range(1, ec_noise.MAX_ROUNDS + 1))
    assert all(2 * 500 * ldr * 8 > 20480 for ldr in range(3, 9))
    assert {s + f for s, _, f in PROGRAM_CASES} == set(range(8, ft_noise.MAX_LDR + 1))
    assert all(bin(m).count("1") % 2 == 1 and m >> s == 0 for s, m, _ in PROGRAM_CASES)


def check_synthetic(device_fn, host_fn, locations, fields):
    """Weights 0 .. 3, each whole and as a second window from a third of the way in, device against host."""
    seen = np.zeros(2, dtype=np.int64)
    for w in range(min(locations, 3) + 1):
        total = math.comb(locations, w)
        third = total // 3
        head, tail = in_pieces(lambda f, n: host_fn(w, f, n), 0, third), in_pieces(lambda f, n: host_fn(w, f, n), third, total - third)
        whole = device_fn(w, 0, total)
        assert np.array_equal(whole, head + tail), (locations, w, "whole")
        assert np.array_equal(device_fn(w, third, total - third), tail), (locations, w, "window")
        assert whole.shape == (w + 1, w + 1, fields)
        seen += (int(whole[:, :, 0].sum()), 3**w * total - int(whole[:, :, 0].sum()))
    return seen


@pytest.mark.parametrize("case", CYCLE_CASES, ids=lambda c: "rounds%d-ldr%d" % (c[0], 1 + c[0] + c[1]))
def test_every_cycle_instantiation(case):
    rounds, nflag = case
    ctx = _native.default_context()
    rng = np.random.default_rng(SEED0 + 16 * rounds + nflag)
    r1, r2 = 5, 4
    for locations in CYCLE_LOCATIONS:
        eff, tables = synthetic_cycle(rng, r1, r2, rounds, nflag, locations)
        circ = ctx.circuit_create(eff)
        args = (rounds, r1, tables[0], tables[1], r2, tables[2], tables[3])
        accepted, rejected = check_synthetic(lambda w, f, n: ctx.ec_enumerate(circ, *args, w, f, n),
                                             lambda w, f, n: _native.ec_enumerate_host(eff, *args, w, f, n), locations, len(EC))
        assert locations == 1 or (accepted > 1 and rejected > 0), (case, locations)
        circ.free()


@pytest.mark.parametrize("case", PROGRAM_CASES, ids=lambda c: "steps%d-ldr%d" % (c[0], c[0] + c[2]))
def test_every_measurement_instantiation(case):
    nsteps, mask, nflag = case
    ctx = _native.default_context()
    rng = np.random.default_rng(SEED0 + 32 * nsteps + nflag)
    r1, r2 = 4, 5
    for locations in PROGRAM_LOCATIONS:
        eff, tables = synthetic_program(rng, r1, r2, nsteps, mask, nflag, locations)
        circ = ctx.ft_circuit_create(eff)
        args = (nsteps, mask, r1, tables[0], tables[1], r2, tables[2], tables[3])
        accepted, rejected = check_synthetic(lambda w, f, n: ctx.ft_enumerate(circ, *args, w, f, n),
                                             lambda w, f, n: _native.ft_enumerate_host(eff, *args, w, f, n), locations, len(FT))
        assert locations == 1 or (accepted > 1 and rejected > 0), (case, locations)
        circ.free()


# ---- 4: windows ------------------------------------------------------------------------------------------------------------------

def test_windows_of_the_measurement():
    prog = program("steane", "XXX")
    L = prog.num_locations
    assert (L, prog.ldr) == (2584, 11)
    total = math.comb(L, 2)
    for first, count in ((0, 1), (12345, 4097), (77, 257), (33, 31), (total - 1000, 1000), (total // 2 + 13, 100003)):
        assert np.array_equal(gadget_device(prog, 2, first, count), gadget_host(prog, 2, first, count)), (first, count)
    total = math.comb(L, 3)
    first = total // 2 + 987654321 % 1000003                                 # 2^20 ranks deep inside weight 3
    got = gadget_device(prog, 3, first, 1 << 20)
    assert np.array_equal(got, gadget_host(prog, 3, first, 1 << 20)) and got[:, :, 0].sum() > 0
    whole = gadget_device(prog, 2)
    cuts = [0, 1, 1234567, math.comb(L, 2)]
    parts = [gadget_device(prog, 2, lo, hi - lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(parts[0] + parts[1] + parts[2], whole)


# ---- 5: several launches -----------------------------------------------------------------------------------------------------------

def test_a_range_of_several_launches_is_the_sum_of_its_parts():
    """A launch covers 2^28 configurations: 40 913 subsets of weight 8.  120 000 subsets of a synthetic 21-location cycle are three
    launches; three unequal parts of one launch each must add up to them, and a window across the first cut is the host statement's."""
    ctx = _native.default_context()
    rng = np.random.default_rng(SEED0 + 5)
    eff, tables = synthetic_cycle(rng, 3, 3, 1, 1, 21)
    circ = ctx.circuit_create(eff)
    args = (1, 3, tables[0], tables[1], 3, tables[2], tables[3])
    per_launch = (1 << 28) // 3**8
    assert per_launch == 40913 and 120000 <= math.comb(21, 8) and 2 * per_launch < 120000
    whole = ctx.ec_enumerate(circ, *args, 8, 0, 120000)
    cuts = [0, 40000, 80001, 120000]
    parts = [ctx.ec_enumerate(circ, *args, 8, lo, hi - lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(parts[0] + parts[1] + parts[2], whole)
    assert 0 < int(whole[:, :, 0].sum()) < 3**8 * 120000
    got = ctx.ec_enumerate(circ, *args, 8, per_launch - 300, 700)           # across the cut, 4.6 x 10^6 configurations on the host
    want = in_pieces(lambda f, n: _native.ec_enumerate_host(eff, *args, 8, f, n), per_launch - 300, 700)
    assert np.array_equal(got, want)
    circ.free()


# ---- 6: public entry points ----------------------------------------------------------------------------------------------------------

def test_public_entry_points():
    code = make_code("steane")
    strata = code.logical_program_strata_exact('XXX', [0, 1, 2])
    assert isinstance(strata, montecarlo.PostSelectedStrata) and strata.fields == FT and strata.nb == 2584
    assert strata.series((1, 0, 0), 'wrong')[1] == 15 and strata.series((1, 1, 1), 'wrong')[1] == 5
    ec = code.error_correct_strata_exact([0, 1])
    classes, flipping = code.error_correct_single_faults()
    accepted = classes & ec_noise.CLASS_ACCEPTED != 0
    assert ec.fields == EC and int(ec.counts[0][0, 0, 0]) == 1
    assert [int(ec.counts[1][1, 0, 0]), int(ec.counts[1][0, 1, 0]), int(ec.counts[1][0, 0, 0])] == accepted.sum(axis=0).tolist()
    assert int(ec.counts[1][:, :, 0].sum()) == 390 and int(ec.counts[1][:, :, 3].sum()) == len(flipping)
    alone = montecarlo.enumerate_sharded(ec_noise.circuit_for(code, 1), [0, 1, 2])       # no process group: the one shard is the whole
    assert isinstance(alone, montecarlo.PostSelectedStrata) and alone.fields == EC
    assert all(np.array_equal(a, b) for a, b in zip(alone.counts, code.error_correct_strata_exact([0, 1, 2]).counts))


# ---- 7: refusals -----------------------------------------------------------------------------------------------------------------------

def test_refusals():
    code = make_code("steane")
    ctx = _native.default_context()
    circ, prog = ec_noise.circuit_for(code, 1), ft_noise.program_for(code, "")
    tables = circ._tables()
    # a circuit in the Monte-Carlo layout ([key_x: 2 words] [key_z: 2 words] [parity]: 5 words) is no cycle: its effects leave the layout
    rng = np.random.default_rng(SEED0 + 7)
    five = rng.integers(0, 1 << 62, (30, 2, 5)).astype("<u8")
    five[:, :, 4] &= np.uint64(3)
    five_dev = ctx.circuit_create(five)
    for rounds in (1, 2, 3):
        with pytest.raises(_native.GF2Error, match="beyond") as err:
            ctx.ec_enumerate(five_dev, rounds, *tables, 1, 0, 1)
        assert err.value.code == _native.GF2_E_ARG
    with pytest.raises(_native.GF2Error, match="8 <= ldr"):
        ctx.ft_enumerate(five_dev, 4, 0b0001, *tables, 1, 0, 1)
    five_dev.free()
    with pytest.raises(_native.GF2Error, match="8 <= ldr"):                  # the cycle's 3 words are no program
        ctx.ft_enumerate(circ.device(), 2, 0b01, *tables, 1, 0, 1)
    with pytest.raises(_native.GF2Error, match="ldr <= 8"):                  # a program of more than 8 words is no cycle
        ctx.ec_enumerate(ft_noise.program_for(code, "XXX").device(), 6, *tables, 1, 0, 1)
    with pytest.raises(_native.GF2Error, match="rounds need"):
        ctx.ec_enumerate(circ.device(), 2, *tables, 1, 0, 1)
    with pytest.raises(_native.GF2Error):                                    # the old enumeration still refuses more than 5 words
        ctx.circuit_enumerate(prog.device(), *tables, 1, 0, 1)
    for call in (lambda: circ.enumerate_strata([3], max_configurations=100), lambda: prog.enumerate_strata([2], max_configurations=10**6),
                 lambda: circ.enumerate_strata([9]), lambda: prog.enumerate_strata([1], first_rank=1585, count=1)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match="more than max_configurations"):
        prog.enumerate_strata([3])                                           # 1.8 x 10^10 configurations: beyond the default budget
    for w, first, count, text in ((9, 0, 1, "weight"), (2, 0, math.comb(330, 2) + 1, "leave"), (2, -1, 1, "leave")):
        with pytest.raises(_native.GF2Error, match=text):
            ctx.ec_enumerate(circ.device(), 1, *tables, w, first, count)
    assert not ctx.ec_enumerate(circ.device(), 1, *tables, 2, 100, 0).any()
    assert not ctx.ft_enumerate(prog.device(), prog.nsteps, prog.measure_mask, *tables, 2, 100, 0).any()
    assert ctx.ft_enumerate(prog.device(), prog.nsteps, prog.measure_mask, *tables, 2, 100, 0).shape == (3, 3, 7)
