"""
Malignant fault sets of the two post-selected gadgets on the GPU (DESIGN.md sections 5b "Malignant fault sets of the cycle" and 5c
"Malignant fault sets of the measurement"): gadget_list_kernel (csrc/gf2_gadget_list.hip) through gf2_ec_enumerate_list /
gf2_ft_enumerate_list, ECCircuit / FTProgram.malignant_faults and CSSCode.*_malignant_faults.  Every comparison is exact: the device's
records against the host statement's (gf2_ec_enumerate_list_host / gf2_ft_enumerate_list_host), byte for byte.

  instantiations  every (LDR, rule) of the kernel on the synthetic effect tables of tests/test_gpu_gadget_enumerate.py: 40 locations,
                  weights 0 .. 3, each whole and as a window from a third of the way in, `select` varied per case
  dense           no flag bit anywhere and select = 1: every lane of every wavefront emits, found = 3^w count
  single hit      a window with exactly one listed configuration
  odd counts      counts that are no multiple of 64 or of the run length
  launches        a range of three launches is the concatenation of single-launch parts; a window across a cut
  capacity        found with capacity 0 and found - 1; malignant_faults' second call
  real gadgets    the Steane cycle and the gate-free programs whole at weight 2 against the host statement, the committed literals and
                  the counting kernel; windows of Steane XXX up to 2^20 ranks deep inside weight 3
  entry points    CSSCode.*_malignant_faults; refusals; count 0

Every test runs under a time limit of its own, none provokes a fault.
"""
import concurrent.futures
import faulthandler
import math

import numpy as np
import pytest

from quantum_css_codes_amd import _native, ec_noise, ft_noise, montecarlo
from tests.test_fault_list import rederived_classes
from tests.test_gadget_enumerate import PAIR_COUNTS
from tests.test_gpu_gadget_enumerate import CYCLE_CASES, PROGRAM_CASES, synthetic_cycle, synthetic_program
from tests.test_gpu_strata import make_code

pytestmark = pytest.mark.gpu

SEED0 = 20261018 + 900
BUDGET = 1 << 40
TIME_LIMIT = 600                                                             # seconds per test
HOST_THREADS = 16
EC_FLIPS = ec_noise.CLASS_FLIP_X | ec_noise.CLASS_FLIP_Z
EC_SELECTS = (1, ec_noise.CLASS_FLIP_X, ec_noise.CLASS_FLIP_Z, EC_FLIPS, ec_noise.CLASS_UNCORRECTABLE_X, ec_noise.CLASS_UNCORRECTABLE_Z, 0x1f, 0x1e)
FT_SELECTS = (1, ft_noise.CLASS_WRONG, ft_noise.CLASS_FIRST_TRIAL_WRONG, ft_noise.CLASS_SPLIT_VOTE, ft_noise.CLASS_UNMATCHED_X,
              ft_noise.CLASS_UNMATCHED_Z, 0x3f, 0x3e, ft_noise.CLASS_WRONG | ft_noise.CLASS_SPLIT_VOTE)


@pytest.fixture(autouse=True)
def own_time_limit():
    faulthandler.dump_traceback_later(TIME_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def cycle(rounds):
    return ec_noise.circuit_for(make_code("steane"), rounds)


def program(name, ops):
    return ft_noise.program_for(make_code(name), ops)


def both(gadget, w, select, first=None, count=None):
    """(device list, host list) of a gadget through malignant_faults."""
    return tuple(gadget.malignant_faults(w, select=select, first_rank=first, count=count, max_configurations=BUDGET, host=host) for host in (False, True))


def same(device, host):
    return device.records.dtype == np.uint64 and device.ranges == host.ranges and np.array_equal(device.records, host.records)


def exact(list_fn, w, first, count, select):
    """The records of list_fn(w, first, count, select, capacity) -> (found, records or None): counted first, then fetched with exactly
    `found` records of room."""
    found, none = list_fn(w, first, count, select, 0)
    assert none is None or found == 0
    got, records = list_fn(w, first, count, select, found)
    assert got == found and records is not None and records.shape == (found, 2)
    return records


# ---- 1: every instantiation on synthetic effect tables -----------------------------------------------------------------------------

def check_synthetic(device_fn, host_fn, locations, select):
    """Weights 0 .. 3, each whole and as a window from a third of the way in, device against host, record for record."""
    listed = 0
    for w in range(4):
        total = math.comb(locations, w)
        third = total // 3
        for first, count in ((0, total), (third, total - third)):
            want = exact(host_fn, w, first, count, select)
            assert np.array_equal(exact(device_fn, w, first, count, select), want), (w, first, count, select)
            found, records = device_fn(w, first, count, select, 1 << 16)      # room to spare: the same list
            assert found == len(want) and (np.array_equal(records, want) if found <= 1 << 16 else records is None)
        listed += len(want)
    return listed


@pytest.mark.parametrize("case", CYCLE_CASES, ids=lambda c: "rounds%d-ldr%d" % (c[0], 1 + c[0] + c[1]))
def test_every_cycle_instantiation(case):
    rounds, nflag = case
    ctx = _native.default_context()
    rng = np.random.default_rng(SEED0 + 16 * rounds + nflag)
    r1, r2 = 5, 4
    eff, tables = synthetic_cycle(rng, r1, r2, rounds, nflag, 40)
    circ = ctx.circuit_create(eff)
    args = (rounds, r1, tables[0], tables[1], r2, tables[2], tables[3])
    listed = 0
    for select in (EC_SELECTS[CYCLE_CASES.index(case) % len(EC_SELECTS)], 1):
        listed += check_synthetic(lambda *tail: ctx.ec_enumerate_list(circ, *args, *tail),
                                  lambda *tail: _native.ec_enumerate_list_host(eff, *args, *tail), 40, select)
    assert listed > 64, case
    circ.free()


@pytest.mark.parametrize("case", PROGRAM_CASES, ids=lambda c: "steps%d-ldr%d" % (c[0], c[0] + c[2]))
def test_every_measurement_instantiation(case):
    nsteps, mask, nflag = case
    ctx = _native.default_context()
    rng = np.random.default_rng(SEED0 + 32 * nsteps + nflag)
    r1, r2 = 4, 5
    eff, tables = synthetic_program(rng, r1, r2, nsteps, mask, nflag, 40)
    circ = ctx.ft_circuit_create(eff)
    args = (nsteps, mask, r1, tables[0], tables[1], r2, tables[2], tables[3])
    listed = 0
    for select in (FT_SELECTS[1 + PROGRAM_CASES.index(case) % (len(FT_SELECTS) - 1)], 1):
        listed += check_synthetic(lambda *tail: ctx.ft_enumerate_list(circ, *args, *tail),
                                  lambda *tail: _native.ft_enumerate_list_host(eff, *args, *tail), 40, select)
    assert listed > 64, case
    circ.free()


def test_cases_cover_the_kernel_instantiations():
    assert {1 + r + f for r, f in CYCLE_CASES} == set(range(3, 9)) and {s + f for s, _, f in PROGRAM_CASES} == set(range(8, ft_noise.MAX_LDR + 1))


# ---- 2: dense emission ----------------------------------------------------------------------------------------------------------------

def test_dense_emission_fills_every_slot():
    """No effect sets a flag bit, so every configuration is accepted, and select = 1 lists them all: every lane of every wavefront
    emits in every trip, the ballots are full (but for the tail), and the slots must tile [0, found) exactly."""
    ctx = _native.default_context()
    rng = np.random.default_rng(SEED0 + 2)
    eff, tables = synthetic_cycle(rng, 5, 4, 2, 1, 40)
    eff[:, :, 3:] = 0
    circ = ctx.circuit_create(eff)
    args = (2, 5, tables[0], tables[1], 4, tables[2], tables[3])
    device_fn = lambda *tail: ctx.ec_enumerate_list(circ, *args, *tail)
    host_fn = lambda *tail: _native.ec_enumerate_list_host(eff, *args, *tail)
    for w, first, count in ((3, 0, math.comb(40, 3)), (2, 0, math.comb(40, 2)), (2, 7, 64), (2, 9, 65), (3, 1234, 4097), (1, 0, 40), (0, 0, 1)):
        got = exact(device_fn, w, first, count, 1)
        assert len(got) == 3**w * count, (w, first, count)
        assert np.array_equal(got, exact(host_fn, w, first, count, 1)), (w, first, count)
        assert np.array_equal(got[:, 0], np.repeat(np.arange(first, first + count, dtype=np.uint64), 3**w))
        assert np.array_equal(got[:, 1] & np.uint64(0xFFFF), np.tile(np.arange(3**w, dtype=np.uint64), count))
    circ.free()
    eff, tables = synthetic_program(rng, 4, 5, 7, 0b0010101, 1, 40)
    eff[:, :, 7:] = 0
    circ = ctx.ft_circuit_create(eff)
    args = (7, 0b0010101, 4, tables[0], tables[1], 5, tables[2], tables[3])
    got = exact(lambda *tail: ctx.ft_enumerate_list(circ, *args, *tail), 3, 0, math.comb(40, 3), 1)
    assert len(got) == 27 * math.comb(40, 3)
    assert np.array_equal(got, exact(lambda *tail: _native.ft_enumerate_list_host(eff, *args, *tail), 3, 0, math.comb(40, 3), 1))
    circ.free()


# ---- 3, 4: a single hit; counts that are no multiple of 64 or of the run length ------------------------------------------------------------

def test_a_window_with_a_single_hit():
    circ = cycle(1)
    whole = circ.malignant_faults(2, select=EC_FLIPS, host=True)
    ranks = whole.ranks.astype(np.int64)
    gaps = np.minimum(np.diff(ranks)[:-1], np.diff(ranks)[1:])                # to the nearest listed rank on either side
    i, gap = int(np.argmax(gaps)) + 1, int(gaps.max())                       # the most isolated record
    assert gap >= 50
    for first, count in ((int(ranks[i]) - gap + 1, 2 * gap - 1), (int(ranks[i]), 1), (int(ranks[i]) - gap + 1, gap)):
        device, host = both(circ, 2, EC_FLIPS, first, count)
        assert len(device) == 1 and same(device, host), (first, count)
        assert int(device.ranks[0]) == int(ranks[i]) and int(device.kind_codes[0]) == int(whole.kind_codes[i])
        assert device.locations().tolist() == whole.locations()[i:i + 1].tolist() and device.kinds().tolist() == whole.kinds()[i:i + 1].tolist()
        assert int(device.classes[0]) == int(whole.classes[i])


def test_windows_of_the_measurement():
    prog = program("steane", "XXX")
    L = prog.num_locations
    assert (L, prog.ldr) == (2584, 11)
    total = math.comb(L, 2)
    listed = 0
    for k, (first, count) in enumerate(((0, 1), (12345, 4097), (77, 257), (33, 31), (5, 63), (6, 65), (total - 1000, 1000), (total // 2 + 13, 100003))):
        select = FT_SELECTS[k % len(FT_SELECTS)]
        device, host = both(prog, 2, select, first, count)
        assert same(device, host), (first, count, select)
        listed += len(device)
    assert listed > 1000
    total = math.comb(L, 3)
    first = total // 2 + 987654321 % 1000003                                 # 2^20 + 77 ranks deep inside weight 3: runs of two ranks,
    count = (1 << 20) + 77                                                   # the last lane's run cut short
    assert count // (2048 * 256) == 2 and count % 2 == 1
    for select in (ft_noise.CLASS_WRONG, ft_noise.CLASS_SPLIT_VOTE | ft_noise.CLASS_FIRST_TRIAL_WRONG):
        device, host = both(prog, 3, select, first, count)
        assert same(device, host) and len(device) > 0, select
    cuts = [0, 1, 1234567, math.comb(L, 2)]
    parts = [prog.malignant_faults(2, first_rank=lo, count=hi - lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
    whole = prog.malignant_faults(2)
    assert np.array_equal((parts[0] + parts[1] + parts[2]).records, whole.records) and len(whole) > 0


# ---- 5: several launches -----------------------------------------------------------------------------------------------------------------

def test_a_range_of_several_launches_is_the_concatenation_of_its_parts():
    """A launch covers 2^28 configurations: 40 913 subsets of weight 8.  120 000 subsets of a synthetic 21-location cycle are three
    launches, through which the counter runs on and the ranks stay absolute: the list of the whole is the concatenation of three
    unequal parts of one launch each, and a window across the first cut is the host statement's.  A quarter of these configurations
    is accepted, and with a table of half the keys every class bit is set in half of those; so the syndrome tables here hold every
    key but one of the z side, and the whole is listed for the class that needs it (3 % of the configurations)."""
    ctx = _native.default_context()
    rng = np.random.default_rng(20261018 + 500 + 5)                          # the effect table of the counting kernel's test
    eff, _ = synthetic_cycle(rng, 3, 3, 1, 1, 21)
    circ = ctx.circuit_create(eff)
    keys_z, keys_x = np.array([0, 1, 2, 3, 4, 6, 7], dtype="<u8"), np.arange(8, dtype="<u8")
    args = (1, 3, keys_z, rng.integers(0, 2, 7, dtype=np.uint8), 3, keys_x, rng.integers(0, 2, 8, dtype=np.uint8))
    sparse = ec_noise.CLASS_UNCORRECTABLE_Z
    device_fn = lambda *tail: ctx.ec_enumerate_list(circ, *args, *tail)
    per_launch = (1 << 28) // 3**8
    assert per_launch == 40913 and 120000 <= math.comb(21, 8) and 2 * per_launch < 120000
    found, none = device_fn(8, 0, 120000, sparse, 0)                       # counted: one pass over the three launches
    assert none is None and 0 < found < 3**8 * 120000
    cuts = [0, 40000, 80001, 120000]
    parts = [device_fn(8, lo, hi - lo, sparse, found) for lo, hi in zip(cuts[:-1], cuts[1:])]     # one launch each, room to spare
    assert sum(n for n, _ in parts) == found and all(len(records) == n > 0 for n, records in parts)
    got, whole = device_fn(8, 0, 120000, sparse, found)                    # listed: exactly enough room
    assert got == found and np.array_equal(np.concatenate([records for _, records in parts]), whole)
    assert int(whole[:, 0].max()) > 2 * per_launch and int(whole[:, 0].min()) < per_launch
    lo, count = per_launch - 300, 700                                        # across the first cut, 4.6 x 10^6 configurations on the host:
    edges = [lo + count * k // HOST_THREADS for k in range(HOST_THREADS + 1)]    # in pieces (the lists of disjoint ranges concatenate)
    piece = lambda a_b: _native.ec_enumerate_list_host(eff, *args, 8, a_b[0], a_b[1] - a_b[0], 1, 3**8 * (a_b[1] - a_b[0]))[1]
    with concurrent.futures.ThreadPoolExecutor(HOST_THREADS) as pool:
        want = np.concatenate(list(pool.map(piece, zip(edges[:-1], edges[1:]))))
    got, window = device_fn(8, lo, count, 1, len(want))
    assert got == len(want) > 0 and np.array_equal(window, want)
    assert np.array_equal(whole[(whole[:, 0] >= lo) & (whole[:, 0] < lo + count)], want[((want[:, 1] >> np.uint64(32)) & np.uint64(sparse)) != 0])
    circ.free()


# ---- 6: capacity ---------------------------------------------------------------------------------------------------------------------------

def test_capacity():
    circ = cycle(1)
    ctx = _native.default_context()
    tables = circ._tables()
    total = math.comb(330, 2)
    want = circ.malignant_faults(2, select=EC_FLIPS, host=True)
    found = len(want)
    assert found == 10263
    for capacity in (0, 1, found - 1):
        assert ctx.ec_enumerate_list(circ.device(), 1, *tables, 2, 0, total, EC_FLIPS, capacity) == (found, None), capacity
    for capacity in (found, found + 1, 1 << 20):
        got, records = ctx.ec_enumerate_list(circ.device(), 1, *tables, 2, 0, total, EC_FLIPS, capacity)
        assert got == found and np.array_equal(records, want.records), capacity
    device, host = both(circ, 2, 1)                                          # more than the first call's 2^16 records: the second call
    assert len(device) > montecarlo.FAULT_LIST_FIRST_CAPACITY and same(device, host)
    assert len(device) == int(circ.enumerate_strata([2]).counts[0][:, :, 0].sum())


# ---- 7: the real gadgets ----------------------------------------------------------------------------------------------------------------------

def test_one_round_of_the_steane_cycle():
    circ = cycle(1)
    assert circ.ldr == 3 and 9 * math.comb(330, 2) + 3 * 330 == 488565 + 990
    for w in (0, 1, 2):
        for select in (EC_FLIPS, 0x1e):
            device, host = both(circ, w, select)
            assert same(device, host), (w, select)
    device = circ.malignant_faults(2)                                        # the default select: the logical flips
    assert len(device) == 10263 and np.array_equal(rederived_classes(circ, device), device.classes)
    counts = circ.enumerate_strata([2]).counts[0]
    assert device.composition_counts().tolist() == counts[:, :, 3].tolist()
    assert device.composition_counts(ec_noise.CLASS_FLIP_X).tolist() == counts[:, :, 1].tolist()
    assert device.coefficient((1, 1, 1)) == circ.enumerate_strata([2]).coefficients((1, 1, 1), 'logical_any')[0]
    assert circ.describe(circ.malignant_faults(1)) == [(fault,) for fault in circ.single_faults()[1]]
    two = cycle(2)
    device, host = both(two, 2, EC_FLIPS)
    assert same(device, host) and len(device) > 2 * 10263


@pytest.mark.parametrize("name, found", [("steane", 37095), ("rm15", 5535)])
def test_weight_2_of_the_gate_free_programs(name, found):
    prog = program(name, "")
    got = prog.malignant_faults(2)                                           # 11.3 and 67.3 million configurations
    assert len(got) == found and got.ranges == ((0, math.comb(prog.num_locations, 2)),)
    assert got.composition_counts(ft_noise.CLASS_WRONG).tolist() == PAIR_COUNTS[name]['wrong']
    strata = prog.enumerate_strata([2])                                      # the counting kernel, in the same process
    assert int(strata.counts[0][:, :, 1].sum()) == found
    assert got.coefficient((1, 1, 1), ft_noise.CLASS_WRONG) == strata.coefficients((1, 1, 1), 'wrong')[0]
    assert np.array_equal(rederived_classes(prog, got), got.classes)
    assert ((got.classes & 1 != 0) & (got.classes & ft_noise.CLASS_WRONG != 0)).all()
    if name == "steane":
        assert same(got, prog.malignant_faults(2, host=True))
    else:
        assert got.coefficient((1, 1, 1)) == 615
        unmatched = prog.malignant_faults(2, select=ft_noise.CLASS_UNMATCHED_X, first_rank=2000000, count=30001)
        assert same(unmatched, prog.malignant_faults(2, select=ft_noise.CLASS_UNMATCHED_X, first_rank=2000000, count=30001, host=True)) and len(unmatched) > 0


# ---- 8: public entry points and refusals -----------------------------------------------------------------------------------------------------

def test_public_entry_points():
    code = make_code("steane")
    wrong = code.logical_program_malignant_faults('XXX', 1)
    prog = ft_noise.program_for(code, 'XXX')
    assert isinstance(wrong, montecarlo.FaultList) and (wrong.nb, wrong.weight, len(wrong)) == (2584, 1, 15)
    assert prog.describe(wrong) == [(fault,) for fault in code.logical_program_single_faults('XXX')[1]]
    assert wrong.class_names == ft_noise.CLASS_NAMES and wrong.coefficient((1, 0, 0)) == 15
    flips = code.error_correct_malignant_faults(2, rounds=1, select=ec_noise.CLASS_FLIP_Z, first_rank=1000, count=20000)
    assert same(flips, ec_noise.circuit_for(code, 1).malignant_faults(2, select=ec_noise.CLASS_FLIP_Z, first_rank=1000, count=20000, host=True))
    assert flips.class_names == ec_noise.CLASS_NAMES and flips.ranges == ((1000, 20000),)
    empty = code.error_correct_malignant_faults(2, first_rank=100, count=0)
    assert len(empty) == 0 and empty.ranges == ((100, 0),) and empty.locations().shape == (0, 2)


def test_refusals():
    code = make_code("steane")
    ctx = _native.default_context()
    circ, prog = ec_noise.circuit_for(code, 1), ft_noise.program_for(code, "")
    tables = circ._tables()
    ec = lambda dev=None, rounds=1, w=1, first=0, count=1, select=1, capacity=8: \
        ctx.ec_enumerate_list(circ.device() if dev is None else dev, rounds, *tables, w, first, count, select, capacity)
    ft = lambda dev=None, nsteps=prog.nsteps, mask=prog.measure_mask, w=1, first=0, count=1, select=1, capacity=8: \
        ctx.ft_enumerate_list(prog.device() if dev is None else dev, nsteps, mask, *tables, w, first, count, select, capacity)
    # a circuit in the Monte-Carlo layout ([key_x: 2 words] [key_z: 2 words] [parity]: 5 words) is no cycle: its effects leave the layout
    rng = np.random.default_rng(SEED0 + 7)
    five = rng.integers(0, 1 << 62, (30, 2, 5)).astype("<u8")
    five[:, :, 4] &= np.uint64(3)
    five_dev = ctx.circuit_create(five)
    xxx = ft_noise.program_for(code, "XXX").device()
    for call, text in ((lambda: ec(five_dev, rounds=1), "beyond"), (lambda: ec(five_dev, rounds=3), "beyond"), (lambda: ft(five_dev, nsteps=4, mask=1), "8 <= ldr"),
                       (lambda: ft(circ.device(), nsteps=2, mask=1), "8 <= ldr"), (lambda: ec(xxx, rounds=6), "ldr <= 8"), (lambda: ec(rounds=2), "rounds need"),
                       (lambda: ec(rounds=0), "rounds"), (lambda: ft(mask=0b010100), "odd number"), (lambda: ft(mask=1 << 6), "at or above nsteps"),
                       (lambda: ft(nsteps=8), "F >= 1"),
                       (lambda: ec(select=0), "select"), (lambda: ec(select=0x20), "class bits"), (lambda: ft(select=0), "select"),
                       (lambda: ft(select=0x40), "class bits"), (lambda: ec(capacity=-1), "capacity"), (lambda: ft(capacity=-1), "capacity"),
                       (lambda: ec(capacity=(1 << 28) + 1), "2\\^28"), (lambda: ft(capacity=(1 << 28) + 1), "2\\^28"),
                       (lambda: ec(w=9), "weight"), (lambda: ec(w=2, count=math.comb(330, 2) + 1), "leave"), (lambda: ec(w=2, first=-1), "leave"),
                       (lambda: ft(w=2, first=math.comb(1585, 2)), "leave")):
        with pytest.raises(_native.GF2Error, match=text) as err:
            call()
        assert err.value.code == _native.GF2_E_ARG, text
    five_dev.free()
    for call in (lambda: circ.malignant_faults(3, max_configurations=100), lambda: prog.malignant_faults(2, max_configurations=10**6),
                 lambda: circ.malignant_faults(9), lambda: prog.malignant_faults(1, first_rank=1585, count=1), lambda: circ.malignant_faults(1, select=0),
                 lambda: prog.malignant_faults(1, select=0x40)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match="more than max_configurations"):
        prog.malignant_faults(3)                                             # 1.8 x 10^10 configurations: beyond the default budget
    found, records = ec(w=2, first=100, count=0)
    assert found == 0 and records.shape == (0, 2)
    found, records = ft(w=2, first=100, count=0, capacity=0)
    assert found == 0 and records.shape == (0, 2)
    assert ec(select=1, capacity=0) == (1, None)                             # counted, not stored
