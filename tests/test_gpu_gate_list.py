"""
Malignant fault sets under gate-level faults on the GPU (DESIGN.md section 5e "Malignant fault sets under gate-level faults"):
gate_list_kernel (csrc/gf2_gate_list.hip) through gf2_ec_gate_enumerate_list / gf2_ft_gate_enumerate_list, ECCircuit /
FTProgram.malignant_gate_faults and CSSCode.*_malignant_gate_faults.  Every comparison is exact: the device's records against the
host statement's byte for byte, or their counts against the counting kernel's (gate_enumerate_kernel, unchanged).

  instantiations  every (LDR, rule) of the kernel on synthetic effect tables with a mixed site table, windows of (2, 1) and (3, 2)
  dense emission  no flag bits and select = accepted: every lane of every trip lists, the slots tile [0, found)
  sparse          a window with a single hit, and one with none
  windows         odd counts, first ranks off every run boundary, a wrap of the one-operand part inside a run, the last ranks, (4, 4)
  launches        a window of (4, 4) of two launches is the concatenation of its halves; its counts are the counting kernel's
  capacity        0, one too few, exact, three more; a buffer too small is left as it was
  real gadgets    whole weight 2 of the one-round cycle (every b) against the host; two program strata against the counting kernel
  state           the same call twice with another call in between, into a buffer that was filled before
  entry points    CSSCode.*_malignant_gate_faults; refusals

The host statement is serial; a large range is handed to it in pieces on a few threads (ctypes releases the interpreter lock, the
lists of disjoint ranges concatenate).  Every test runs under a time limit of its own, none provokes a fault.
"""
import concurrent.futures
import faulthandler
import math

import numpy as np
import pytest

from quantum_css_codes_amd import _native, ec_noise, ft_noise, montecarlo
from tests.state_check import FILL
from tests.test_gpu_gadget_enumerate import CYCLE_CASES, PROGRAM_CASES, synthetic_cycle, synthetic_program
from tests.test_gpu_gate_enumerate import mixed_sites
from tests.test_gpu_strata import make_code

pytestmark = pytest.mark.gpu

SEED0 = 20261020 + 700
BUDGET = 1 << 40
TIME_LIMIT = 300                                                             # seconds per test
HOST_THREADS = 16
EC, FT = ec_noise.EC_FIELDS, ft_noise.FT_FIELDS
EC_ALL, FT_ALL = 0x1F, 0x3F
EC_FLIPS = ec_noise.CLASS_FLIP_X | ec_noise.CLASS_FLIP_Z
# the class bits (or unions of them) that one indicator field of the tally counts: mask -> field
EC_FIELD_OF_MASK = {1: 'accepted', 2: 'logical_x', 4: 'logical_z', 6: 'logical_any', 8: 'uncorrectable_x', 16: 'uncorrectable_z'}
FT_FIELD_OF_MASK = {1: 'accepted', 2: 'wrong', 4: 'first_trial_wrong', 8: 'split_vote'}


@pytest.fixture(autouse=True)
def own_time_limit():
    faulthandler.dump_traceback_later(TIME_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def cycle(rounds):
    return ec_noise.circuit_for(make_code("steane"), rounds)


def program(name, ops):
    return ft_noise.program_for(make_code(name), ops)


def total(gadget, w, b):
    _, n1, n2, _ = gadget.gate_sites()
    return math.comb(n1, w - b) * math.comb(n2, b)


def exact(list_fn, w, b, first, count, select):
    """The records of list_fn(w, b, first, count, select, capacity) -> (found, records or None): counted first, then fetched with
    exactly `found` records of room."""
    found, none = list_fn(w, b, first, count, select, 0)
    assert none is None or found == 0
    got, records = list_fn(w, b, first, count, select, found)
    assert got == found and records is not None and records.shape == (found, 2)
    return records


def in_pieces(host_fn, w, b, first, count, select):
    """exact(host_fn, ...) over up to HOST_THREADS pieces of the range, one thread each, concatenated."""
    if count < 4096:
        return exact(host_fn, w, b, first, count, select)
    cuts = [first + count * k // HOST_THREADS for k in range(HOST_THREADS + 1)]
    with concurrent.futures.ThreadPoolExecutor(HOST_THREADS) as pool:
        parts = list(pool.map(lambda lo_hi: exact(host_fn, w, b, lo_hi[0], lo_hi[1] - lo_hi[0], select), zip(cuts[:-1], cuts[1:])))
    return np.concatenate(parts)


def entries(gadget):
    """(device_fn, host_fn) of a real gadget, both (w, b, first, count, select, capacity) -> (found, records or None)."""
    sites = gadget.gate_sites()[:3]
    device_entry, host_entry = gadget._entry("%s_gate_enumerate_list"), gadget._entry("%s_gate_enumerate_list", host=True)
    return (lambda *tail: device_entry(*sites, *tail)), (lambda *tail: host_entry(*sites, *tail))


def same(got, want):
    return got.dtype == want.dtype == np.uint64 and got.shape == want.shape and got.tobytes() == want.tobytes()


def counts_of(records, a, b, mask):
    """[c]: the records with a class bit of `mask` per number of two-operand kinds among the b CNOT picks (the nibbles from a on)."""
    kappa = ((records[:, 1][:, None] >> (np.uint64(4) * np.arange(a, a + b, dtype=np.uint64))) & np.uint64(15)).astype(np.int64).reshape(len(records), b)
    c = (((kappa & 3) != 0) & ((kappa >> 2) != 0)).sum(axis=1)
    hit = ((records[:, 1] >> np.uint64(32)) & np.uint64(mask)) != 0
    return np.bincount(c[hit], minlength=b + 1)


# ---- 1: every instantiation on synthetic effect tables --------------------------------------------------------------------------------

def check_synthetic(device_fn, host_fn, sites, select):
    """A window of a few thousand ranks of (2, 1) and of a few hundred of (3, 2), device against host, byte for byte."""
    _, n1, n2 = sites
    listed = 0
    for w, b, first, count in ((2, 1, 2 * n1 - 77, 3001), (3, 2, 5 * n1 - 40, 301)):
        assert first + count <= math.comb(n1, w - b) * math.comb(n2, b)
        for sel in (select, 1):
            want = exact(host_fn, w, b, first, count, sel)
            assert same(exact(device_fn, w, b, first, count, sel), want), (w, b, sel)
            found, records = device_fn(w, b, first, count, sel, 1 << 16)       # room to spare: the same list
            assert found == len(want) and (same(records, want) if found <= 1 << 16 else records is None)
            listed += len(want)
    return listed


@pytest.mark.parametrize("case", CYCLE_CASES, ids=lambda c: "rounds%d-ldr%d" % (c[0], 1 + c[0] + c[1]))
def test_every_cycle_instantiation(case):
    rounds, nflag = case
    ctx = _native.default_context()
    rng = np.random.default_rng(SEED0 + 16 * rounds + nflag)
    r1, r2 = 5, 4
    eff, tables = synthetic_cycle(rng, r1, r2, rounds, nflag, 500)
    sites = mixed_sites(rng, 500)
    assert min(sites[1:]) >= 100
    circ = ctx.circuit_create(eff)
    args = (rounds, r1, tables[0], tables[1], r2, tables[2], tables[3]) + sites
    select = (EC_FLIPS, 2, 4, 8, 16, 0x1e)[CYCLE_CASES.index(case) % 6]
    listed = check_synthetic(lambda *tail: ctx.ec_gate_enumerate_list(circ, *args, *tail),
                             lambda *tail: _native.ec_gate_enumerate_list_host(eff, *args, *tail), sites, select)
    assert listed > 64, case
    circ.free()


@pytest.mark.parametrize("case", PROGRAM_CASES, ids=lambda c: "steps%d-ldr%d" % (c[0], c[0] + c[2]))
def test_every_measurement_instantiation(case):
    nsteps, mask, nflag = case
    ctx = _native.default_context()
    rng = np.random.default_rng(SEED0 + 32 * nsteps + nflag)
    r1, r2 = 4, 5
    eff, tables = synthetic_program(rng, r1, r2, nsteps, mask, nflag, 300)
    sites = mixed_sites(rng, 300)
    assert min(sites[1:]) >= 60
    circ = ctx.ft_circuit_create(eff)
    args = (nsteps, mask, r1, tables[0], tables[1], r2, tables[2], tables[3]) + sites
    select = (2, 4, 8, 16, 32, 0x3e, 0x0a)[PROGRAM_CASES.index(case) % 7]
    listed = check_synthetic(lambda *tail: ctx.ft_gate_enumerate_list(circ, *args, *tail),
                             lambda *tail: _native.ft_gate_enumerate_list_host(eff, *args, *tail), sites, select)
    assert listed > 64, case
    circ.free()


# ---- 2: dense emission ----------------------------------------------------------------------------------------------------------------

def test_dense_emission_fills_every_slot():
    """No effect sets a flag bit, so every configuration is accepted, and select = 1 lists them all: every lane of every wavefront
    emits in every trip, the ballots are full (but for the tail), and the slots must tile [0, found) exactly."""
    ctx = _native.default_context()
    rng = np.random.default_rng(SEED0 + 2)
    eff, tables = synthetic_cycle(rng, 5, 4, 2, 1, 80)
    eff[:, :, 3:] = 0
    sites = mixed_sites(rng, 80)
    _, n1, n2 = sites
    assert min(n1, n2) >= 20
    circ = ctx.circuit_create(eff)
    args = (2, 5, tables[0], tables[1], 4, tables[2], tables[3]) + sites
    device_fn = lambda *tail: ctx.ec_gate_enumerate_list(circ, *args, *tail)
    host_fn = lambda *tail: _native.ec_gate_enumerate_list_host(eff, *args, *tail)
    for w, b, first, count in ((2, 1, 0, n1 * n2), (2, 2, 0, math.comb(n2, 2)), (2, 0, 7, 64), (2, 1, 9, 65), (3, 1, 123, 409), (3, 3, 5, 33),
                               (1, 1, 0, n2), (1, 0, 0, n1), (0, 0, 0, 1)):
        kinds = 3**(w - b) * 15**b
        got = exact(device_fn, w, b, first, count, 1)
        assert len(got) == kinds * count, (w, b, first, count)
        assert same(got, exact(host_fn, w, b, first, count, 1)), (w, b, first, count)
        assert np.array_equal(got[:, 0], np.repeat(np.arange(first, first + count, dtype=np.uint64), kinds))
    circ.free()
    eff, tables = synthetic_program(rng, 4, 5, 7, 0b0010101, 1, 80)
    eff[:, :, 7:] = 0
    circ = ctx.ft_circuit_create(eff)
    args = (7, 0b0010101, 4, tables[0], tables[1], 5, tables[2], tables[3]) + sites
    got = exact(lambda *tail: ctx.ft_gate_enumerate_list(circ, *args, *tail), 2, 1, 0, n1 * n2, 1)
    assert len(got) == 45 * n1 * n2
    assert same(got, exact(lambda *tail: _native.ft_gate_enumerate_list_host(eff, *args, *tail), 2, 1, 0, n1 * n2, 1))
    circ.free()


# ---- 3: a single hit, and none ------------------------------------------------------------------------------------------------------------

def test_windows_with_a_single_hit_and_with_none():
    """The flips of the cycle come in clusters (several kinds of one pair of gates, neighbouring pairs); of the X flips of two CNOTs
    52 pairs are listed once, the most isolated of them three ranks from the next listed pair."""
    circ = cycle(1)
    device_fn, host_fn = entries(circ)
    select = ec_noise.CLASS_FLIP_X
    _, whole = host_fn(2, 2, 0, total(circ, 2, 2), select, 1 << 16)
    ranks = whole[:, 0].astype(np.int64)
    before, after = np.diff(ranks, prepend=-1 << 40), np.diff(ranks, append=1 << 40)
    alone = np.flatnonzero((before > 0) & (after > 0))                        # ranks listed once
    gaps = np.minimum(before, after)[alone]
    i, gap = int(alone[np.argmax(gaps)]), int(gaps.max())                     # the most isolated record
    assert gap >= 3
    r = int(ranks[i])
    for first, count in ((r - gap + 1, 2 * gap - 1), (r, 1), (r - gap + 1, gap), (r, gap)):
        found, got = device_fn(2, 2, first, count, select, 8)
        assert found == 1 and same(got, np.ascontiguousarray(whole[i:i + 1])), (first, count)
    j = int(np.argmax(after[:-1]))                                            # the widest stretch of ranks with nothing to list
    empty = (int(ranks[j]) + 1, int(after[j]) - 1)
    assert empty[1] >= 64
    for first, count in ((r - gap + 1, gap - 1), (r + 1, gap - 1), empty):
        found, got = device_fn(2, 2, first, count, select, 8)
        assert found == 0 and got.shape == (0, 2), (first, count)
        assert host_fn(2, 2, first, count, select, 8)[0] == 0


# ---- 4: windows ------------------------------------------------------------------------------------------------------------------------

def test_windows_of_the_measurement():
    prog = program("steane", "XXX")
    device_fn, host_fn = entries(prog)
    _, n1, n2, _ = prog.gate_sites()
    assert (n1, n2, prog.ldr) == (990, 797, 11)
    c1 = n1                                                                  # (2, 1): C(n_1, 1) one-operand subsets per CNOT
    listed = 0
    selects = (ft_noise.CLASS_WRONG, 1, 0x3e, ft_noise.CLASS_SPLIT_VOTE, FT_ALL)
    for k, (b, first, count) in enumerate(((1, 0, 1), (1, 12345, 4097), (1, 77, 257), (1, 33, 31), (1, 5 * c1 - 3, 7), (1, 7 * c1 - 1, 2),
                                           (1, total(prog, 2, 1) - 1000, 1000), (0, total(prog, 2, 0) - 777, 777), (2, 99, 10001),
                                           (2, total(prog, 2, 2) - 1, 1))):
        select = selects[k % len(selects)]
        want = in_pieces(host_fn, 2, b, first, count, select)
        assert same(exact(device_fn, 2, b, first, count, select), want), (b, first, count, select)
        listed += len(want)
    assert listed > 1000
    # runs of two ranks per lane, the one-operand part wrapping inside runs: 2^20 + 4097 subsets of (3, 1) from just below a wrap
    c1 = math.comb(n1, 2)
    first, count = 5 * c1 - 1001, (1 << 20) + 4097
    assert count // (2048 * 256) == 2 and count > 2 * c1
    want = in_pieces(host_fn, 3, 1, first, count, ft_noise.CLASS_WRONG)
    assert len(want) > 0 and same(exact(device_fn, 3, 1, first, count, ft_noise.CLASS_WRONG), want)
    # weight 4: 2 001 subsets of (4, 2) across a wrap, 2 025 kinds each, and the last 40 of (4, 4), 50 625 kinds each
    first = 3 * c1 - 1000
    want = in_pieces(host_fn, 4, 2, first, 2001, 0x3e)
    assert same(exact(device_fn, 4, 2, first, 2001, 0x3e), want)
    first = total(prog, 4, 4) - 40
    want = in_pieces(host_fn, 4, 4, first, 40, 0x3e)
    assert same(exact(device_fn, 4, 4, first, 40, 0x3e), want) and (len(want) == 0 or int(want[-1, 0]) < total(prog, 4, 4))


# ---- 5: several launches -----------------------------------------------------------------------------------------------------------------

def test_a_range_of_two_launches_is_the_concatenation_of_its_halves():
    """A launch covers 2^28 configurations: 5 302 subsets of (4, 4), 50 625 kinds each.  6 000 subsets of the one-round cycle are two
    launches, through which the counter runs on and the ranks stay absolute."""
    circ = cycle(1)
    device_fn, host_fn = entries(circ)
    per_launch = (1 << 28) // 15**4
    first, count = total(circ, 4, 4) // 2 + 4321, 6000
    assert per_launch == 5302 < count <= 2 * per_launch
    select = 0x1e                                                            # a flip or an uncorrectable final syndrome
    whole = exact(device_fn, 4, 4, first, count, select)
    halves = [exact(device_fn, 4, 4, lo, n, select) for lo, n in ((first, 3000), (first + 3000, 3000))]
    assert len(halves[0]) > 0 and len(halves[1]) > 0 and same(np.concatenate(halves), whole)
    assert int(whole[:, 0].min()) < first + per_launch <= int(whole[:, 0].max()) and int(whole[:, 0].max()) < first + count
    counts = circ.enumerate_gate_range(4, 4, first, count)                   # the counting kernel, unchanged
    for mask in (2, 4, 6, 8, 16):
        assert counts_of(whole, 0, 4, mask).tolist() == counts[:, EC.index(EC_FIELD_OF_MASK[mask])].astype(np.int64).tolist(), mask
    for lo, n in ((first + per_launch - 3, 3), (first + per_launch, 3), (first + per_launch - 2, 5)):       # on either side of the cut, across it
        want = exact(host_fn, 4, 4, lo, n, select)
        assert same(exact(device_fn, 4, 4, lo, n, select), want), (lo, n)
        assert same(np.ascontiguousarray(whole[(whole[:, 0] >= lo) & (whole[:, 0] < lo + n)]), want)


# ---- 6: capacity ---------------------------------------------------------------------------------------------------------------------------

def test_capacity():
    circ = cycle(1)
    device_fn, host_fn = entries(circ)
    all_ = total(circ, 2, 1)
    want = exact(host_fn, 2, 1, 0, all_, EC_FLIPS)
    found = len(want)
    assert found == 3526 + 6562
    for capacity in (0, 1, found - 1):
        buf = np.full((max(capacity, 1), 2), FILL, dtype="<u8")
        assert device_fn(2, 1, 0, all_, EC_FLIPS, capacity, buf) == (found, None), capacity
        assert (buf == FILL).all(), capacity                                # a buffer too small is left as it was
    for capacity in (found, found + 3):
        buf = np.full((capacity, 2), FILL, dtype="<u8")
        got, records = device_fn(2, 1, 0, all_, EC_FLIPS, capacity, buf)
        assert got == found and same(np.ascontiguousarray(buf[:found]), want) and (buf[found:] == FILL).all(), capacity
    got, records = device_fn(2, 1, 0, all_, EC_FLIPS, 1 << 20)
    assert got == found and same(records, want)


# ---- 7: the real gadgets ----------------------------------------------------------------------------------------------------------------------

def test_whole_weight_2_of_the_one_round_cycle():
    circ = cycle(1)
    device = circ.malignant_gate_faults(2, select=EC_ALL)                    # (2, 1) and (2, 2): more than 2^16 records, the second call
    host = circ.malignant_gate_faults(2, select=EC_ALL, host=True)
    strata = circ.enumerate_gate_strata([2])                                 # the counting kernel
    assert isinstance(device, montecarlo.GateFaultLists) and len(device) > montecarlo.FAULT_LIST_FIRST_CAPACITY
    for b in range(3):
        assert same(device[b].records, host[b].records) and device[b].ranges == host[b].ranges == ((0, total(circ, 2, b)),), b
    for mask, field in EC_FIELD_OF_MASK.items():
        assert device.counts(mask).tolist() == strata.counts[0][:, :, EC.index(field)].astype(np.int64).tolist(), field
    flips = circ.malignant_gate_faults(2)                                    # the default select
    assert [len(l) for l in flips] == [188, 3526 + 6562, 6543 + 19319 + 13863]


@pytest.mark.parametrize("name, b, select", [("steane", 2, 0x0E), ("rm15", 0, 1)])
def test_weight_2_of_the_gate_free_programs_against_the_counting_kernel(name, b, select):
    """Two CNOTs of the Steane program with a wrong bit, a wrong first trial or a split vote (2.7 x 10^7 configurations), and two
    one-operand gates of the Reed-Muller program (6.6 x 10^6): no pair of those does any harm, so every accepted one is listed, 1.6
    million records, which takes the second call of the retry."""
    prog = program(name, "")
    got = prog.malignant_gate_faults(2, b, select=select, max_configurations=BUDGET)
    counts = prog.enumerate_gate_range(2, b, 0, total(prog, 2, b))
    assert len(got) > 0 and (got.classes & select != 0).all()
    for mask in (m for m in FT_FIELD_OF_MASK if m & select):
        assert got.counts(mask).tolist() == counts[:, FT.index(FT_FIELD_OF_MASK[mask])].astype(np.int64).tolist(), mask
    if select == 1:
        assert len(got) == int(counts[:, 0].sum()) > montecarlo.FAULT_LIST_FIRST_CAPACITY and not counts[:, 1:5].any()
    assert np.array_equal(got.ranks, np.sort(got.ranks)) and int(got.ranks[-1]) < total(prog, 2, b)


# ---- 8: no state between calls -----------------------------------------------------------------------------------------------------------------

def test_the_result_does_not_depend_on_earlier_calls():
    circ, prog = cycle(1), program("steane", "")
    device_fn, host_fn = entries(circ)
    other_fn, _ = entries(prog)
    first, count = 126 * 17 + 5, 3001
    want = exact(host_fn, 2, 1, first, count, EC_ALL)
    assert len(want) > 100
    clean = np.zeros((len(want) + 4, 2), dtype="<u8")
    dirty = np.full((len(want) + 4, 2), FILL, dtype="<u8")
    assert device_fn(2, 1, first, count, EC_ALL, len(clean), clean)[0] == len(want)
    assert other_fn(2, 2, 1000, 5000, FT_ALL, 1 << 20)[0] > len(want)       # another gadget, a longer list: the workspace is reused
    assert device_fn(2, 2, 100, 2000, 1, 1 << 20)[0] > len(want)
    assert device_fn(2, 1, first, count, EC_ALL, len(dirty), dirty)[0] == len(want)
    assert same(np.ascontiguousarray(clean[:len(want)]), want) and same(np.ascontiguousarray(dirty[:len(want)]), want)
    assert not clean[len(want):].any() and (dirty[len(want):] == FILL).all()
    assert device_fn(2, 1, first, count, EC_ALL, 0) == (len(want), None)    # the counter starts at zero again


# ---- 9: public entry points and refusals ---------------------------------------------------------------------------------------------------

def test_public_entry_points():
    code = make_code("steane")
    wrong = code.logical_program_malignant_gate_faults('XXX', 1)
    prog = ft_noise.program_for(code, 'XXX')
    assert isinstance(wrong, montecarlo.GateFaultLists) and [len(l) for l in wrong] == [0, 45] and wrong[1].counts().tolist() == [15, 30]
    assert sorted((g, gate, paulis) for ((g, gate, _, paulis),) in prog.describe_gate_faults(wrong)) == sorted(code.logical_program_gate_single_faults('XXX')[1])
    assert wrong.class_names == ft_noise.CLASS_NAMES
    flips = code.error_correct_malignant_gate_faults(2, rounds=1, b=1, select=ec_noise.CLASS_FLIP_Z, first_rank=1000, count=5000)
    want = ec_noise.circuit_for(code, 1).malignant_gate_faults(2, 1, select=ec_noise.CLASS_FLIP_Z, first_rank=1000, count=5000, host=True)
    assert isinstance(flips, montecarlo.GateFaultList) and same(flips.records, want.records) and flips.ranges == ((1000, 5000),)
    empty = code.error_correct_malignant_gate_faults(2, b=1, first_rank=100, count=0)
    assert len(empty) == 0 and empty.ranges == ((100, 0),) and empty.sites().shape == (0, 2)


def test_refusals():
    code = make_code("steane")
    ctx = _native.default_context()
    circ, prog = ec_noise.circuit_for(code, 1), ft_noise.program_for(code, "")
    tables = circ._tables()
    ec_sites, ft_sites = circ.gate_sites()[:3], prog.gate_sites()[:3]
    ec = lambda device=None, rounds=1, sites=ec_sites, w=1, b=0, first=0, count=1, select=1, capacity=8: \
        ctx.ec_gate_enumerate_list(circ.device() if device is None else device, rounds, *tables, *sites, w, b, first, count, select, capacity)
    ft = lambda device=None, nsteps=prog.nsteps, mask=prog.measure_mask, sites=ft_sites, w=1, b=0, first=0, count=1, select=1, capacity=8: \
        ctx.ft_gate_enumerate_list(prog.device() if device is None else device, nsteps, mask, *tables, *sites, w, b, first, count, select, capacity)
    rng = np.random.default_rng(SEED0 + 9)
    five = rng.integers(0, 1 << 62, (30, 2, 5)).astype("<u8")                # the Monte-Carlo layout is no cycle: its effects leave the layout
    five[:, :, 4] &= np.uint64(3)
    five_dev = ctx.circuit_create(five)
    thirty = (np.arange(30, dtype=np.int32), 30, 0)
    twice = ec_sites[0].copy()
    twice[5] = twice[6]
    who_ec, who_ft = ": gf2_ec_gate_enumerate_list: ", ": gf2_ft_gate_enumerate_list: "
    for call, text in ((lambda: ec(select=0), who_ec + "select names no class bit"), (lambda: ec(select=0x20), who_ec + "select 0x20 has bits outside"),
                       (lambda: ec(capacity=-1), who_ec + "negative capacity"), (lambda: ec(capacity=(1 << 28) + 1), who_ec + "capacity .* above"),
                       (lambda: ft(select=0), who_ft + "select names no class bit"), (lambda: ft(select=0x40), "class bits 0x3f"),
                       (lambda: ft(capacity=-1), who_ft + "negative capacity"),
                       (lambda: ec(five_dev, sites=thirty), "beyond"), (lambda: ft(five_dev, nsteps=4, mask=1, sites=thirty), "8 <= ldr"),
                       (lambda: ft(circ.device(), nsteps=2, mask=1, sites=ec_sites), "8 <= ldr"),
                       (lambda: ec(ft_noise.program_for(code, "XXX").device(), rounds=6), "ldr <= 8"), (lambda: ec(rounds=2), "rounds need"),
                       (lambda: ec(w=5), who_ec + "weight 5 outside"), (lambda: ec(w=2, b=3), who_ec + "3 CNOT picks outside"),
                       (lambda: ec(w=2, b=1, count=126 * 102 + 1), "leave"), (lambda: ec(first=-1), "leave"),
                       (lambda: ec(sites=(twice, 126, 102)), who_ec + "the site table is no partition"),
                       (lambda: ec(sites=(ec_sites[0][:-1], 126, 101)), "partition"), (lambda: ft(sites=ec_sites), who_ft + "the site table is no partition"),
                       (lambda: ft(w=2, b=1, first=603 * 491, count=1), "leave")):
        with pytest.raises(_native.GF2Error, match=text) as err:
            call()
        assert err.value.code == _native.GF2_E_ARG, text
    five_dev.free()
    for call in (lambda: circ.malignant_gate_faults(3, max_configurations=100), lambda: prog.malignant_gate_faults(3),
                 lambda: circ.malignant_gate_faults(5), lambda: circ.malignant_gate_faults(1, select=0x20),
                 lambda: circ.malignant_gate_faults(2, first_rank=5)):
        with pytest.raises(ValueError):
            call()
    assert ec(w=2, b=1, first=100, count=0)[0] == 0 and ft(w=2, b=2, first=100, count=0)[0] == 0
    assert ec(capacity=0) == (1, None)                                       # (rank 0 of (1, 0), select 1: accepted)
