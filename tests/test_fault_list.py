"""
Malignant fault sets of the two post-selected gadgets on the CPU (DESIGN.md sections 5b "Malignant fault sets of the cycle" and 5c
"Malignant fault sets of the measurement"): gf2_ec_enumerate_list_host / gf2_ft_enumerate_list_host (csrc/gf2_host.cpp),
ECCircuit / FTProgram.malignant_faults(host=True) and describe, montecarlo.FaultList.  Every comparison is exact.

  restatement     the host statement against tests/fault_list_ref.py, record for record: whole weights 0 and 1, windows of weight 2,
                  `select` varied
  census          the weight-1 lists are the single-fault censuses; describe() reads as single_faults()[1] (a record is a tuple over
                  its picks, so a weight-1 record is a 1-tuple of the census' entry)
  completeness    the whole weight 2 of the gate-free Steane program: 37 095 records, PAIR_COUNTS' compositions, the strata's A_2
  soundness       every listed record re-derived from its locations() / kinds() through tally_host(classes=True)
  capacity        0 counts, found - 1 leaves the buffer alone, found fills it; ranges concatenate; refusals
  round trip      FaultList.locations(): rank -> picks -> rank, up to the last ranks of weight 8
"""
import ctypes
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

from quantum_css_codes_amd import _native, ec_noise, ft_noise, montecarlo
from quantum_css_codes_amd.montecarlo import FaultList
from tests import fault_list_ref as flr
from tests import gadget_enumerate_ref as ger
from tests.test_gadget_enumerate import PAIR_COUNTS, cycle, literal_strata, program

BUDGET = 1 << 40
EC_SELECTS = (1, ec_noise.CLASS_FLIP_X, ec_noise.CLASS_FLIP_Z, ec_noise.CLASS_FLIP_X | ec_noise.CLASS_FLIP_Z,
              ec_noise.CLASS_UNCORRECTABLE_X | ec_noise.CLASS_UNCORRECTABLE_Z, 0x1f)
FT_SELECTS = (1, ft_noise.CLASS_WRONG, ft_noise.CLASS_FIRST_TRIAL_WRONG, ft_noise.CLASS_SPLIT_VOTE, ft_noise.CLASS_UNMATCHED_X | ft_noise.CLASS_UNMATCHED_Z,
              0x3f)


def host(gadget, w, select, first=None, count=None):
    return gadget.malignant_faults(w, select=select, first_rank=first, count=count, max_configurations=BUDGET, host=True)


def same_records(got, want):
    return got.dtype == np.uint64 and got.shape == want.shape and np.array_equal(got, want)


# ---- the host statement against the restatement -----------------------------------------------------------------------------------

def check_against_restatement(gadget, ref, eff, selects):
    L = ref.locations
    assert gadget.num_locations == L and gadget.ldr == ref.ldr
    for w in (0, 1):
        for select in selects:
            got = host(gadget, w, select)
            assert same_records(got.records, flr.records(ref, eff, w, 0, math.comb(L, w), select)), (w, select)
            assert (got.nb, got.weight, got.ranges) == (L, w, ((0, math.comb(L, w)),))
    assert len(host(gadget, 0, 1)) == 1 and len(host(gadget, 0, selects[1])) == 0          # no fault: accepted, and nothing else
    total = math.comb(L, 2)
    windows = ((0, 1), (1, 1), (12345, 4097), (77, 257), (total - 1000, 1000), (total // 3 + 7, 30001))
    seen = 0
    for k, (first, count) in enumerate(windows):
        for select in (selects[k % len(selects)], selects[(k + 3) % len(selects)]):
            got = host(gadget, 2, select, first, count)
            assert same_records(got.records, flr.records(ref, eff, 2, first, count, select)), (first, count, select)
            seen += len(got)
    assert seen > 100


def test_cycle_against_the_restatement():
    circ, ref, eff = cycle(1)
    check_against_restatement(circ, ref, eff, EC_SELECTS)
    circ, ref, eff = cycle(2)
    first = math.comb(ref.locations, 2) // 2 + 11
    for select in (1, ec_noise.CLASS_FLIP_X | ec_noise.CLASS_FLIP_Z):
        assert same_records(host(circ, 2, select, first, 9001).records, flr.records(ref, eff, 2, first, 9001, select)), select


def test_gate_free_steane_program_against_the_restatement():
    prog, ref, eff = program("steane", "")
    check_against_restatement(prog, ref, eff, FT_SELECTS)
    first = math.comb(ref.locations, 3) // 2 + 54321                          # 257 ranks deep inside weight 3
    assert same_records(host(prog, 3, 1, first, 257).records, flr.records(ref, eff, 3, first, 257, 1))


def test_rm15_program_lists_unmatched_keys():
    prog, ref, eff = program("rm15", "")
    got = host(prog, 2, ft_noise.CLASS_UNMATCHED_X, 2000000, 30001)
    assert same_records(got.records, flr.records(ref, eff, 2, 2000000, 30001, ft_noise.CLASS_UNMATCHED_X)) and len(got) > 0
    assert (got.classes & ft_noise.CLASS_UNMATCHED_X).all()


# ---- the weight-1 lists are the censuses --------------------------------------------------------------------------------------------

def test_weight_1_lists_are_the_censuses():
    circ = cycle(1)[0]
    classes, flipping = circ.single_faults()
    got = host(circ, 1, ec_noise.CLASS_FLIP_X | ec_noise.CLASS_FLIP_Z)
    described = circ.describe(got)
    assert len(got) == 3 and all(len(record) == 1 for record in described) and [record[0] for record in described] == flipping
    every = host(circ, 1, 1)
    assert len(every) == 390 and np.array_equal(every.classes, classes[every.locations()[:, 0], every.kinds()[:, 0]])
    for bit in (ec_noise.CLASS_FLIP_X, ec_noise.CLASS_FLIP_Z, ec_noise.CLASS_UNCORRECTABLE_X, ec_noise.CLASS_UNCORRECTABLE_Z):
        assert len(host(circ, 1, bit)) == int(((classes & 1 != 0) & (classes & bit != 0)).sum()), bit
    prog = program("steane", "XXX")[0]
    classes, wrong = prog.single_faults()
    got = host(prog, 1, ft_noise.CLASS_WRONG)
    assert len(got) == 15 and [record[0] for record in prog.describe(got)] == wrong
    assert got.composition_counts().tolist() == [[0, 0], [15, 0]] and got.coefficient((1, 1, 1)) == 5 and got.coefficient((1, 0, 0)) == 15
    every = host(prog, 1, 1)
    assert len(every) == 3032 and np.array_equal(every.classes, classes[every.locations()[:, 0], every.kinds()[:, 0]])


# ---- the whole weight 2 of the gate-free Steane program ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def steane_pairs():
    return host(program("steane", "")[0], 2, ft_noise.CLASS_WRONG)           # 11 297 880 configurations


def test_full_weight_2_of_the_gate_free_steane_program():
    got = steane_pairs()
    assert len(got) == 37095 and got.ranges == ((0, math.comb(1585, 2)),)
    assert got.composition_counts(ft_noise.CLASS_WRONG).tolist() == PAIR_COUNTS["steane"]['wrong']
    assert got.composition_counts().tolist() == PAIR_COUNTS["steane"]['wrong']
    strata = literal_strata("steane")
    for kinds in ((1, 1, 1), (1, 0, 0), (2, 3, 5)):
        coefficient = got.coefficient(kinds, ft_noise.CLASS_WRONG)
        assert isinstance(coefficient, Fraction) and coefficient == strata.coefficients(kinds, 'wrong')[2], kinds
    counts = got.location_counts()
    assert counts.shape == (1585,) and int(counts.sum()) == 2 * 37095
    assert np.array_equal(counts, np.bincount(got.locations().reshape(-1), minlength=1585))
    split = got.location_counts(ft_noise.CLASS_SPLIT_VOTE)
    assert int(split.sum()) == 2 * int((got.classes & ft_noise.CLASS_SPLIT_VOTE != 0).sum()) and (split <= counts).all()


def rederived_classes(gadget, fault_list):
    """The class bytes of a list's records from their locations() and kinds() alone: the picks' effect words XOR-ed, judged by the
    gadget's tally_host."""
    eff = gadget.effects
    single = np.stack((eff[:, 0], eff[:, 0] ^ eff[:, 1], eff[:, 1]), axis=1)                 # X, Y, Z
    words = np.zeros((len(fault_list), gadget.ldr), dtype=np.uint64)
    for j in range(fault_list.weight):
        words ^= single[fault_list.locations()[:, j], fault_list.kinds()[:, j]]
    return gadget.tally_host(words, classes=True)[1]


def test_every_listed_record_is_sound():
    got = steane_pairs()
    assert np.array_equal(rederived_classes(program("steane", "")[0], got), got.classes)
    assert ((got.classes & 1 != 0) & (got.classes & ft_noise.CLASS_WRONG != 0)).all()
    circ = cycle(1)[0]
    for select in (1, ec_noise.CLASS_FLIP_X | ec_noise.CLASS_FLIP_Z):
        flips = host(circ, 2, select)
        assert np.array_equal(rederived_classes(circ, flips), flips.classes) and (flips.classes & select != 0).all()
    assert len(flips) == 10263
    locations = flips.locations()
    assert (locations[:, 0] < locations[:, 1]).all() and locations.max() < 330 and flips.kinds().max() <= 2


# ---- capacity, concatenation, refusals ------------------------------------------------------------------------------------------------

def raw_ec(circ, w, first, count, select, capacity, fill=0xA5):
    """gf2_ec_enumerate_list_host through ctypes with a buffer of max(capacity, 1) records filled with `fill`: (found, buffer)."""
    eff = np.ascontiguousarray(circ.effects, dtype="<u8")
    r1, keys1, flips1, r2, keys2, flips2 = circ._tables()
    keep, (t1, t2) = _native._enumerate_tables(keys1, flips1, keys2, flips2)
    buf = np.full((max(capacity, 1), 2), fill * 0x0101010101010101, dtype="<u8")
    found = ctypes.c_int64(-1)
    _native.check(_native.lib().gf2_ec_enumerate_list_host(_native._ptr(eff), eff.shape[0], eff.shape[2], circ.rounds, int(r1), *t1, int(r2), *t2,
                                                           w, first, count, select, capacity, _native._ptr(buf), ctypes.byref(found)))
    return int(found.value), buf


def test_capacity():
    circ = cycle(1)[0]
    select = ec_noise.CLASS_FLIP_X | ec_noise.CLASS_FLIP_Z
    whole = host(circ, 2, select)
    found = len(whole)
    untouched = np.uint64(0xA5A5A5A5A5A5A5A5)
    total = math.comb(330, 2)
    for capacity in (0, 1, found - 1):
        got, buf = raw_ec(circ, 2, 0, total, select, capacity)
        assert got == found and (buf == untouched).all(), capacity
    for capacity in (found, found + 5):
        got, buf = raw_ec(circ, 2, 0, total, select, capacity)
        assert got == found and np.array_equal(buf[:found], whole.records) and (buf[found:] == untouched).all(), capacity
    tables = circ._tables()
    assert _native.ec_enumerate_list_host(circ.effects, 1, *tables, 2, 0, total, select, 0) == (found, None)
    assert _native.ec_enumerate_list_host(circ.effects, 1, *tables, 2, 0, total, select, found - 1) == (found, None)
    count, records = _native.ec_enumerate_list_host(circ.effects, 1, *tables, 2, 100, 0, select, 4)
    assert count == 0 and records.shape == (0, 2)
    prog = program("steane", "")[0]
    args = (prog.effects, prog.nsteps, prog.measure_mask) + tuple(tables)
    found, records = _native.ft_enumerate_list_host(*args, 1, 0, 1585, 1, 1 << 12)
    assert found == 1835 and records.shape == (1835, 2)
    assert _native.ft_enumerate_list_host(*args, 1, 0, 1585, 1, 1834) == (1835, None)


def test_the_retry_returns_the_whole_list(monkeypatch):
    circ = cycle(1)[0]
    whole = host(circ, 2, 1)                                                  # every accepted pair: more than the first capacity
    assert len(whole) > montecarlo.FAULT_LIST_FIRST_CAPACITY
    assert int(circ.enumerate_strata([2], host=True).counts[0][:, :, 0].sum()) == len(whole)
    monkeypatch.setattr(montecarlo, "FAULT_LIST_MAX_RECORDS", 1000)
    with pytest.raises(ValueError, match="narrower select"):
        host(circ, 2, 1)
    assert len(host(circ, 1, 1)) == 390                                       # (within the first capacity: no limit applies)


def test_ranges_concatenate():
    circ = cycle(1)[0]
    select = ec_noise.CLASS_FLIP_X | ec_noise.CLASS_FLIP_Z
    whole = host(circ, 2, select)
    total = math.comb(330, 2)
    cuts = [0, 1, 20011, 20011, total]
    parts = [host(circ, 2, select, lo, hi - lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
    joined = parts[0] + parts[1] + parts[2] + parts[3]
    assert isinstance(joined, FaultList) and same_records(joined.records, whole.records)
    assert joined.ranges == tuple((lo, hi - lo) for lo, hi in zip(cuts[:-1], cuts[1:]))
    assert np.array_equal(joined.location_counts(), whole.location_counts()) and joined.coefficient() == whole.coefficient()
    with pytest.raises(ValueError, match="ascending"):
        parts[3] + parts[0]
    with pytest.raises(ValueError, match="ascending"):
        parts[1] + parts[1]
    with pytest.raises(ValueError, match="one"):
        parts[0] + host(circ, 1, select)
    with pytest.raises(ValueError, match="one"):
        parts[0] + host(program("steane", "")[0], 2, ft_noise.CLASS_WRONG, 0, 10)


def test_a_fault_list_is_immutable_and_checks_its_records():
    circ = cycle(1)[0]
    got = host(circ, 1, 1)
    with pytest.raises(AttributeError):
        got.weight = 2
    with pytest.raises(ValueError):
        got.records[0, 0] = 5
    with pytest.raises(ValueError):
        got.ranks[0] = 5
    names = ec_noise.CLASS_NAMES
    rec = lambda rank, code, cls: (rank, code | cls << 32)
    FaultList(10, 2, [rec(3, 0, 1), rec(3, 4, 3), rec(7, 8, 1)], names)
    for bad in ([rec(7, 0, 1), rec(3, 0, 1)], [rec(3, 4, 1), rec(3, 4, 1)], [rec(3, 9, 1)], [rec(45, 0, 1)], [rec(3, 0, 2)], [(3, 1 << 20 | 1 << 32)]):
        with pytest.raises(ValueError, match="records"):
            FaultList(10, 2, bad, names)
    with pytest.raises(ValueError, match="weight"):
        FaultList(10, 9, [], names)
    with pytest.raises(ValueError, match="accepted"):
        FaultList(10, 2, [], ('wrong',))
    empty = FaultList(10, 2, [], names, [(5, 0)])
    assert len(empty) == 0 and empty.locations().shape == (0, 2) and empty.kinds().shape == (0, 2) and empty.coefficient() == 0
    assert not empty.location_counts().any() and empty.location_counts().shape == (10,) and not empty.composition_counts().any()


def test_refused_arguments_of_the_host_entry_points():
    circ, prog = cycle(1)[0], program("steane", "")[0]
    tables = circ._tables()
    r1, keys1, flips1, r2, keys2, flips2 = tables
    ec = lambda eff=circ.effects, rounds=1, tables=tables, w=1, first=0, count=1, select=1, capacity=8: \
        _native.ec_enumerate_list_host(eff, rounds, *tables, w, first, count, select, capacity)
    ft = lambda eff=prog.effects, nsteps=prog.nsteps, mask=prog.measure_mask, tables=tables, w=1, first=0, count=1, select=1, capacity=8: \
        _native.ft_enumerate_list_host(eff, nsteps, mask, *tables, w, first, count, select, capacity)
    wide_ec, wide_ft = np.zeros((4, 2, 9), dtype="<u8"), np.zeros((4, 2, 17), dtype="<u8")
    for call, text in ((lambda: ec(select=0), "select"), (lambda: ec(select=0x20), "class bits"), (lambda: ec(select=1 << 40), "class bits"),
                       (lambda: ec(capacity=-1), "capacity"),
                       (lambda: ft(select=0), "select"), (lambda: ft(select=0x40), "class bits"), (lambda: ft(capacity=-1), "capacity"),
                       (lambda: ec(w=9), "weight"), (lambda: ec(w=-1), "weight"), (lambda: ec(np.zeros((2, 2, 3), dtype="<u8"), w=3), "weight"),
                       (lambda: ec(w=2, count=math.comb(330, 2) + 1), "leave"), (lambda: ec(first=330, count=1), "leave"),
                       (lambda: ec(first=-1), "leave"), (lambda: ec(count=-1), "leave"),
                       (lambda: ec(wide_ec, rounds=2), "ldr <= 8"), (lambda: ec(rounds=2), "F >= 1"), (lambda: ec(rounds=0), "rounds"),
                       (lambda: ec(np.zeros((4, 2, 8), dtype="<u8"), rounds=7), "rounds <= 6"),
                       (lambda: ec(tables=(32, keys1, flips1, r2, keys2, flips2)), "<= 31"), (lambda: ec(tables=(r1, keys1, flips1, 0, keys2, flips2)), "<= 31"),
                       (lambda: ec(tables=(r1, np.append(keys1, keys1[:1]), np.append(flips1, 0), r2, keys2, flips2)), "twice"),
                       (lambda: ec(circ.effects | np.uint64(1 << 20)), "beyond"),
                       (lambda: ft(w=9), "weight"), (lambda: ft(w=2, first=math.comb(1585, 2), count=1), "leave"),
                       (lambda: ft(wide_ft, nsteps=6), "ldr <= 16"), (lambda: ft(nsteps=8), "F >= 1"), (lambda: ft(nsteps=0, mask=0), "nsteps >= 1"),
                       (lambda: ft(mask=0b010100), "odd number"), (lambda: ft(mask=1 << 6), "at or above nsteps"),
                       (lambda: ft(tables=(r1, keys1, flips1, 32, keys2, flips2)), "<= 31"),
                       (lambda: ft(prog.effects | np.uint64(1 << 40)), "beyond")):
        with pytest.raises(_native.GF2Error, match=text) as err:
            call()
        assert err.value.code == _native.GF2_E_ARG, text
    assert ec(w=2, first=100, count=0)[0] == 0 and ft(w=2, first=100, count=0)[0] == 0
    assert ec(capacity=0) == (1, None)                                        # (rank 0 of weight 1, select 1: accepted)
    for call in (lambda: circ.malignant_faults(1, select=0, host=True), lambda: circ.malignant_faults(1, select=0x20, host=True),
                 lambda: prog.malignant_faults(1, select=0x40, host=True), lambda: circ.malignant_faults(9, host=True),
                 lambda: prog.malignant_faults(1, first_rank=1585, count=1, host=True), lambda: prog.malignant_faults(3, host=True),
                 lambda: circ.malignant_faults(2, max_configurations=100, host=True)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match="locations"):
        circ.describe(prog.malignant_faults(1, host=True))


# ---- rank -> picks -> rank -------------------------------------------------------------------------------------------------------------

def test_locations_round_trip():
    names = ft_noise.CLASS_NAMES
    rng = np.random.default_rng(20261018)
    nb_8 = max(n for n in range(8, 2000) if math.comb(n, 8) < 1 << 63)        # the widest weight-8 list whose ranks fit 63 bits
    assert math.comb(nb_8 + 1, 8) >= 1 << 63
    for nb, w in ((1585, 2), (3867, 2), (2584, 3), (330, 1), (40, 5), (21, 8), (200, 8), (nb_8, 8), (8, 8), (1 << 20, 3), (5, 0)):
        total = math.comb(nb, w)
        edge = [r for r in (0, 1, 2, total // 2, total - 3, total - 2, total - 1) if 0 <= r < total]
        ranks = sorted(set(edge + [int(rng.integers(0, total)) for _ in range(40 if total > 50 else 0)]))
        got = FaultList(nb, w, [(r, 1 << 32) for r in ranks], names)
        picks = got.locations()
        assert picks.shape == (len(ranks), w) and picks.dtype == np.int64
        assert [ger.rank_of(row) for row in picks.tolist()] == ranks, (nb, w)
        assert all(0 <= row[0] and row[-1] < nb and all(a < b for a, b in zip(row[:-1], row[1:])) for row in picks.tolist() if w)
        for r, row in list(zip(ranks, picks.tolist()))[:8] + list(zip(ranks, picks.tolist()))[-4:]:
            assert _native.subset_unrank(nb, w, r).tolist() == row, (nb, w, r)
        if w:
            assert picks[-1].tolist() == list(range(nb - w, nb))              # the last rank: the top w locations
    codes = FaultList(10, 3, [(5, c | 1 << 32) for c in range(27)], names)
    assert codes.kinds().tolist() == [[c % 3, c // 3 % 3, c // 9] for c in range(27)]
    assert codes.composition_counts().sum() == 27 and codes.composition_counts()[3, 0] == 1 and codes.composition_counts()[1, 1] == 6
    assert codes.coefficient((1, 1, 1)) == 1 and codes.coefficient((1, 0, 0)) == 1 and codes.coefficient((0.5, 0.25, 0.25)) == pytest.approx(1.0)
