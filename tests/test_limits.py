"""
tests/test_gpu_limits.py tied to what exists, without a GPU, so that it does not stand on one leg (DESIGN.md section 5g "Top of the accepted
ranges").  Every comparison is exact.

  limits            the table of the largest L with C(L, w) < 2^63 and the gate-level site tables, computed and compared with the
                    literals; one step beyond each is refused by the host statements with the documented message
  non-vacuity       every reference of the GPU file meets, for the committed seeds, the conditions it asserts before the device is asked
  host statements   every host statement the GPU file compares the device with equals its NumPy restatement on a short window or a
                    short sample range of the very tables used there
  resolving power   eight wrong kernels, restated, each change the reference words or counts of a case the GPU file runs
  coverage          every entry point of the issue appears in the GPU file with the limit it reaches
"""
import inspect
import itertools
import math
import re

import numpy as np
import pytest

from quantum_css_codes_amd import _native
from tests import enumerate_ref, fault_list_ref, gadget_enumerate_ref, gadget_strata_ref, gadget_tally_ref as ref, gate_enumerate_ref, gate_mc_ref
from tests import gate_strata_ref as gsr, strata_ref, stream_ref
from tests import test_gpu_limits as gpu_cases
from tests.test_gpu_limits import CACHED, LMAX, SEG, TALLIES, TOP, table

TWO63 = 1 << 63
SHORT = 64                                                                   # samples of a short range


@pytest.fixture(scope="module", autouse=True)
def drop_the_references():
    yield
    for fn in CACHED:
        fn.cache_clear()


# ---- the restated gadgets on plain tables ---------------------------------------------------------------------------------------------

#  the count fields that make the class byte's bits, from bit 0 (include/gf2hip.h "malignant fault sets")
CLASS_FIELDS = {"cycle": (0, 1, 2, 4, 5), "program": (0, 1, 3, 4, 5, 6)}


class Gadget(object):
    """What tests/gadget_enumerate_ref.py, tests/gate_enumerate_ref.py and tests/fault_list_ref.py ask of a gadget, on a synthetic effect
    table: locations, ldr, gates and tally(words) -> (counts, class bytes) by the rules of tests/gadget_tally_ref.py."""

    def __init__(self, kind, eff, args, gates=None, classes=False):
        self.kind, self.args, self.gates, self.classes = kind, args, gates, classes
        self.locations, self.ldr = eff.shape[0], eff.shape[2]

    def tally(self, words):
        counts = [int(v) for v in TALLIES[self.kind](words, *self.args)]
        classes = np.zeros(len(words), dtype=np.uint8)
        if self.classes:
            for i in range(len(words)):
                one = TALLIES[self.kind](words[i:i + 1], *self.args)
                classes[i] = sum(1 << bit for bit, field in enumerate(CLASS_FIELDS[self.kind]) if one[field])
        return counts, classes


def short_windows(wins, configurations, rows=12000, most=5):
    """The windows of the GPU file cut to a few ranks around the same boundaries: (first, count) with count * configurations <= rows."""
    count = max(1, min(most, rows // configurations))
    return [(first + n // 2 - count // 2, count) if k not in (0, len(wins) - 1) else (first, count) if k == 0 else (first + n - count, count)
            for k, (first, n) in enumerate(wins)]


# ---- the limits ---------------------------------------------------------------------------------------------------------------------------

def test_the_largest_rank_spaces():
    assert [gpu_cases.largest_locations(w) for w in gpu_cases.ENUM_WEIGHTS] == [TOP, TOP, 121977, 16175, 4337, 1733, 887] == list(LMAX.values())
    assert math.comb(TOP, 3).bit_length() == 58
    for w, L in LMAX.items():
        assert math.comb(L, w) < TWO63 and (L == TOP or math.comb(L + 1, w) >= TWO63)
        n = gpu_cases.window_size(3**w)
        assert n % 2 == 1 and n >= 257 and n * 3**w <= 4 * 10**6
    tables = {s: gpu_cases.gate_enum_sites(*s) for s in gpu_cases.GATE_ENUM_STRATA}
    assert tables == {(2, 0): (TOP, 0), (0, 2): (0, TOP >> 1), (3, 0): (TOP, 0), (2, 2): tables[2, 2], (4, 0): (121977, 0), (0, 4): (0, 121977),
                      (1, 3): tables[1, 3]}
    for (a, b), (n1, n2) in tables.items():
        assert n1 + 2 * n2 <= TOP and math.comb(n1, a) * math.comb(n2, b) < TWO63 and (a == 0 or b == 0 or n1 >= 2 * n2 > 0)
        more = gpu_cases.one_site_more(a, b)
        assert (more is None) == (n1 + 2 * n2 == TOP) and (more is None or math.comb(more[0], a) * math.comb(more[1], b) >= TWO63)
    assert [(-(-n1 // SEG), -(-n2 // SEG)) for n1, n2 in gpu_cases.SITE_TABLES] == [(2048, 0), (0, 1024), (1025, 512)]
    assert [((n1 - 1) % SEG + 1 if n1 else 0, (n2 - 1) % SEG + 1 if n2 else 0) for n1, n2 in gpu_cases.SITE_TABLES] == [(512, 0), (0, 512), (2, 511)]
    assert [-(-L // SEG) for L in gpu_cases.LOCATIONS] == [2048] * 3 and [(L - 1) % SEG + 1 for L in gpu_cases.LOCATIONS] == [512, 511, 1]


def refused(text, fn, *args):
    with pytest.raises(_native.GF2Error, match=text) as err:
        fn(*args)
    assert err.value.code == _native.GF2_E_ARG, err.value.message


@pytest.mark.parametrize("w", [4, 5, 6, 7, 8])
def test_one_location_beyond_is_refused_by_the_host_statements(w):
    L = LMAX[w] + 1
    text = r"C\(%d, %d\) subsets do not fit 63 bits" % (L, w)
    eff, args = table("decode", gpu_cases.DECODE_ONE, L)
    refused(text, _native.circuit_enumerate_host, eff, *args, w, 0, 1)
    eff, args = table("cycle", gpu_cases.CYCLE_LDR3, L)
    refused(text, _native.ec_enumerate_host, eff, *args, w, 0, 1)
    refused(text, _native.ec_enumerate_list_host, eff, *args, w, 0, 1, 1, 8)
    eff, args = table("program", gpu_cases.PROGRAM_LDR8, L)
    refused(text, _native.ft_enumerate_host, eff, *args, w, 0, 1)
    refused(text, _native.ft_enumerate_list_host, eff, *args, w, 0, 1, 1, 8)
    eff, args = table("cycle", gpu_cases.CYCLE_LDR3, L - 1)                   # ... and the limit itself is taken, to its last rank
    assert _native.ec_enumerate_host(eff, *args, w, math.comb(L - 1, w) - 1, 1).sum() >= 0


@pytest.mark.parametrize("a, b", [s for s in gpu_cases.GATE_ENUM_STRATA if gpu_cases.one_site_more(*s)], ids=lambda v: str(v))
def test_one_site_beyond_is_refused_by_the_host_statements(a, b):
    n1, n2 = gpu_cases.one_site_more(a, b)
    text = r"C\(%d, %d\) C\(%d, %d\) subsets do not fit 63 bits" % (n1, a, n2, b)
    site_loc = np.concatenate((np.arange(n1), n1 + 2 * np.arange(n2))).astype(np.int32)
    eff, args = table("cycle", gpu_cases.CYCLE_LDR3, n1 + 2 * n2)
    refused(text, _native.ec_gate_enumerate_host, eff, *args, site_loc, n1, n2, a + b, b, 0, 1)
    eff, args = table("program", gpu_cases.PROGRAM_LDR8, n1 + 2 * n2)
    refused(text, _native.ft_gate_enumerate_host, eff, *args, site_loc, n1, n2, a + b, b, 0, 1)


def test_beyond_2_to_the_20_locations_and_beyond_weight_16_is_refused_by_the_host_statements():
    eff, args = table("cycle", gpu_cases.CYCLE_LDR3, TOP)
    beyond = np.concatenate((eff, eff[:1]))
    text = r"needs 1 <= L <= 1048576 \(2\^20\) locations, got 1048577"
    refused(text, _native.ec_enumerate_host, beyond, *args, 2, 0, 1)
    refused(r"needs 1 <= locations <= 1048576 \(2\^20\), got 1048577", _native.stratum_outcomes_host, beyond, 1, 1)
    refused(text, _native.gate_stratum_outcomes_host, beyond, np.arange(TOP + 1, dtype=np.int32), TOP + 1, 0, 1, 0, 1)
    refused(text, _native.gate_outcomes_host, beyond, np.arange(TOP + 1, dtype=np.int32), TOP + 1, 0, 1, 0.1, 0.1)
    refused(r"weight 17 outside \[0, min\(L = 1048576, 16\)\]", _native.stratum_outcomes_host, eff, 17, 1)
    sites = gpu_cases.site_table(*gpu_cases.SITE_TABLES[2])
    for a, b in ((17, 0), (0, 17), (9, 8)):
        refused(r"a \+ b <= 16 faulty gates", _native.gate_stratum_outcomes_host, eff, *sites, a, b, 1)


# ---- the references of the GPU file are not vacuous ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(gpu_cases.SAMPLER_CASES))
def test_sampler_references_are_not_vacuous(name):
    entry = gpu_cases.SAMPLER_CASES[name][0]
    reference = gpu_cases.sampler_reference(name)
    gpu_cases.assert_sparse_run(name, reference)
    if entry in ("store", "ft"):
        gpu_cases.assert_dense_run(name, gpu_cases.sampler_reference(name, True))
    eff, args, seed, first, p, faults, words, counts = reference
    # the fault list drawn in chunks and XOR-ed here is gadget_tally_ref.sampled_words; the restated tally is the host statement's
    assert np.array_equal(words[:SHORT], ref.sampled_words(eff, seed, first, SHORT, p))
    if entry in ("ec", "ft"):
        host = _native.ec_tally_host if entry == "ec" else _native.ft_tally_host
        assert host(words, *args).tolist() == counts


@pytest.mark.parametrize("name", list(gpu_cases.STRATA_CASES))
def test_strata_references_are_not_vacuous(name):
    reference = gpu_cases.strata_reference(name)
    gpu_cases.assert_strata(name, reference)
    eff, args, seed, first, counts = reference
    for w in gpu_cases.STRATA_WEIGHTS:                                       # gf2_stratum_outcomes_host on a short range of the same table
        want = gadget_strata_ref.stratum_words(eff, seed, first, SHORT, w, gpu_cases.STRATA_KINDS)
        assert np.array_equal(_native.stratum_outcomes_host(eff, w, SHORT, gpu_cases.STRATA_KINDS, seed, first), want), (name, w)


@pytest.mark.parametrize("n1, n2", gpu_cases.SITE_TABLES, ids=lambda v: str(v))
def test_gate_references_are_not_vacuous(n1, n2):
    for name in gpu_cases.GATE_CASES:
        reference = gpu_cases.gate_strata_reference(name, n1, n2)
        gpu_cases.assert_gate_strata(reference)
        eff, args, sites, strata = reference
        for a, b, seed, first, counts in strata:                              # gf2_gate_stratum_outcomes_host on a short range
            words, c = gsr.gate_stratum_words(eff, sites[0], n1, n2, seed, first, SHORT, a, b)
            got, got_c = _native.gate_stratum_outcomes_host(eff, *sites, a, b, SHORT, seed, first)
            assert np.array_equal(got, words) and np.array_equal(got_c, c), (name, a, b)
        eff, args, sites, seed, first, p, counts = gpu_cases.gate_mc_reference(name, n1, n2)
        gpu_cases.assert_gate_mc(n1, n2, counts)
        words, abc = gate_mc_ref.gate_mc_words(eff, sites[0], n1, n2, seed, first, 8, *p)     # gf2_gate_outcomes_host, likewise
        got, got_abc = _native.gate_outcomes_host(eff, *sites, 8, *p, seed, first)
        assert np.array_equal(got, words) and np.array_equal(got_abc, abc), name
        assert np.array_equal(gpu_cases.words_of_gate_faults(eff, sites[0], gpu_cases.gate_mc_fault_list(n1, n2), gpu_cases.GATE_MC_SAMPLES)[:8], words)


# ---- the host statements of the enumerations against the restatements -------------------------------------------------------------------

@pytest.mark.parametrize("name, w", gpu_cases.ENUM_RUNS)
def test_enumeration_host_statements_are_the_restatements(name, w):
    entry, kind, case, _ = gpu_cases.ENUM_CASES[name]
    L = LMAX[w]
    eff, args = table(kind, case, L)
    gadget = Gadget(kind, eff, args)
    for first, count in short_windows(gpu_cases.windows(L, w), 3**w):
        want = gadget_enumerate_ref.enumerate_range(gadget, eff, w, first, count)
        got = gpu_cases.ENUM_HOST[entry](eff, *args, w, first, count)
        assert got.tolist() == want.tolist(), (name, w, first)
    if entry != "decode":
        listing = Gadget(kind, eff, args, classes=True)
        first, count = short_windows(gpu_cases.windows(L, w), 3**w, 3000)[1]   # across C(L - 1, w)
        for select in gpu_cases.LIST_SELECTS[entry]:
            want = fault_list_ref.records(listing, eff, w, first, count, select)
            found, got = gpu_cases.LIST_HOST[entry](eff, *args, w, first, count, select, 3**w * count)
            assert found == len(want) and got.tobytes() == want.tobytes(), (name, w, select)


def test_enumeration_references_are_not_vacuous():
    for name, w in gpu_cases.ENUM_RUNS:
        gpu_cases.assert_enumeration(name, w, gpu_cases.enumerate_reference(name, w))


@pytest.mark.parametrize("a, b", gpu_cases.GATE_ENUM_STRATA, ids=lambda v: str(v))
def test_gate_enumeration_host_statements_are_the_restatements(a, b):
    n1, n2 = gpu_cases.gate_enum_sites(a, b)
    sites = gpu_cases.gate_enum_site_table(n1, n2)
    assert sites[0].tolist() == gate_enumerate_ref.sites(gpu_cases.gate_enum_gates(n1, n2))[0]
    for name, (entry, kind, case) in gpu_cases.GATE_ENUM_CASES.items():
        gpu_cases.assert_gate_enumeration(a, b, gpu_cases.gate_enumerate_reference(name, a, b))
        eff, args = table(kind, case, n1 + 2 * n2)
        gadget = Gadget(kind, eff, args, gates=gpu_cases.gate_enum_gates(n1, n2))
        big = n1 + 2 * n2 == TOP                                              # (the restatement walks the 2^20 gates in Python, tabulates every kind
        wins = short_windows(gpu_cases.gate_windows(n1, n2, a, b), 3**a * 15**b, 60000, 2 if big else 5)   # mask of every site and unranks by a linear scan,
        for first, count in wins[-1:] if big and entry == "ft" else wins:     # per call: of the measurement on those tables the last window alone)
            want = gate_enumerate_ref.enumerate_range(gadget, eff, a + b, b, first, count)
            got = gpu_cases.GATE_ENUM_HOST[entry](eff, *args, *sites, a + b, b, first, count)
            assert got.tolist() == want.tolist(), (name, a, b, first)


# ---- resolving power: eight wrong kernels -------------------------------------------------------------------------------------------------

def test_a_dropped_or_wrapped_segment_changes_the_sampler_references():
    for name in ("store-3-words", "ec-ldr3", "ft-ldr16", "ec-ldr3-last1"):
        entry, kind, case, locations = gpu_cases.SAMPLER_CASES[name]
        eff, args, seed, first, p, (fault_first, location, fkind), words, counts = gpu_cases.sampler_reference(name)
        sample = np.repeat(np.arange(gpu_cases.SAMPLES), np.diff(fault_first))

        def wrong(keep, where):
            kept_first = np.concatenate(([0], np.cumsum(np.bincount(sample[keep], minlength=gpu_cases.SAMPLES))))
            return gpu_cases.words_of_faults(eff, (kept_first, where[keep], fkind[keep]))

        dropped = wrong(location // SEG != 2047, location)                    # segment 2047 dropped
        wrapped = wrong(np.ones(len(location), dtype=bool), location % (1 << 19))   # the location index taken modulo 2^19
        for mutant in (dropped, wrapped):
            assert not np.array_equal(mutant, words), name
            assert counts is None or list(TALLIES[kind](mutant, *args)) != counts, name


def test_a_last_segment_taken_as_whole_changes_the_sampler_references():
    """The last segment's size taken as 512 when it is 1 or 511: the oracle's sampler over 2^20 locations with the rates of the case,
    the faults past the table dropped.  A last segment of 511 locations has some two faults in the 2085 samples of a mean-2 run, and
    a fault's place changes with the segment's size half of the time: the dense store run of the case, with some forty, tells."""
    changed = {}
    for name, dense in (("store-3-words-last511", False), ("store-3-words-last511", True), ("ec-ldr3-last511", False),
                        ("store-3-words-last1", False), ("store-3-words-last1", True), ("ec-ldr3-last1", False)):
        entry, kind, case, locations = gpu_cases.SAMPLER_CASES[name]
        eff, args, seed, first, p, faults, words, counts = gpu_cases.sampler_reference(name, dense)
        parts = [stream_ref.sampled_faults(TOP, seed, first + at, min(gpu_cases.CHUNK, gpu_cases.SAMPLES - at), p) for at in range(0, gpu_cases.SAMPLES, gpu_cases.CHUNK)]
        location, fkind = np.concatenate([part[1] for part in parts]), np.concatenate([part[2] for part in parts])
        sample = np.repeat(np.arange(gpu_cases.SAMPLES), np.concatenate([np.diff(part[0]) for part in parts]))
        keep = location < locations
        kept_first = np.concatenate(([0], np.cumsum(np.bincount(sample[keep], minlength=gpu_cases.SAMPLES))))
        mutant = gpu_cases.words_of_faults(eff, (kept_first, location[keep], fkind[keep]))
        changed[name, dense] = not np.array_equal(mutant, words) if counts is None else list(TALLIES[kind](mutant, *args)) != counts
    assert changed["store-3-words-last511", True] and changed["store-3-words-last1", False] and changed["store-3-words-last1", True], changed


def test_a_target_row_read_at_the_control_changes_the_gate_references():
    """The CNOT target row read at l instead of l + 1."""
    for n1, n2 in gpu_cases.SITE_TABLES[1:]:
        for name, (entry, kind, case) in gpu_cases.GATE_CASES.items():
            eff, args, sites, seed, first, p, counts = gpu_cases.gate_mc_reference(name, n1, n2)
            sample, site, kappa = gpu_cases.gate_mc_fault_list(n1, n2)
            mutant = np.zeros((gpu_cases.GATE_MC_SAMPLES, eff.shape[2]), dtype=np.uint64)
            loc = np.asarray(sites[0], dtype=np.int64)[site]
            for bit in range(4):
                has = ((kappa >> bit) & 1).astype(bool)
                np.bitwise_xor.at(mutant, sample[has], eff[loc[has], bit & 1])
            assert list(TALLIES[kind](mutant, *args)) != counts, (name, n1, n2)
            eff, args, sites, strata = gpu_cases.gate_strata_reference(name, n1, n2)
            for a, b, seed, first, want in strata:
                if b:
                    site, kappa = gsr.gate_stratum_draws(seed, first, gpu_cases.STRATA_SAMPLES, n1, n2, a, b)
                    words = np.zeros((gpu_cases.STRATA_SAMPLES, eff.shape[2]), dtype=np.uint64)
                    for k in range(a + b):
                        loc = np.asarray(sites[0], dtype=np.int64)[site[:, k]]
                        for bit in range(4):
                            has = ((kappa[:, k] >> bit) & 1).astype(bool)
                            words[has] ^= eff[loc[has], bit & 1]
                    got = gpu_cases.by_two_operand(words, gsr.two_operand(kappa, a), lambda w: TALLIES[kind](w, *args), want.shape[1])
                    assert not np.array_equal(got, want), (name, n1, n2, a, b)


def test_a_fallback_without_its_step_changes_the_strata_references():
    """Floyd's fallback L - w + k replaced by L - w."""
    changed = 0
    for name, (entry, kind, case) in gpu_cases.STRATA_CASES.items():
        eff, args, seed, first, counts = gpu_cases.strata_reference(name)
        w, count = 16, gpu_cases.STRATA_SAMPLES
        pos, fkind = strata_ref.stratum_draws(seed, first, count, TOP, w, gpu_cases.STRATA_KINDS)
        t = gpu_cases.floyd_candidates(seed, first, count, w + 1, [TOP - w + k for k in range(w)])
        wrong = pos.copy()
        for k in range(w):                                                    # the draw again, the fallback without its step
            taken = (wrong[:, :k] == t[:, k:k + 1]).any(axis=1)
            wrong[:, k] = np.where(taken, TOP - w, t[:, k])
        assert (wrong != pos).any(), name
        words = np.zeros((count, eff.shape[2]), dtype=np.uint64)
        for k in range(w):
            has_x, has_z = (fkind[:, k] & 1).astype(bool), (fkind[:, k] >> 1).astype(bool)
            words[has_x] ^= eff[wrong[has_x, k], 0]
            words[has_z] ^= eff[wrong[has_z, k], 1]
        changed += list(TALLIES[kind](words, *args)) != counts[-1]
    assert changed >= 1
    for n1, n2 in gpu_cases.SITE_TABLES:                                      # ... and over gates: the picks change in every stratum
        sites = gpu_cases.site_table(n1, n2)
        for a, b in gpu_cases.gate_strata_of(n1, n2):
            seed, first = gpu_cases.GATE_STRATA_SEEDS[n1, n2, a, b]
            assert gpu_cases.gate_strata_fallbacks(sites, a, b, seed, first)[0] >= 1


def wrapping_binom(s, k):
    """C(s, k) as 64-bit c * m / d, the product wrapping."""
    if s < k:
        return 0
    c = 1
    for i in range(k):
        c = ((c * (s - k + 1 + i)) & (TWO63 * 2 - 1)) // (i + 1)
    return c


def unrank_with(nb, w, rank, binom=math.comb, top=None):
    """tests/enumerate_ref.unrank with another binomial, or with the top pick's search bounded by `top`."""
    out, hi = [], nb if top is None else top
    for k in range(w, 0, -1):
        lo = k - 1
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if binom(mid, k) <= rank else (lo, mid)
        out.append(lo)
        rank -= binom(lo, k)
        hi = lo
    return out[::-1]


def window_counts(kind, eff, args, subsets):
    """The counts of the restated tally over every kind assignment of the subsets."""
    picks = np.array(subsets, dtype=np.int64)
    total = None
    for kinds in itertools.product((1, 2, 3), repeat=picks.shape[1]):
        words = np.zeros((len(picks), eff.shape[2]), dtype=np.uint64)
        for k, bits in enumerate(kinds):
            if bits & 1:
                words ^= eff[picks[:, k], 0]
            if bits & 2:
                words ^= eff[picks[:, k], 1]
        got = list(TALLIES[kind](words, *args))
        total = got if total is None else [x + y for x, y in zip(total, got)]
    return total


def test_wrong_unranking_changes_the_enumeration_references():
    """Binomials computed as wrapping 64-bit c * m / d; the top pick's search bounded by L - 1 instead of L."""
    for w in (4, 5):
        L = LMAX[w]
        eff, args = table("cycle", gpu_cases.CYCLE_LDR3, L)
        wins = gpu_cases.windows(L, w)
        for mutant, windows_hit in ((dict(binom=wrapping_binom), wins[1:]), (dict(top=L - 1), wins[2:])):
            for first, n in windows_hit:
                ranks = range(first + n - 9, first + n)                       # the window's last ranks
                right = [enumerate_ref.unrank(L, w, r) for r in ranks]
                assert right == [unrank_with(L, w, r) for r in ranks] and right[-1][-1] == L - 1
                wrong = [unrank_with(L, w, r, **mutant) for r in ranks]
                assert wrong != right, (w, mutant, first)
                assert window_counts("cycle", eff, args, wrong) != window_counts("cycle", eff, args, right), (w, mutant, first)
    assert wrapping_binom(LMAX[4] - 1, 4) != math.comb(LMAX[4] - 1, 4) and wrapping_binom(1000, 4) == math.comb(1000, 4)


def gate_subset_counts(kind, eff, args, site_loc, n1, subset):
    """The counts of the restated tally over every kind assignment of one (one-operand picks, CNOT picks) subset."""
    ones, twos = subset
    masks = [gate_enumerate_ref.mask_words(eff, [site_loc[s]], 2)[0] for s in ones] + [gate_enumerate_ref.mask_words(eff, [site_loc[n1 + c]], 4)[0] for c in twos]
    words = np.zeros((1, eff.shape[2]), dtype=np.uint64)
    for table_of_pick in masks:                                               # every mask of every pick: the product, pick by pick
        words = (words[:, None, :] ^ table_of_pick[None, 1:, :]).reshape(-1, eff.shape[2])
    return list(TALLIES[kind](words, *args))


def test_a_wrong_rank_split_changes_the_gate_enumeration_references():
    """The gate rank split using C(n1, a) - 1: the subsets change, and with them the counts of the restated tally."""
    entry, kind, case = gpu_cases.GATE_ENUM_CASES["ec-ldr3"]
    for a, b in ((2, 2), (1, 3)):
        n1, n2 = gpu_cases.gate_enum_sites(a, b)
        eff, args = table(kind, case, n1 + 2 * n2)
        site_loc = gpu_cases.gate_enum_site_table(n1, n2)[0]
        c1 = math.comb(n1, a)
        for first, n in gpu_cases.gate_windows(n1, n2, a, b)[1:]:
            changed = 0
            for r in (first, first + n - 1):                                  # (below C(n1, a) - 1 the two splits agree)
                right = (enumerate_ref.unrank(n1, a, r % c1), enumerate_ref.unrank(n2, b, r // c1))
                assert gate_enumerate_ref.subsets_of_range(n1, n2, a, b, r, 1) == [tuple(map(tuple, right))]
                wrong = (enumerate_ref.unrank(n1, a, r % (c1 - 1)), enumerate_ref.unrank(n2, b, r // (c1 - 1)))
                changed += wrong != right and gate_subset_counts(kind, eff, args, site_loc, n1, wrong) != gate_subset_counts(kind, eff, args, site_loc, n1, right)
            assert changed >= 1, (a, b, first)


# ---- coverage -----------------------------------------------------------------------------------------------------------------------------

#  entry point: (the test of tests/test_gpu_limits.py that reaches it, the limit it reaches there)
COVERED = {
    "gf2_circuit_outcomes_dev": ("test_samplers_over_2048_segments", "2^20 locations, 1, 3 and 8 words"),
    "gf2_mc_circuit_decode": ("test_samplers_over_2048_segments", "2^20 locations, key layouts (1, 1) and (2, 2)"),
    "gf2_mc_circuit_run": ("test_samplers_over_2048_segments", "2^20 locations, key layouts (1, 1) and (2, 2)"),
    "gf2_mc_ec_decode": ("test_samplers_over_2048_segments", "2^20 locations, LDR 3 and 8, 6 rounds, 5 flag words"),
    "gf2_ft_outcomes_dev": ("test_samplers_over_2048_segments", "2^20 locations, LDR 8 and 16"),
    "gf2_mc_ft_decode": ("test_samplers_over_2048_segments", "2^20 locations, LDR 8 and 16, 15 steps"),
    "gf2_mc_circuit_decode_strata": ("test_strata_over_2_to_the_20_locations", "weight 16 of 2^20 locations"),
    "gf2_mc_ec_decode_strata": ("test_strata_over_2_to_the_20_locations", "weight 16 of 2^20 locations, LDR 8"),
    "gf2_mc_ft_decode_strata": ("test_strata_over_2_to_the_20_locations", "weight 16 of 2^20 locations, LDR 16"),
    "gf2_mc_ec_decode_gate_strata": ("test_gate_strata_over_2_to_the_20_locations", "(16, 0), (0, 16), (9, 7) of 2^20 / 2^19 sites"),
    "gf2_mc_ft_decode_gate_strata": ("test_gate_strata_over_2_to_the_20_locations", "(16, 0), (0, 16), (9, 7) of 2^20 / 2^19 sites"),
    "gf2_mc_ec_decode_gate": ("test_gate_monte_carlo_over_2_to_the_20_locations", "2048 / 0, 0 / 1024, 1025 / 512 segments"),
    "gf2_mc_ft_decode_gate": ("test_gate_monte_carlo_over_2_to_the_20_locations", "2048 / 0, 0 / 1024, 1025 / 512 segments"),
    "gf2_circuit_enumerate": ("test_enumerations_where_the_rank_space_is_largest", "C(Lmax(w), w) < 2^63, w = 2 .. 8"),
    "gf2_ec_enumerate": ("test_enumerations_where_the_rank_space_is_largest", "C(Lmax(w), w) < 2^63, LDR 3 and 8"),
    "gf2_ft_enumerate": ("test_enumerations_where_the_rank_space_is_largest", "C(Lmax(w), w) < 2^63, LDR 8 and 16"),
    "gf2_ec_enumerate_list": ("test_enumerations_where_the_rank_space_is_largest", "ranks above 2^62"),
    "gf2_ft_enumerate_list": ("test_enumerations_where_the_rank_space_is_largest", "ranks above 2^62"),
    "gf2_ec_gate_enumerate": ("test_gate_enumerations_where_the_rank_space_is_largest", "C(n1, a) C(n2, b) < 2^63, a + b <= 4"),
    "gf2_ft_gate_enumerate": ("test_gate_enumerations_where_the_rank_space_is_largest", "C(n1, a) C(n2, b) < 2^63, a + b <= 4"),
}


def test_cases_cover_the_limits():
    for entry_point, (test, limit) in COVERED.items():                       # the named test calls the Context method, which calls the entry point
        method = entry_point[len("gf2_"):]
        assert re.search(r"ctx\.%s\b" % method, inspect.getsource(getattr(gpu_cases, test))), (entry_point, test)
        assert re.search(r"lib\(\)\.%s\b" % entry_point, inspect.getsource(getattr(_native.Context, method))), entry_point
        assert hasattr(_native.lib(), entry_point) and limit
    cases = gpu_cases.SAMPLER_CASES
    at_top = {name: case for name, case in cases.items() if case[3] == TOP}
    width = lambda case: table(case[1], case[2], 64)[0].shape[2]
    assert {width(c) for c in at_top.values() if c[0] == "store"} == {1, 3, 8}
    assert {width(c) for c in at_top.values() if c[0] == "decode"} == {3, 5} and {c[2] for c in at_top.values() if c[0] == "decode"} == {(3, 3), (70, 70)}
    assert {(width(c),) + c[2] for c in at_top.values() if c[0] == "ec"} == {(3, 1, 1), (8, 2, 5), (8, 6, 1)}
    assert {(width(c), c[2][0]) for c in at_top.values() if c[0] == "ft"} == {(8, 7), (16, 15)}
    assert {(c[0], width(c), c[3]) for c in cases.values() if c[3] != TOP} == {(e, 3, L) for e in ("store", "ec") for L in (TOP - 1, TOP - 511)}
    assert gpu_cases.SAMPLES == 2048 + 37 and gpu_cases.FIRSTS == (777, (1 << 33) + 5) and {gpu_cases.sampler_first(n) for n in cases} == set(gpu_cases.FIRSTS)
    assert gpu_cases.STRATA_WEIGHTS == [1, 2, 16] and gpu_cases.STRATA_SAMPLES == (1 << 12) + 37 and gsr.MAX_WEIGHT == 16
    assert {c[0] for c in gpu_cases.STRATA_CASES.values()} == {"decode", "ec", "ft"}
    assert {width((None,) + c[1:]) for c in gpu_cases.STRATA_CASES.values()} == {3, 8, 16}
    assert set(gpu_cases.GATE_STRATA) == {(16, 0), (0, 16), (9, 7)} and all(a + b == 16 for a, b in gpu_cases.GATE_STRATA)
    assert gpu_cases.SITE_TABLES == ((TOP, 0), (0, TOP >> 1), ((TOP >> 1) + 2, (TOP >> 2) - 1)) and all(n1 + 2 * n2 == TOP for n1, n2 in gpu_cases.SITE_TABLES)
    assert [gpu_cases.gate_strata_of(*t) for t in gpu_cases.SITE_TABLES] == [[(16, 0)], [(0, 16)], [(16, 0), (0, 16), (9, 7)]]
    assert {(c[0], width((None,) + c[1:])) for c in gpu_cases.GATE_CASES.values()} == {("ec", 3), ("ec", 8), ("ft", 8), ("ft", 16)}
    assert gpu_cases.GATE_MC_SAMPLES == 1024 + 37
    assert set(gpu_cases.ENUM_RUNS) == {(n, w) for n in gpu_cases.ENUM_CASES for w in range(2, 9)} - {("ft-ldr16", 2), ("ft-ldr16", 3)}
    assert {(c[0], width((None,) + c[1:3])) for c in gpu_cases.ENUM_CASES.values()} == {("decode", 3), ("ec", 3), ("ec", 8), ("ft", 8), ("ft", 16)}
    assert set(gpu_cases.GATE_ENUM_STRATA) == {(2, 0), (0, 2), (3, 0), (2, 2), (4, 0), (0, 4), (1, 3)}
    assert {c[0] for c in gpu_cases.GATE_ENUM_CASES.values()} == {"ec", "ft"}
