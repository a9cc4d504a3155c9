"""
The circuit-fault kernels at the top of the ranges include/gf2hip.h accepts (DESIGN.md section 5g "Top of the accepted ranges"):
2^20 fault locations (2048 sampler segments of 512), strata of 16 faults, exact enumerations where C(L, w) is just below 2^63, effect rows
of 8 words (cycle) and 16 words (measurement).  Every comparison is exact: words byte for byte, counts integer for integer.

  (a) samplers      circuit_kernel, ec_kernel and ft_kernel over L = 2^20, 2^20 - 1 and 2^20 - 511 locations (a last segment of 512,
                    511 and 1), 2048 + 37 samples, against the oracle's sampler run over the L locations, XOR of the effect rows and the
                    tally rules of tests/gadget_tally_ref.py; the fault list is drawn once per (L, seed, first, rate), in chunks of 512
                    samples, and serves every table width
  (b) strata        gadget_strata_kernel and gate_strata_kernel at weights 1, 2, 16 and (a, b) = (16, 0), (0, 16), (9, 7) over 2^20
                    locations, against tests/strata_ref.py and tests/gate_strata_ref.py
  (c) gate MC       gate_mc_kernel over site tables of 2048 / 0, 0 / 1024 and 1025 / 512 segments, against tests/gate_mc_ref.py; the
                    tables are its own, shuffled so that a CNOT it draws takes the last two locations
  (d) enumerations  enumerate_kernel, gadget_enumerate_kernel, gadget_list_kernel and gate_enumerate_kernel at L = Lmax(w), the largest
                    L <= 2^20 with C(L, w) < 2^63, on three windows of ranks: the first, one across C(L - 1, w) where the top pick
                    becomes L - 1, the last.  The reference is the host statement; tests/test_limits.py ties every host statement used
                    here to its NumPy restatement on a shorter window of the same table, without a GPU (the restatements judge one
                    configuration at a time in Python: 10^6 configurations take them a minute, the host statement a fraction of a second)
  (e) refusals      one step beyond every limit gives GF2_E_ARG with the documented message

Every reference asserts that it is not vacuous before the device is asked; tests/test_limits.py asserts the same without a GPU, and
that each of eight wrong kernels would change a reference used here.  Tables and references are made once and shared (frozen arrays,
functools.lru_cache) and dropped when the module is done.  Every test runs under a time limit of its own, none provokes a fault.

Measured, one run, the references made first and the tests then run on the warm caches (host seconds on the MI355X machine's host;
device seconds are what the tests take there once the references exist, uploads of up to 256 MiB and the non-vacuity assertions
included).  An 8-core machine without a GPU needs 3.5 times the host seconds.

  group                 cases   host    device   slowest case on the device
  (a) samplers          14      9.1     0.51     0.25
  (b) strata             5      0.1     0.05     0.02
  (b) gate strata       12      0.3     0.19     0.03
  (c) gate MC           12      2.6     0.22     0.02
  (d) enumerations      33      5.0     2.34     0.56
  (d) gate enumerations 14      2.6     1.57     0.77
  (e) refusals          10      0.53 s in all, tables included; the slowest case 0.19 s

The whole module takes 28 to 30 s there.  The slowest test of tests/test_gpu_sampler_instantiations.py took 0.45 s in the same session
(test_every_cycle_instantiation[rounds1-ldr3], references included).  The slowest enumeration cases take longer than that on the device:
few subsets of many kinds each keep few lanes busy for long.  The windows of weight 8 are the smallest the cases allow (257 subsets), those
of (0, 4) are cut to 79 subsets (4 10^6 configurations).
"""
import concurrent.futures
import contextlib
import functools
import math

import numpy as np
import pytest

from quantum_css_codes_amd import _native, ec_noise, ft_noise
from tests import gadget_strata_ref, gadget_tally_ref as ref, gate_enumerate_ref, gate_mc_ref, gate_strata_ref as gsr, strata_ref, stream_ref
from tests.test_gpu_enumerate import synthetic
from tests.test_gpu_gadget_strata import synthetic_cycle, synthetic_program
from tests.test_gpu_sampler_instantiations import decode_tally, device_circuit, frozen, own_time_limit, rates, weight_histograms  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

SEED0 = 20261019 + 1400
TOP = 1 << 20                                                                # GF2_CIRCUIT_MAX_LOCATIONS
SEG = 512
HOST_THREADS = 8
FIRSTS = (777, (1 << 33) + 5)                                                # alternating over the cases
CYCLE_R, PROGRAM_R = (5, 4), (4, 5)                                          # (r_1, r_2)
EC, FT = ref.EC_FIELDS, ref.FT_FIELDS
#  rounds, flag words -> LDR 3, 8, 8
CYCLE_LDR3, CYCLE_LDR8, CYCLE_SIX_ROUNDS = (1, 1), (2, 5), (6, 1)
#  nsteps, measure_mask, flag words -> LDR 8, 16
PROGRAM_LDR8, PROGRAM_LDR16 = (7, 0b0010101, 1), (15, 0b001010101010101, 1)
DECODE_ONE, DECODE_TWO = (3, 3), (70, 70)                                    # (r_1, r_2): key layouts (1, 1) and (2, 2), LDR 3 and 5


# ---- tables: made once, shared, never modified ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def cycle_table(case, locations):
    """(eff, args) of a synthetic cycle; args are (rounds, r1, keys1, flips1, r2, keys2, flips2)."""
    rounds, nflag = case
    rng = np.random.default_rng([SEED0, 1, rounds, nflag, locations])
    eff, tables = synthetic_cycle(rng, *CYCLE_R, rounds, nflag, locations)
    frozen(eff, *tables)
    return eff, (rounds, CYCLE_R[0], tables[0], tables[1], CYCLE_R[1], tables[2], tables[3])


@functools.lru_cache(maxsize=None)
def program_table(case, locations):
    """(eff, args) of a synthetic program; args are (nsteps, measure_mask, r1, keys1, flips1, r2, keys2, flips2)."""
    nsteps, mask, nflag = case
    rng = np.random.default_rng([SEED0, 2, nsteps, nflag, locations])
    eff, tables = synthetic_program(rng, *PROGRAM_R, nsteps, mask, nflag, locations)
    frozen(eff, *tables)
    return eff, (nsteps, mask, PROGRAM_R[0], tables[0], tables[1], PROGRAM_R[1], tables[2], tables[3])


@functools.lru_cache(maxsize=None)
def decode_table(case, locations):
    """(eff, args) in the Monte-Carlo layout; args are (r1, keys1, flips1, r2, keys2, flips2)."""
    r1, r2 = case
    rng = np.random.default_rng([SEED0, 3, r1, r2, locations])
    eff, tables = synthetic(rng, r1, r2, locations)
    frozen(eff, *tables)
    return eff, (r1, tables[0], tables[1], r2, tables[2], tables[3])


@functools.lru_cache(maxsize=None)
def narrow_table(ldr, locations):
    rng = np.random.default_rng([SEED0, 4, ldr, locations])
    return frozen(rng.integers(0, 1 << 64, (locations, 2, ldr), dtype=np.uint64))[0], ()   # all 64 bits


TABLES = {"cycle": cycle_table, "program": program_table, "decode": decode_table, "narrow": narrow_table}
TALLIES = {"cycle": ref.ec_tally, "program": ref.ft_tally, "decode": decode_tally}


def table(kind, case, locations):
    return TABLES[kind](case, locations)


# ---- (a) the location-model samplers at 2048 segments --------------------------------------------------------------------------------

SAMPLES = 2048 + 37
CHUNK = 512                                                                  # the oracle's packed errors at n = 2^20 are 128 KiB per sample and component
LOCATIONS = (TOP, TOP - 1, TOP - 511)                                        # the last segment has 512, 511, 1 locations
MEAN, DENSE_MEAN = 2, 40                                                     # faults per sample
#  name: (entry point, table kind, table case, locations)
SAMPLER_CASES = {
    "store-1-word": ("store", "narrow", 1, TOP), "store-3-words": ("store", "cycle", CYCLE_LDR3, TOP), "store-8-words": ("store", "cycle", CYCLE_LDR8, TOP),
    "decode-1-1": ("decode", "decode", DECODE_ONE, TOP), "decode-2-2": ("decode", "decode", DECODE_TWO, TOP),
    "ec-ldr3": ("ec", "cycle", CYCLE_LDR3, TOP), "ec-ldr8-rounds2": ("ec", "cycle", CYCLE_LDR8, TOP), "ec-ldr8-rounds6": ("ec", "cycle", CYCLE_SIX_ROUNDS, TOP),
    "ft-ldr8": ("ft", "program", PROGRAM_LDR8, TOP), "ft-ldr16": ("ft", "program", PROGRAM_LDR16, TOP),
    "store-3-words-last511": ("store", "cycle", CYCLE_LDR3, TOP - 1), "ec-ldr3-last511": ("ec", "cycle", CYCLE_LDR3, TOP - 1),
    "store-3-words-last1": ("store", "cycle", CYCLE_LDR3, TOP - 511), "ec-ldr3-last1": ("ec", "cycle", CYCLE_LDR3, TOP - 511),
}
#  (locations, first sample) -> seed, picked on the CPU so that a sample of the mean-2 run has a fault in the last segment (a last
#  segment of one location is hit by one seed in 250)
SAMPLER_SEEDS = {(TOP, FIRSTS[0]): SEED0, (TOP, FIRSTS[1]): SEED0, (TOP - 1, FIRSTS[0]): SEED0, (TOP - 1, FIRSTS[1]): SEED0,
                 (TOP - 511, FIRSTS[0]): SEED0 + 46, (TOP - 511, FIRSTS[1]): SEED0 + 124}
#  ... and what the mean-40 run adds to that seed (the one location of a last segment is hit by one seed in 12)
DENSE_SEED_STEPS = {(TOP - 511, FIRSTS[0]): 4, (TOP - 511, FIRSTS[1]): 3}


def sampler_first(name):
    return FIRSTS[list(SAMPLER_CASES).index(name) % 2]


@functools.lru_cache(maxsize=None)
def fault_list(locations, seed, first, mean, count=SAMPLES):
    """((fault_first, location, kind), p) of samples [first, first + count) at a mean of `mean` faults per sample, drawn once for every
    table width, in chunks of CHUNK samples (tests/stream_ref.sampled_faults: the C oracle's sampler with n := L)."""
    p = rates(mean, locations)
    parts = [stream_ref.sampled_faults(locations, seed, first + at, min(CHUNK, count - at), p) for at in range(0, count, CHUNK)]
    fault_first = np.concatenate([[0]] + [np.diff(part[0]) for part in parts]).cumsum()
    return frozen(fault_first, np.concatenate([part[1] for part in parts]), np.concatenate([part[2] for part in parts])), p


def words_of_faults(eff, faults):
    """tests/gadget_tally_ref.sampled_words on a fault list drawn before: XOR of eff[l, 0] over the faults with an X component and of
    eff[l, 1] over those with a Z component."""
    fault_first, location, kind = faults
    sample = np.repeat(np.arange(len(fault_first) - 1), np.diff(fault_first))
    out = np.zeros((len(fault_first) - 1, eff.shape[2]), dtype=np.uint64)
    for component in (0, 1):
        has = ((kind >> component) & 1) == 1
        np.bitwise_xor.at(out, sample[has], eff[location[has], component])
    return out


@functools.lru_cache(maxsize=None)
def sampler_reference(name, dense=False):
    """(eff, args, seed, first, p, faults, words, counts or None) of a case at a mean of 2 faults per sample, or of 40."""
    entry, kind, case, locations = SAMPLER_CASES[name]
    eff, args = table(kind, case, locations)
    first = sampler_first(name)
    seed = SAMPLER_SEEDS[locations, first] + (DENSE_SEED_STEPS.get((locations, first), 1) if dense else 0)
    faults, p = fault_list(locations, seed, first, DENSE_MEAN if dense else MEAN)
    words, = frozen(words_of_faults(eff, faults))
    counts = None if entry == "store" or dense else TALLIES[kind](words, *args)
    return eff, args, seed, first, p, faults, words, counts


def segments_hit(faults, locations):
    """(distinct segments with a fault, faults in the last segment)."""
    segment = faults[1] // SEG
    return len(np.unique(segment)), int(np.count_nonzero(segment == (locations - 1) // SEG))


def assert_sparse_run(name, reference):
    """What a mean-2 reference must show before the device is asked: faults in at least 1000 distinct segments and one in the last;
    of a post-selected tally 200 samples accepted and 200 rejected, and every count field at least 10."""
    entry, kind, case, locations = SAMPLER_CASES[name]
    eff, args, seed, first, p, faults, words, counts = reference
    distinct, last = segments_hit(faults, locations)
    assert distinct >= 1000 and last >= 1, (name, distinct, last)
    assert 1000 < np.count_nonzero(words.any(axis=1)) < SAMPLES, name
    if entry in ("ec", "ft"):
        assert counts[0] >= 200 and SAMPLES - counts[0] >= 200 and min(counts) >= 10, (name, counts)
    elif entry == "decode":
        assert all(10 <= v <= SAMPLES - 10 for v in counts), (name, counts)


def assert_dense_run(name, reference):
    """Of a mean-40 reference: faults in every segment, and one at the last location or within the last 512."""
    locations = SAMPLER_CASES[name][3]
    faults = reference[5]
    assert segments_hit(faults, locations)[0] == -(-locations // SEG) == 2048 and int(faults[1].max()) >= locations - SEG, name
    assert len(faults[1]) > 30 * SAMPLES


def stored_words(store, circ, seed, first, count, p, ldr):
    buf = _native.default_context().alloc(count * ldr * 8).zero()
    try:
        store(circ, seed, first, count, *p, buf, ldr)
        return buf.download((count, ldr), np.uint64)
    finally:
        buf.free()


@pytest.mark.parametrize("name", list(SAMPLER_CASES))
def test_samplers_over_2048_segments(name):
    entry, kind, case, locations = SAMPLER_CASES[name]
    sparse = sampler_reference(name)
    assert_sparse_run(name, sparse)
    eff, args, seed, first, p, faults, words, want = sparse
    with device_circuit(eff, ft=entry == "ft") as (ctx, circ):
        if entry in ("store", "ft"):                                          # the store epilogues: sparse and dense
            dense = sampler_reference(name, True)
            assert_dense_run(name, dense)
            store = ctx.ft_outcomes_dev if entry == "ft" else ctx.circuit_outcomes_dev
            for _, _, seed_, first_, p_, _, words_, _ in (sparse, dense):
                assert np.array_equal(stored_words(store, circ, seed_, first_, SAMPLES, p_, eff.shape[2]), words_), (name, p_)
        if entry == "ec":
            got = ctx.mc_ec_decode(circ, *args, seed, first, SAMPLES, *p)
            assert got.tolist() == want, (name, dict(zip(EC, got.tolist())), dict(zip(EC, want)))
        elif entry == "ft":
            got = ctx.mc_ft_decode(circ, *args, seed, first, SAMPLES, *p)
            assert got.tolist() == want, (name, dict(zip(FT, got.tolist())), dict(zip(FT, want)))
        elif entry == "decode":
            got = ctx.mc_circuit_decode(circ, *args, seed, first, SAMPLES, *p)
            assert got.tolist() == want, (name, got.tolist(), want)
            hist_z, hist_x = ctx.mc_circuit_run(circ, case[0], case[1], seed, first, SAMPLES, *p, _native.HIST_WEIGHT)
            want_z, want_x = weight_histograms(words, *case)
            assert np.array_equal(hist_z, want_z) and np.array_equal(hist_x, want_x), name
            assert np.count_nonzero(hist_z) > 2 and np.count_nonzero(hist_x) > 2


# ---- (b) strata of exactly w faults over 2^20 locations ------------------------------------------------------------------------------

STRATA_SAMPLES = (1 << 12) + 37
STRATA_WEIGHTS = [1, 2, 16]
STRATA_KINDS = (1, 2, 1)
#  name: (entry point, table kind, table case)
STRATA_CASES = {"circuit": ("decode", "decode", DECODE_ONE), "ec-ldr3": ("ec", "cycle", CYCLE_LDR3), "ec-ldr8": ("ec", "cycle", CYCLE_LDR8),
                "ft-ldr8": ("ft", "program", PROGRAM_LDR8), "ft-ldr16": ("ft", "program", PROGRAM_LDR16)}
#  first sample -> seed, picked on the CPU so that Floyd's fallback fires in a sample of weight 16 (about 1e-4 per sample at L = 2^20)
STRATA_SEEDS = {FIRSTS[0]: SEED0 + 5, FIRSTS[1]: SEED0 + 3}


def floyd_candidates(seed, first, count, slot, tops):
    """(count, len(tops)) int64: Floyd's candidates t_k = ((v_k >> 32) (j_k + 1)) >> 32 of the stratified samplers before the
    fallback, j_k = tops[k]; slot is w + 1 for the strata over locations and 64 + 17 b + a + 1 for those over gates."""
    with np.errstate(over="ignore"):
        i = np.arange(count, dtype=np.uint64) + np.uint64(first)
        ks = strata_ref.mix64(np.uint64(seed) + np.uint64(strata_ref.GOLDEN) * (i + np.uint64(1)))
        d = strata_ref.mix64(ks + np.uint64(strata_ref.STREAM_MULT) * np.uint64(slot))
        out = np.zeros((count, len(tops)), dtype=np.int64)
        for k, j in enumerate(tops):
            v = strata_ref.mix64(d + np.uint64(strata_ref.GOLDEN) * np.uint64(k + 1))
            out[:, k] = ((v >> np.uint64(32)) * np.uint64(j + 1)) >> np.uint64(32)
    return out


def fallbacks(candidates, picks):
    """How many samples drew a candidate that an earlier pick (of the same columns) had taken."""
    fired = np.zeros(len(picks), dtype=bool)
    for k in range(1, picks.shape[1]):
        fired |= (picks[:, :k] == candidates[:, k:k + 1]).any(axis=1)
    return int(fired.sum())


def strata_fallbacks(seed, first, nb=TOP, w=16, count=STRATA_SAMPLES):
    pos, _ = strata_ref.stratum_draws(seed, first, count, nb, w, STRATA_KINDS)
    return fallbacks(floyd_candidates(seed, first, count, w + 1, [nb - w + k for k in range(w)]), pos), int(pos.max())


@functools.lru_cache(maxsize=None)
def strata_reference(name):
    """(eff, args, seed, first, [counts per weight])."""
    entry, kind, case = STRATA_CASES[name]
    eff, args = table(kind, case, TOP)
    first = FIRSTS[list(STRATA_CASES).index(name) % 2]
    seed = STRATA_SEEDS[first]
    counts = [list(TALLIES[kind](gadget_strata_ref.stratum_words(eff, seed, first, STRATA_SAMPLES, w, STRATA_KINDS), *args)) for w in STRATA_WEIGHTS]
    return eff, args, seed, first, counts


def assert_strata(name, reference):
    eff, args, seed, first, counts = reference
    fired, top = strata_fallbacks(seed, first)
    assert fired >= 1 and top >= TOP - 16, (name, fired, top)
    if STRATA_CASES[name][0] != "decode":
        assert all(10 <= c[0] <= STRATA_SAMPLES - 10 for c in counts) and all(max(c[1:]) > 0 for c in counts), (name, counts)
    else:
        assert all(0 < v < STRATA_SAMPLES for c in counts for v in c), (name, counts)


@pytest.mark.parametrize("name", list(STRATA_CASES))
def test_strata_over_2_to_the_20_locations(name):
    entry = STRATA_CASES[name][0]
    reference = strata_reference(name)
    assert_strata(name, reference)
    eff, args, seed, first, want = reference
    with device_circuit(eff, ft=entry == "ft") as (ctx, circ):
        run = {"decode": ctx.mc_circuit_decode_strata, "ec": ctx.mc_ec_decode_strata, "ft": ctx.mc_ft_decode_strata}[entry]
        got = run(circ, *args, seed, first, STRATA_WEIGHTS, [STRATA_SAMPLES] * len(STRATA_WEIGHTS), *(float(k) for k in STRATA_KINDS))
        assert got.tolist() == want, (name, got.tolist(), want)


# ---- the gate-level site tables of (b) and (c) -----------------------------------------------------------------------------------------

#  (n1, n2): n1 + 2 n2 = 2^20 locations; 2048 / 0, 0 / 1024 and 1025 / 512 segments per class, last segments of 512, 512, 2 and 511 sites
SITE_TABLES = ((TOP, 0), (0, TOP >> 1), ((TOP >> 1) + 2, (TOP >> 2) - 1))
SITE_TABLE_SEEDS = {SITE_TABLES[0]: SEED0, SITE_TABLES[1]: SEED0, SITE_TABLES[2]: SEED0 + 10}   # the mixed table: a CNOT takes the last two locations
GATE_STRATA = ((16, 0), (0, 16), (9, 7))
#  name: (entry point, table kind, table case)
GATE_CASES = {"ec-ldr3": ("ec", "cycle", CYCLE_LDR3), "ec-ldr8": ("ec", "cycle", CYCLE_LDR8), "ft-ldr8": ("ft", "program", PROGRAM_LDR8),
              "ft-ldr16": ("ft", "program", PROGRAM_LDR16)}
#  (n1, n2, a, b) -> (seed, first sample), picked on the CPU: Floyd's fallback fires, and where b > 0 the CNOT at the table's end is drawn
GATE_STRATA_SEEDS = {SITE_TABLES[0] + (16, 0): (SEED0 + 1, FIRSTS[0]), SITE_TABLES[1] + (0, 16): (SEED0 + 7, FIRSTS[1]),
                     SITE_TABLES[2] + (16, 0): (SEED0 + 1, FIRSTS[0]), SITE_TABLES[2] + (0, 16): (SEED0 + 4, FIRSTS[0]), SITE_TABLES[2] + (9, 7): (SEED0 + 15, FIRSTS[0])}


@functools.lru_cache(maxsize=None)
def site_table(n1, n2):
    """(site_loc, n1, n2) from gate_strata_ref.synthetic_sites, shuffled."""
    assert n1 + 2 * n2 == TOP
    site_loc, = frozen(gsr.synthetic_sites(n1, n2, np.random.default_rng(SITE_TABLE_SEEDS[n1, n2])))
    return site_loc, n1, n2


def end_site(sites):
    """The CNOT site whose first location is L - 2 (its target row is the table's last), or None."""
    site_loc, n1, n2 = sites
    at = np.flatnonzero(site_loc[n1:] == TOP - 2)
    return None if len(at) == 0 else n1 + int(at[0])


def gate_strata_of(n1, n2):
    return [(a, b) for a, b in GATE_STRATA if a <= n1 and b <= n2]


def by_two_operand(words, c, tally, nfields):
    """gate_strata_ref.gate_stratum_counts with a tally on plain tables: the (17, F) counts [c][field]."""
    out = np.zeros((gsr.MAX_WEIGHT + 1, nfields), dtype=np.uint64)
    for value in np.unique(c).tolist():
        out[value] = tally(words[c == value])
    return out


def gate_strata_fallbacks(sites, a, b, seed, first, count=STRATA_SAMPLES):
    """(samples whose fallback fired, samples that drew the table's end site)."""
    site_loc, n1, n2 = sites
    site, _ = gsr.gate_stratum_draws(seed, first, count, n1, n2, a, b)
    t = floyd_candidates(seed, first, count, 64 + 17 * b + a + 1, [n1 - a + k for k in range(a)] + [n2 - b + k for k in range(b)])
    fired = fallbacks(t[:, :a], site[:, :a]) + fallbacks(t[:, a:] + n1, site[:, a:])
    end = end_site(sites)
    return fired, 0 if end is None else int((site == end).any(axis=1).sum())


@functools.lru_cache(maxsize=None)
def gate_strata_reference(name, n1, n2):
    """(eff, args, sites, [(a, b, seed, first, counts (17, F))])."""
    entry, kind, case = GATE_CASES[name]
    eff, args = table(kind, case, TOP)
    sites = site_table(n1, n2)
    out = []
    for a, b in gate_strata_of(n1, n2):
        seed, first = GATE_STRATA_SEEDS[n1, n2, a, b]
        words, c = gsr.gate_stratum_words(eff, sites[0], n1, n2, seed, first, STRATA_SAMPLES, a, b)
        out.append((a, b, seed, first, by_two_operand(words, c, lambda w: TALLIES[kind](w, *args), len(EC if entry == "ec" else FT))))
    return eff, args, sites, out


def assert_gate_strata(reference):
    eff, args, sites, strata = reference
    site_loc, n1, n2 = sites
    assert (n2 == 0) == (end_site(sites) is None)
    for a, b, seed, first, counts in strata:
        fired, end = gate_strata_fallbacks(sites, a, b, seed, first)
        assert fired >= 1 and (end >= 1 or b == 0), (n1, n2, a, b, fired, end)
        accepted = int(counts[:, 0].sum())
        assert 10 <= accepted <= STRATA_SAMPLES - 10 and counts[:, 1:].sum() > 0 and not counts[b + 1:].any(), (n1, n2, a, b, accepted)


@pytest.mark.parametrize("n1, n2", SITE_TABLES, ids=lambda v: str(v))
@pytest.mark.parametrize("name", list(GATE_CASES))
def test_gate_strata_over_2_to_the_20_locations(name, n1, n2):
    entry = GATE_CASES[name][0]
    reference = gate_strata_reference(name, n1, n2)
    assert_gate_strata(reference)
    eff, args, sites, strata = reference
    with device_circuit(eff, ft=entry == "ft") as (ctx, circ):
        run = ctx.mc_ec_decode_gate_strata if entry == "ec" else ctx.mc_ft_decode_gate_strata
        for a, b, seed, first, want in strata:
            got = run(circ, *args, *sites, seed, first, [(a, b)], [STRATA_SAMPLES])
            assert np.array_equal(got[0], want), (name, n1, n2, a, b, got[0].tolist(), want.tolist())


# ---- (c) the direct gate-level Monte-Carlo ------------------------------------------------------------------------------------------------

GATE_MC_SAMPLES = 1024 + 37
#  (n1, n2) -> (seed, first sample), picked on the CPU so that both classes have a fault in their last segment (the mixed table's last
#  one-operand segment has two sites: one seed in 120)
GATE_MC_SEEDS = {SITE_TABLES[0]: (SEED0, FIRSTS[1]), SITE_TABLES[1]: (SEED0, FIRSTS[0]), SITE_TABLES[2]: (SEED0 + 1, FIRSTS[1])}
#  (n1, n2) -> the step of the site table's shuffle, picked on the CPU so that a CNOT site drawn with the seeds above takes the last two
#  locations (some 2100 of the 2^19 or 2^18 CNOT sites are drawn: one shuffle in 250 and in 360); the draw does not depend on the shuffle
GATE_MC_SHUFFLES = {SITE_TABLES[0]: 0, SITE_TABLES[1]: 145, SITE_TABLES[2]: 36}


@functools.lru_cache(maxsize=None)
def gate_mc_site_table(n1, n2):
    """(site_loc, n1, n2) from gate_strata_ref.synthetic_sites, shuffled: the Monte-Carlo's own tables."""
    assert n1 + 2 * n2 == TOP
    site_loc, = frozen(gsr.synthetic_sites(n1, n2, np.random.default_rng([SEED0, 6, n1, n2, GATE_MC_SHUFFLES[n1, n2]])))
    return site_loc, n1, n2


def gate_mc_rates(n1, n2):
    """A mean of 2 faults per class."""
    return (MEAN / n1 if n1 else 0.0), (MEAN / n2 if n2 else 0.0)


@functools.lru_cache(maxsize=None)
def gate_mc_fault_list(n1, n2):
    """(sample, site, kappa) of tests/gate_mc_ref.gate_mc_faults, drawn once per site table for every effect table."""
    seed, first = GATE_MC_SEEDS[n1, n2]
    return frozen(*gate_mc_ref.gate_mc_faults(seed, first, GATE_MC_SAMPLES, n1, n2, *gate_mc_rates(n1, n2)))


def words_of_gate_faults(eff, site_loc, faults, count):
    """tests/gate_mc_ref.gate_mc_words on faults drawn before."""
    sample, site, kappa = faults
    words = np.zeros((count, eff.shape[2]), dtype=np.uint64)
    loc = np.asarray(site_loc, dtype=np.int64)[site]
    for bit in range(4):
        has = ((kappa >> bit) & 1).astype(bool)
        np.bitwise_xor.at(words, sample[has], eff[loc[has] + (bit >> 1), bit & 1])
    return words


@functools.lru_cache(maxsize=None)
def gate_mc_reference(name, n1, n2):
    """(eff, args, sites, seed, first, rates, counts)."""
    entry, kind, case = GATE_CASES[name]
    eff, args = table(kind, case, TOP)
    sites = gate_mc_site_table(n1, n2)
    words = words_of_gate_faults(eff, sites[0], gate_mc_fault_list(n1, n2), GATE_MC_SAMPLES)
    return (eff, args, sites) + GATE_MC_SEEDS[n1, n2] + (gate_mc_rates(n1, n2), list(TALLIES[kind](words, *args)))


def assert_gate_mc(n1, n2, counts=None):
    """The faulty gates' first locations lie in at least 1000 distinct segments of 512 locations; each class has a fault in its last
    segment of sites, and in at least half of its segments; the CNOT whose target row is the table's last is drawn; of a tally 200
    samples accepted, 200 rejected and every count field at least 10."""
    sample, site, kappa = gate_mc_fault_list(n1, n2)
    sites = gate_mc_site_table(n1, n2)
    assert len(np.unique(sites[0][site] // SEG)) >= 1000, (n1, n2)
    for m, base in ((n1, 0), (n2, n1)):
        if m:
            segment = (site[(site >= base) & (site < base + m)] - base) // SEG
            assert 2 * len(np.unique(segment)) >= -(-m // SEG) and (segment == (m - 1) // SEG).any(), (n1, n2, base)
    end = end_site(sites)
    assert (n2 == 0) == (end is None) and (end is None or ((site == end) & (kappa >> 2 != 0)).any()), (n1, n2, end)   # with a kind on the target
    if counts is not None:
        assert counts[0] >= 200 and GATE_MC_SAMPLES - counts[0] >= 200 and min(counts) >= 10, (n1, n2, counts)


@pytest.mark.parametrize("n1, n2", SITE_TABLES, ids=lambda v: str(v))
@pytest.mark.parametrize("name", list(GATE_CASES))
def test_gate_monte_carlo_over_2_to_the_20_locations(name, n1, n2):
    entry = GATE_CASES[name][0]
    eff, args, sites, seed, first, p, want = gate_mc_reference(name, n1, n2)
    assert_gate_mc(n1, n2, want)
    with device_circuit(eff, ft=entry == "ft") as (ctx, circ):
        run = ctx.mc_ec_decode_gate if entry == "ec" else ctx.mc_ft_decode_gate
        got = run(circ, *args, *sites, seed, first, GATE_MC_SAMPLES, *p)
        assert got.tolist() == want, (name, n1, n2, got.tolist(), want)


# ---- (d) exact enumerations where C(L, w) is largest ------------------------------------------------------------------------------------

ENUM_WEIGHTS = tuple(range(2, 9))
LMAX = dict(zip(ENUM_WEIGHTS, (TOP, TOP, 121977, 16175, 4337, 1733, 887)))
EC_FLIPS = ec_noise.CLASS_FLIP_X | ec_noise.CLASS_FLIP_Z
#  name: (entry point, table kind, table case, the least weight: LDR 16 only from weight 4, to bound the table)
ENUM_CASES = {"circuit": ("decode", "decode", DECODE_ONE, 2), "ec-ldr3": ("ec", "cycle", CYCLE_LDR3, 2), "ec-ldr8": ("ec", "cycle", CYCLE_LDR8, 2),
              "ft-ldr8": ("ft", "program", PROGRAM_LDR8, 2), "ft-ldr16": ("ft", "program", PROGRAM_LDR16, 4)}


def largest_locations(w, below=1 << 63, top=TOP):
    """The largest L <= top with C(L, w) < below."""
    lo, hi = w, top + 1                                                      # C(lo, w) < below <= C(hi, w), or hi is beyond the top
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if math.comb(mid, w) < below else (lo, mid)
    return lo


def window_size(configurations):
    """Odd, at most 1025, and 250 000 configurations where that leaves a choice; at least 257 where 257 subsets are no more than
    4 10^6 configurations (every w <= 8, every gate stratum but (0, 4): 15^4 kinds a subset leave 79)."""
    n, most = min(1025, 250000 // configurations), 4 * 10**6 // configurations
    return max(min(257, most - (1 - most % 2)), n - (1 - n % 2))


def in_threads(calls):
    """The results of the calls, each on a thread of its own (ctypes releases the interpreter lock while a host statement runs)."""
    with concurrent.futures.ThreadPoolExecutor(HOST_THREADS) as pool:
        return [future.result() for future in [pool.submit(call) for call in calls]]


def windows(L, w):
    """[(first rank, count)]: the first ranks, a window across C(L - 1, w) where the top pick becomes L - 1, the last ranks."""
    total, n = math.comb(L, w), window_size(3**w)
    return [(0, n), (math.comb(L - 1, w) - n // 2, n), (total - n, n)]


ENUM_HOST = {"decode": _native.circuit_enumerate_host, "ec": _native.ec_enumerate_host, "ft": _native.ft_enumerate_host}
LIST_HOST = {"ec": _native.ec_enumerate_list_host, "ft": _native.ft_enumerate_list_host}
LIST_SELECTS = {"ec": (1, EC_FLIPS), "ft": (1, ft_noise.CLASS_WRONG)}


@functools.lru_cache(maxsize=None)
def enumerate_reference(name, w):
    """(eff, args, [(first, count, counts, {select: records})]) by the host statements."""
    entry, kind, case, _ = ENUM_CASES[name]
    L = LMAX[w]
    eff, args = table(kind, case, L)
    wins, selects = windows(L, w), LIST_SELECTS.get(entry, ())
    counted = in_threads([functools.partial(ENUM_HOST[entry], eff, *args, w, first, count) for first, count in wins])
    listed = in_threads([functools.partial(LIST_HOST[entry], eff, *args, w, first, count, select, 3**w * count) for first, count in wins for select in selects])
    out = []
    for k, (first, count) in enumerate(wins):
        counts, = frozen(counted[k])
        lists = {}
        for select, (found, records) in zip(selects, listed[k * len(selects):]):
            assert found == len(records) == int(counts[:, :, 0 if select == 1 else 3 if entry == "ec" else 1].sum()), (name, w, first, select)
            lists[select] = frozen(records)[0]
        out.append((first, count, counts, lists))
    return eff, args, out


def assert_enumeration(name, w, reference):
    from tests import enumerate_ref
    L = LMAX[w]
    total = math.comb(L, w)
    assert total < 1 << 63 and (L == TOP or math.comb(L + 1, w) >= 1 << 63)
    (first, n, _, _), (mid, _, _, _), (top, _, _, _) = reference[2]
    assert n % 2 == 1 and n >= 257 and n * 3**w <= 4 * 10**6 and first == 0 and top + n == total
    assert enumerate_ref.unrank(L, w, mid)[-1] == L - 2 and enumerate_ref.unrank(L, w, mid + n - 1)[-1] == L - 1
    assert enumerate_ref.unrank(L, w, top)[-1] == L - 1 and enumerate_ref.unrank(L, w, total - 1) == list(range(L - w, L))
    summed = sum(np.asarray(counts, dtype=object) for _, _, counts, _ in reference[2]).sum(axis=(0, 1))
    assert summed[0] > 0 and any(int(v) > 0 for v in summed[1:]), (name, w, summed)
    assert all(len(records) > 0 for _, _, _, lists in reference[2] for records in lists.values())
    if w >= 4:                                                                # ranks above 2^62 are listed
        assert top > 1 << 62 and all(int(records[:, 0].min()) > 1 << 62 for records in reference[2][2][3].values())


ENUM_RUNS = [(name, w) for name in ENUM_CASES for w in ENUM_WEIGHTS if w >= ENUM_CASES[name][3]]


@pytest.mark.parametrize("name, w", ENUM_RUNS)
def test_enumerations_where_the_rank_space_is_largest(name, w):
    entry, kind, case, least = ENUM_CASES[name]
    reference = enumerate_reference(name, w)
    assert_enumeration(name, w, reference)
    eff, args, wins = reference
    with device_circuit(eff, ft=entry == "ft") as (ctx, circ):
        count_fn = {"decode": ctx.circuit_enumerate, "ec": ctx.ec_enumerate, "ft": ctx.ft_enumerate}[entry]
        list_fn = {"ec": ctx.ec_enumerate_list, "ft": ctx.ft_enumerate_list}.get(entry)
        for first, count, want, lists in wins:
            got = count_fn(circ, *args, w, first, count)
            assert np.array_equal(got, want), (name, w, first, got.tolist(), want.tolist())
            for select, records in lists.items():
                found, listed = list_fn(circ, *args, w, first, count, select, len(records))
                assert found == len(records) and listed.dtype == records.dtype and listed.tobytes() == records.tobytes(), (name, w, first, select)


# ---- ... and under gate-level faults ----------------------------------------------------------------------------------------------------

GATE_ENUM_STRATA = ((2, 0), (0, 2), (3, 0), (2, 2), (4, 0), (0, 4), (1, 3))
GATE_ENUM_CASES = {"ec-ldr3": ("ec", "cycle", CYCLE_LDR3), "ft-ldr8": ("ft", "program", PROGRAM_LDR8)}
GATE_ENUM_HOST = {"ec": _native.ec_gate_enumerate_host, "ft": _native.ft_gate_enumerate_host}


def gate_enum_sites(a, b):
    """(n1, n2): one class empty where the stratum has no pick of it, else the largest n2 whose n1 = 2 n2 keeps C(n1, a) C(n2, b) below
    2^63 and n1 + 2 n2 within 2^20, and then the largest n1 that does: one site more of the class that binds is refused."""
    if b == 0:
        return largest_locations(a), 0
    if a == 0:
        return 0, largest_locations(b, top=TOP >> 1)
    lo, hi = b, (TOP >> 2) + 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if math.comb(2 * mid, a) * math.comb(mid, b) < 1 << 63 else (lo, mid)
    return largest_locations(a, below=-(-(1 << 63) // math.comb(lo, b)), top=TOP - 2 * lo), lo


@functools.lru_cache(maxsize=None)
def gate_enum_gates(n1, n2):
    """A gate list (kind, 0, 0) of n1 one-operand gates and n2 CNOTs in random order, the last gate a CNOT where there is one: its site
    table is tests/gate_enumerate_ref.sites', and the last CNOT site's target row is the table's last."""
    rng = np.random.default_rng([SEED0, 5, n1, n2])
    kinds = np.where(rng.permutation(n1 + n2) < n2, gate_enumerate_ref.CNOT, 2)
    if n2 and kinds[-1] != gate_enumerate_ref.CNOT:
        swap = np.flatnonzero(kinds == gate_enumerate_ref.CNOT)[-1]
        kinds[[swap, -1]] = kinds[[-1, swap]]
    gates = np.zeros((n1 + n2, 3), dtype=np.int64)
    gates[:, 0] = kinds
    return frozen(gates)[0]


@functools.lru_cache(maxsize=None)
def gate_enum_site_table(n1, n2):
    """(site_loc, n1, n2) of gate_enum_gates by a walk of its own: one location per operand in gate order, the one-operand sites first."""
    kinds = gate_enum_gates(n1, n2)[:, 0]
    width = np.where(kinds == gate_enumerate_ref.CNOT, 2, 1)
    start = np.cumsum(width) - width
    site_loc = np.concatenate((start[width == 1], start[width == 2])).astype(np.int32)
    return frozen(site_loc)[0], n1, n2


def gate_windows(n1, n2, a, b):
    """[(first rank, count)] of rank = r_s + C(n1, a) r_c: the first ranks, a window across the rank where the top pick of the last
    class with a pick becomes its last site (with a, b > 0 a multiple of C(n1, a): the one-operand part wraps, the CNOT part steps), a
    window across the first multiple of C(n1, a) where both classes have picks, the last ranks."""
    c1, c2 = math.comb(n1, a), math.comb(n2, b)
    n = window_size(3**a * 15**b)
    mid = c1 * math.comb(n2 - 1, b) if b else math.comb(n1 - 1, a)
    out = [(0, n), (mid - n // 2, n), (c1 * c2 - n, n)]
    if a and b:
        out.insert(1, (c1 - n // 2, n))
    return out


@functools.lru_cache(maxsize=None)
def gate_enumerate_reference(name, a, b):
    """(eff, args, sites, [(first, count, counts)]) by the host statements."""
    entry, kind, case = GATE_ENUM_CASES[name]
    n1, n2 = gate_enum_sites(a, b)
    eff, args = table(kind, case, n1 + 2 * n2)
    sites = gate_enum_site_table(n1, n2)
    wins = gate_windows(n1, n2, a, b)
    counted = in_threads([functools.partial(GATE_ENUM_HOST[entry], eff, *args, *sites, a + b, b, first, count) for first, count in wins])
    return eff, args, sites, [(first, count, frozen(counts)[0]) for (first, count), counts in zip(wins, counted)]


def assert_gate_enumeration(a, b, reference):
    eff, args, (site_loc, n1, n2), wins = reference
    L = n1 + 2 * n2
    assert L <= TOP and math.comb(n1, a) * math.comb(n2, b) < 1 << 63
    assert n1 >= 2 * n2 or a == 0
    if L < TOP:                                                               # bound by the product: one site more is refused
        assert math.comb(n1 + 1, a) * math.comb(n2 + (0 if a else 1), b) >= 1 << 63
    assert n2 == 0 or int(site_loc[n1 + n2 - 1]) == L - 2                     # the top CNOT pick of the top window reads the last row
    assert all(count % 2 == 1 and (count >= 257 or (a, b) == (0, 4) and count == 79) and count * 3**a * 15**b <= 4 * 10**6 for _, count, _ in wins)
    summed = sum(np.asarray(counts, dtype=object) for _, _, counts in wins).sum(axis=0)
    assert summed[0] > 0 and any(int(v) > 0 for v in summed[1:]), (a, b, summed)


@pytest.mark.parametrize("a, b", GATE_ENUM_STRATA, ids=lambda v: str(v))
@pytest.mark.parametrize("name", list(GATE_ENUM_CASES))
def test_gate_enumerations_where_the_rank_space_is_largest(name, a, b):
    entry = GATE_ENUM_CASES[name][0]
    reference = gate_enumerate_reference(name, a, b)
    assert_gate_enumeration(a, b, reference)
    eff, args, sites, wins = reference
    with device_circuit(eff, ft=entry == "ft") as (ctx, circ):
        run = ctx.ec_gate_enumerate if entry == "ec" else ctx.ft_gate_enumerate
        for first, count, want in wins:
            got = run(circ, *args, *sites, a + b, b, first, count)
            assert np.array_equal(got, want), (name, a, b, first, got.tolist(), want.tolist())


# ---- (e) one step beyond is refused ---------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def refused(text, who):
    with pytest.raises(_native.GF2Error, match=text) as err:
        yield
    assert err.value.code == _native.GF2_E_ARG and who in err.value.message, (text, who, err.value.message)


@pytest.mark.parametrize("w", [4, 5, 6, 7, 8])
def test_one_location_beyond_the_largest_rank_space_is_refused(w):
    L = LMAX[w] + 1
    text = r"C\(%d, %d\) subsets do not fit 63 bits" % (L, w)
    for kind, case, ft in (("decode", DECODE_ONE, False), ("cycle", CYCLE_LDR3, False), ("program", PROGRAM_LDR8, True)):
        eff, args = table(kind, case, L)
        with device_circuit(eff, ft=ft) as (ctx, circ):
            if kind == "decode":
                with refused(text, "gf2_circuit_enumerate"):
                    ctx.circuit_enumerate(circ, *args, w, 0, 1)
            elif kind == "cycle":
                with refused(text, "gf2_ec_enumerate"):
                    ctx.ec_enumerate(circ, *args, w, 0, 1)
                with refused(text, "gf2_ec_enumerate_list"):
                    ctx.ec_enumerate_list(circ, *args, w, 0, 1, 1, 8)
            else:
                with refused(text, "gf2_ft_enumerate"):
                    ctx.ft_enumerate(circ, *args, w, 0, 1)
                with refused(text, "gf2_ft_enumerate_list"):
                    ctx.ft_enumerate_list(circ, *args, w, 0, 1, 1, 8)


def one_site_more(a, b):
    """(n1, n2) of gate_enum_sites with one site more in the class that binds, where the product and not 2^20 locations binds."""
    n1, n2 = gate_enum_sites(a, b)
    return None if n1 + 2 * n2 == TOP else (n1 + 1, n2) if a else (n1, n2 + 1)


@pytest.mark.parametrize("a, b", [s for s in GATE_ENUM_STRATA if one_site_more(*s)], ids=lambda v: str(v))
def test_one_site_beyond_the_largest_gate_rank_space_is_refused(a, b):
    n1, n2 = one_site_more(a, b)
    assert math.comb(n1, a) * math.comb(n2, b) >= 1 << 63 and n1 + 2 * n2 <= TOP
    text = r"C\(%d, %d\) C\(%d, %d\) subsets do not fit 63 bits" % (n1, a, n2, b)
    sites = (np.concatenate((np.arange(n1), n1 + 2 * np.arange(n2))).astype(np.int32), n1, n2)
    for kind, case, ft in (("cycle", CYCLE_LDR3, False), ("program", PROGRAM_LDR8, True)):
        eff, args = table(kind, case, n1 + 2 * n2)
        with device_circuit(eff, ft=ft) as (ctx, circ):
            with refused(text, "gf2_ft_gate_enumerate" if ft else "gf2_ec_gate_enumerate"):
                (ctx.ft_gate_enumerate if ft else ctx.ec_gate_enumerate)(circ, *args, *sites, a + b, b, 0, 1)


def test_beyond_2_to_the_20_locations_and_beyond_weight_16_is_refused():
    ctx = _native.default_context()
    eff = np.zeros((TOP + 1, 2, 1), dtype="<u8")
    for create, who in ((ctx.circuit_create, "gf2_circuit_create"), (ctx.ft_circuit_create, "gf2_ft_circuit_create")):
        with refused(r"needs 1 <= locations <= 1048576 \(2\^20\), got 1048577", who):
            create(eff)
    for name, entry, who in (("circuit", ctx.mc_circuit_decode_strata, "gf2_mc_circuit_decode_strata"), ("ec-ldr3", ctx.mc_ec_decode_strata, "gf2_mc_ec_decode_strata"),
                             ("ft-ldr8", ctx.mc_ft_decode_strata, "gf2_mc_ft_decode_strata")):
        eff, args = table(*STRATA_CASES[name][1:], TOP)
        with device_circuit(eff, ft=name.startswith("ft")) as (ctx, circ):
            with refused(r"weight 17 outside \[0, min\(L = 1048576, 16\)\]", who):
                entry(circ, *args, SEED0, 0, [17], [10], 1.0, 1.0, 1.0)
    sites = site_table(*SITE_TABLES[2])
    for name, who in (("ec-ldr3", "gf2_mc_ec_decode_gate_strata"), ("ft-ldr8", "gf2_mc_ft_decode_gate_strata")):
        eff, args = table(*GATE_CASES[name][1:], TOP)
        with device_circuit(eff, ft=name.startswith("ft")) as (ctx, circ):
            for stratum in ((17, 0), (0, 17), (9, 8)):
                with refused(r"a \+ b <= 16 faulty gates", who):
                    (ctx.mc_ft_decode_gate_strata if name.startswith("ft") else ctx.mc_ec_decode_gate_strata)(circ, *args, *sites, SEED0, 0, [stratum], [10])


# ---- the references are dropped with the module ------------------------------------------------------------------------------------

CACHED = (cycle_table, program_table, decode_table, narrow_table, fault_list, sampler_reference, strata_reference, site_table, gate_strata_reference,
          gate_mc_site_table, gate_mc_fault_list, gate_mc_reference, enumerate_reference, gate_enum_gates, gate_enum_site_table, gate_enumerate_reference)


@pytest.fixture(scope="module", autouse=True)
def drop_the_references():
    yield
    for fn in CACHED:
        fn.cache_clear()
