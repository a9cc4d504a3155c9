"""
Every template instantiation of the two direct samplers on synthetic effect tables: ec_kernel<LDR, STAGED> (csrc/gf2_ec.hip) through
gf2_mc_ec_decode, ft_kernel<LDR, EPI> (csrc/gf2_ft.hip) through gf2_mc_ft_decode and gf2_ft_outcomes_dev, and with them the store
epilogue of circuit_kernel (csrc/gf2_circuit.hip) at every width and its decode epilogue at every key layout.  tests/test_gpu_ec.py and
tests/test_gpu_ft.py reach only the widths the Steane and Reed-Muller gadgets have.  Every comparison of counts and words is exact,
against tests/gadget_tally_ref.py: the oracle's sampler run over the L locations, XOR of the effect rows, the tally rules restated on
plain dicts.  tests/test_gadget_tally_ref.py ties that restatement to tests/ec_ref.py, tests/ft_ref.py and the host statements, on
the very words used here, and needs no GPU.

  cycles          ec_kernel at LDR 3 .. 8, staged and unstaged, one, exactly one whole and three sampler segments, the two table
                  sizes on either side of the staging limit; circuit_kernel's store epilogue on the same tables
  programs        ft_kernel at LDR 8 .. 16 in both epilogues, 1 to 3 flag words, unmatched keys on both sides
  dense           several faults per 512-location segment (Floyd's map), 1100 locations.  Cycle (3, 1) and program (12, 0b10101, 1) at
                  a mean of 6 faults per segment: their one flag word takes four values (tests/test_gpu_gadget_strata.flag_words), so
                  however many faults there are a quarter of the samples is accepted -- the restatement rejects 62 % and 63 % at a
                  mean of 6, 73 % at 12 -- and "nine in ten rejected" is out of their reach at any mean; what is asserted of them is
                  1000 samples accepted, 1000 rejected and the mean number of faults.  Cycle (2, 5) and program (8, 0b00101010, 3),
                  with 5 and 3 flag words, at a mean of 12: there the restatement rejects 94 % and 91 % (at 10: 90 % and 87 %),
                  and nine in ten rejected with one accepted is asserted
  shards          two adjacent sample ranges add up to the whole
  narrow stores   circuit_kernel's store epilogue at 1 and 2 words, staged and through L2
  decode layouts  circuit_kernel's decode and histogram epilogues at (kwx, kwz) = (1, 1), (1, 2), (2, 1), (2, 2); gf2_mc_circuit_decode
                  takes r_1 = r_2 = 70, so (2, 2) is decoded as well as binned

Every case asserts on the restatement's counts that it is not vacuous before the device is asked.  Every test runs under a time limit
of its own, none provokes a fault.
"""
import contextlib
import faulthandler
import functools

import numpy as np
import pytest

from quantum_css_codes_amd import _native
from tests import gadget_tally_ref as ref
from tests.test_gpu_enumerate import synthetic
from tests.test_gpu_gadget_strata import CYCLE_CASES, PROGRAM_CASES, synthetic_cycle, synthetic_program

pytestmark = pytest.mark.gpu

SEED0 = 20261018 + 1200
TIME_LIMIT = 600                                                             # seconds per test
SAMPLES = (1 << 14) + 37                                                     # five workgroups, thirteen grid-stride trips per lane
FIRSTS = (777, (1 << 33) + 5)                                                # alternating over the cases
STAGE_LIMIT = 20480                                                          # bytes: effect tables up to this size are staged in LDS
CYCLE_R, PROGRAM_R = (5, 4), (4, 5)                                          # (r_1, r_2)
CYCLE_LOCATIONS, PROGRAM_LOCATIONS = (40, 512, 1100), (200, 512, 1100)       # one short, exactly one, three sampler segments
BOUNDARY_LOCATIONS = {(3, 1): (256, 257), (6, 1): (160, 161)}                # 2 L LDR 8 = STAGE_LIMIT, and one location more
DENSE_LOCATIONS = 1100
#        cycle or program, case, mean faults per 512-location segment, nine in ten rejected
DENSE = {"cycle-ldr5": (True, (3, 1), 6, False), "program-ldr13": (False, (12, 0b000000010101, 1), 6, False),
         "cycle-ldr8": (True, (2, 5), 12, True), "program-ldr11": (False, (8, 0b00101010, 3), 12, True)}
DECODE_LOCATIONS = (60, 700)
NARROW_LOCATIONS = (60, 700, 1300)                                            # one word of 700 locations is still staged, of 1300 not
#               r_1, r_2 -> LDR 3, 4, 4, 5
DECODE_CASES = [(3, 3), (64, 63), (40, 70), (70, 70)]


@pytest.fixture(autouse=True)
def own_time_limit():
    faulthandler.dump_traceback_later(TIME_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def rates(mean, per):
    """(p_x, p_y, p_z) with a mean of `mean` faults in every `per` locations."""
    return tuple(f * mean / per for f in (0.4, 0.2, 0.4))


def cycle_locations(case):
    return CYCLE_LOCATIONS + BOUNDARY_LOCATIONS.get(case, ())


# ---- the cases and their references: made once, shared, never modified -------------------------------------------------------------

def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def cycle_tables(case):
    """((locations, eff, args), ...) of a cycle case; args are (rounds, r1, keys1, flips1, r2, keys2, flips2)."""
    rounds, nflag = case
    rng = np.random.default_rng(SEED0 + 16 * rounds + nflag)
    out = []
    for locations in cycle_locations(case):
        eff, tables = synthetic_cycle(rng, *CYCLE_R, rounds, nflag, locations)
        frozen(eff, *tables)
        out.append((locations, eff, (rounds, CYCLE_R[0], tables[0], tables[1], CYCLE_R[1], tables[2], tables[3])))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def program_tables(case):
    """((locations, eff, args), ...) of a program case; args are (nsteps, measure_mask, r1, keys1, flips1, r2, keys2, flips2)."""
    nsteps, mask, nflag = case
    rng = np.random.default_rng(SEED0 + 32 * nsteps + nflag)
    out = []
    for locations in PROGRAM_LOCATIONS:
        eff, tables = synthetic_program(rng, *PROGRAM_R, nsteps, mask, nflag, locations)
        frozen(eff, *tables)
        out.append((locations, eff, (nsteps, mask, PROGRAM_R[0], tables[0], tables[1], PROGRAM_R[1], tables[2], tables[3])))
    return tuple(out)


def first_sample(cases, case):
    return FIRSTS[cases.index(case) % 2]


@functools.lru_cache(maxsize=None)
def cycle_reference(case):
    """((locations, eff, args, first, p, words, counts), ...): the restatement alone."""
    out = []
    for locations, eff, args in cycle_tables(case):
        first, p = first_sample(CYCLE_CASES, case), rates(2, locations)
        words, = frozen(ref.sampled_words(eff, SEED0, first, SAMPLES, p))
        out.append((locations, eff, args, first, p, words, ref.ec_tally(words, *args)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def program_reference(case):
    out = []
    for locations, eff, args in program_tables(case):
        first, p = first_sample(PROGRAM_CASES, case), rates(2, locations)
        words, = frozen(ref.sampled_words(eff, SEED0, first, SAMPLES, p))
        out.append((locations, eff, args, first, p, words, ref.ft_tally(words, *args)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def dense_reference(name):
    """(eff, args, first, p, words, counts, mean faults per sample) of a dense case."""
    cycle, case, mean, _ = DENSE[name]
    tables, tally = (cycle_tables(case), ref.ec_tally) if cycle else (program_tables(case), ref.ft_tally)
    (eff, args), = [(e, a) for locations, e, a in tables if locations == DENSE_LOCATIONS]
    first, p = FIRSTS[0], rates(mean, 512)
    words, = frozen(ref.sampled_words(eff, SEED0 + 1, first, SAMPLES, p))
    faults = ref.stream_ref.sampled_faults(DENSE_LOCATIONS, SEED0 + 1, first, SAMPLES, p)[0]
    return eff, args, first, p, words, tally(words, *args), float(np.diff(faults).mean())


def assert_not_vacuous(counts, fields, one_trial=False):
    """What a case's reference counts must show before the device is asked: samples accepted and rejected in number, and every count
    field well away from zero (a vote of one trial cannot be split)."""
    assert counts[0] >= 1000 and SAMPLES - counts[0] >= 1000, dict(zip(fields, counts))
    for name, value in zip(fields, counts):
        assert value >= 100 or (name == 'split_vote' and one_trial), dict(zip(fields, counts))


def assert_dense(name, counts, faults):
    """Of a dense case's reference: 1100 locations are 2.15 segments, so a sample has more than twice the segment's mean; nine in ten
    samples rejected and one accepted where the flag words allow it, else 1000 of each."""
    _, _, mean, nine_in_ten = DENSE[name]
    assert faults > 2 * mean, (name, faults)
    if nine_in_ten:
        assert counts[0] >= 1 and 10 * (SAMPLES - counts[0]) >= 9 * SAMPLES, (name, counts)
    else:
        assert counts[0] >= 1000 and SAMPLES - counts[0] >= 1000, (name, counts)


def decode_tally(words, r1, keys1, flips1, r2, keys2, flips2):
    """gf2_mc_circuit_decode's five counts restated: the words are [key_x: kwx] [key_z: kwz] [parity]; a key of several words is
    looked up as a tuple; a hit XORs the table's flip into the side's parity bit, a miss counts as uncorrectable."""
    kwx, kwz = (1 if r2 <= 63 else 2), (1 if r1 <= 63 else 2)
    tables = [{tuple(k): int(f) & 1 for k, f in zip(np.asarray(keys).reshape(-1, kw).tolist(), np.asarray(flips).tolist())}
              for keys, flips, kw in ((keys2, flips2, kwx), (keys1, flips1, kwz))]
    counts = [0] * 5
    for row in np.asarray(words).tolist():
        assert len(row) == kwx + kwz + 1
        flip = []
        for side, key in enumerate((tuple(row[:kwx]), tuple(row[kwx:kwx + kwz]))):
            bit = (row[-1] >> side) & 1
            if key in tables[side]:
                bit ^= tables[side][key]
            else:
                counts[3 + side] += 1
            flip.append(bit)
        counts[0] += flip[0]
        counts[1] += flip[1]
        counts[2] += flip[0] | flip[1]
    return counts


def weight_histograms(words, r1, r2):
    """gf2_mc_circuit_run's (hist_z, hist_x) in GF2_HIST_WEIGHT mode: samples binned by the number of set bits of each key."""
    kwx, kwz = (1 if r2 <= 63 else 2), (1 if r1 <= 63 else 2)
    bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8).reshape(len(words), -1, 8), axis=2).sum(axis=2)   # per word
    weight_x, weight_z = bits[:, :kwx].sum(axis=1), bits[:, kwx:kwx + kwz].sum(axis=1)
    return np.bincount(weight_z, minlength=r1 + 1).astype(np.uint64), np.bincount(weight_x, minlength=r2 + 1).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def decode_reference(case):
    """((locations, eff, tables, first, p, words, counts), ...) of a decode case; tables are (r1, keys1, flips1, r2, keys2, flips2)."""
    r1, r2 = case
    rng = np.random.default_rng(SEED0 + 64 * r1 + r2)
    out = []
    for locations in DECODE_LOCATIONS:
        eff, (keys1, flips1, keys2, flips2) = synthetic(rng, r1, r2, locations)
        first, p = first_sample(DECODE_CASES, case), rates(2, locations)
        words, = frozen(ref.sampled_words(eff, SEED0, first, SAMPLES, p))
        tables = (r1, keys1, flips1, r2, keys2, flips2)
        out.append((locations, eff, tables, first, p, words, decode_tally(words, *tables)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def narrow_tables(ldr):
    rng = np.random.default_rng(SEED0 + 1000 + ldr)
    return tuple((locations, frozen(rng.integers(0, 1 << 64, (locations, 2, ldr), dtype=np.uint64))[0]) for locations in NARROW_LOCATIONS)   # all 64 bits


# ---- coverage ----------------------------------------------------------------------------------------------------------------------

def test_cases_cover_the_kernel_instantiations():
    staged = {(1 + r + f, 2 * loc * (1 + r + f) * 8 <= STAGE_LIMIT) for r, f in CYCLE_CASES for loc in cycle_locations((r, f))}
    assert staged == {(ldr, s) for ldr in range(3, 9) for s in (True, False)}                       # ec_kernel<LDR, STAGED>
    assert {r for r, _ in CYCLE_CASES} == set(range(1, 7)) and {f for _, f in CYCLE_CASES} == {1, 3, 5}
    for case, pair in BOUNDARY_LOCATIONS.items():                                                   # the staging limit from both sides
        assert case in CYCLE_CASES and [2 * loc * (1 + sum(case)) * 8 - STAGE_LIMIT for loc in pair] == [0, 16 * (1 + sum(case))]
    assert {1 + sum(case) for case in BOUNDARY_LOCATIONS} == {5, 8}
    assert [-(-loc // 512) for loc in CYCLE_LOCATIONS] == [1, 1, 3] and CYCLE_LOCATIONS[1] % 512 == 0 and CYCLE_LOCATIONS[2] % 512
    # ft_kernel<LDR, EPI>: every program case runs both epilogues
    assert {s + f for s, _, f in PROGRAM_CASES} == set(range(8, 17)) and {f for _, _, f in PROGRAM_CASES} == {1, 2, 3}
    assert all(bin(m).count("1") % 2 == 1 and m >> s == 0 for s, m, _ in PROGRAM_CASES)
    assert any(bin(m).count("1") == 1 for _, m, _ in PROGRAM_CASES) and any(m & 1 for _, m, _ in PROGRAM_CASES)
    assert any(m >> (s - 1) for s, m, _ in PROGRAM_CASES)                                          # a measure bit at the top step
    # circuit_kernel's store epilogue: widths 1 and 2 of the narrow tables, 3 .. 8 of the cycle cases
    assert {1, 2} | {1 + r + f for r, f in CYCLE_CASES} == set(range(1, 9))
    assert all({2 * loc * ldr * 8 <= STAGE_LIMIT for loc in NARROW_LOCATIONS} == {True, False} for ldr in (1, 2))
    assert all((2 * loc * ldr * 8 <= STAGE_LIMIT) == (loc == 60) for loc in DECODE_LOCATIONS for ldr in (3, 4, 5))
    # ... and its decode epilogue: the four key layouts
    layouts = [((1 if r2 <= 63 else 2), (1 if r1 <= 63 else 2)) for r1, r2 in DECODE_CASES]
    assert layouts == [(1, 1), (1, 2), (2, 1), (2, 2)] and [1 + x + z for x, z in layouts] == [3, 4, 4, 5]
    assert all(case in (CYCLE_CASES if cycle else PROGRAM_CASES) for cycle, case, _, _ in DENSE.values())
    assert DENSE_LOCATIONS in CYCLE_LOCATIONS and DENSE_LOCATIONS in PROGRAM_LOCATIONS


# ---- the cycle: ec_kernel, and circuit_kernel's store epilogue -------------------------------------------------------------------------

@contextlib.contextmanager
def device_circuit(eff, ft=False):
    """(context, circuit) of an effect table; the circuit is freed whatever the test finds."""
    ctx = _native.default_context()
    circ = ctx.ft_circuit_create(eff) if ft else ctx.circuit_create(eff)
    try:
        yield ctx, circ
    finally:
        circ.free()


def stored_words(store, circ, seed, first, p, ldr):
    buf = _native.default_context().alloc(SAMPLES * ldr * 8).zero()
    try:
        store(circ, seed, first, SAMPLES, *p, buf, ldr)
        return buf.download((SAMPLES, ldr), np.uint64)
    finally:
        buf.free()


@pytest.mark.parametrize("case", CYCLE_CASES, ids=lambda c: "rounds%d-ldr%d" % (c[0], 1 + c[0] + c[1]))
def test_every_cycle_instantiation(case):
    for locations, eff, args, first, p, words, want in cycle_reference(case):
        assert_not_vacuous(want, ref.EC_FIELDS)
        with device_circuit(eff) as (ctx, circ):
            got = ctx.mc_ec_decode(circ, *args, SEED0, first, SAMPLES, *p)
            assert got.tolist() == want, (case, locations, dict(zip(ref.EC_FIELDS, got.tolist())), dict(zip(ref.EC_FIELDS, want)))
            stored = stored_words(ctx.circuit_outcomes_dev, circ, SEED0, first, p, eff.shape[2])
            assert np.array_equal(stored, words), (case, locations)


# ---- the program: ft_kernel in both epilogues ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", PROGRAM_CASES, ids=lambda c: "steps%d-ldr%d" % (c[0], c[0] + c[2]))
def test_every_measurement_instantiation(case):
    one_trial = bin(case[1]).count("1") == 1
    for locations, eff, args, first, p, words, want in program_reference(case):
        assert_not_vacuous(want, ref.FT_FIELDS, one_trial)
        assert want[6] > 0 and (want[4] == 0) == one_trial                   # unmatched z keys on the device; one trial, no split vote
        with device_circuit(eff, ft=True) as (ctx, circ):
            stored = stored_words(ctx.ft_outcomes_dev, circ, SEED0, first, p, eff.shape[2])
            assert np.array_equal(stored, words), (case, locations)
            got = ctx.mc_ft_decode(circ, *args, SEED0, first, SAMPLES, *p)
            assert got.tolist() == want, (case, locations, dict(zip(ref.FT_FIELDS, got.tolist())), dict(zip(ref.FT_FIELDS, want)))


# ---- several faults per segment ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(DENSE))
def test_dense_segments(name):
    eff, args, first, p, words, want, faults = dense_reference(name)
    assert_dense(name, want, faults)
    cycle = DENSE[name][0]
    with device_circuit(eff, ft=not cycle) as (ctx, circ):
        decode, store = (ctx.mc_ec_decode, ctx.circuit_outcomes_dev) if cycle else (ctx.mc_ft_decode, ctx.ft_outcomes_dev)
        assert decode(circ, *args, SEED0 + 1, first, SAMPLES, *p).tolist() == want
        assert np.array_equal(stored_words(store, circ, SEED0 + 1, first, p, eff.shape[2]), words)


# ---- shards ----------------------------------------------------------------------------------------------------------------------------

def test_adjacent_ranges_add_up():
    cut = 5003
    locations, eff, args, first, p, words, want = cycle_reference((2, 5))[2]                         # LDR 8, three segments
    with device_circuit(eff) as (ctx, circ):
        parts = [ctx.mc_ec_decode(circ, *args, SEED0, first + start, n, *p) for start, n in ((0, cut), (cut, SAMPLES - cut))]
        assert parts[0].tolist() == ref.ec_tally(words[:cut], *args) and (parts[0] + parts[1]).tolist() == want
    locations, eff, args, first, p, words, want = program_reference((13, 0b1010101010101, 2))[1]     # LDR 15, one whole segment
    with device_circuit(eff, ft=True) as (ctx, circ):
        parts = [ctx.mc_ft_decode(circ, *args, SEED0, first + start, n, *p) for start, n in ((0, cut), (cut, SAMPLES - cut))]
        assert parts[0].tolist() == ref.ft_tally(words[:cut], *args) and (parts[0] + parts[1]).tolist() == want


# ---- circuit_kernel's store epilogue at 1 and 2 words ---------------------------------------------------------------------------------

@pytest.mark.parametrize("ldr", [1, 2])
def test_narrow_store_widths(ldr):
    for locations, eff in narrow_tables(ldr):
        first, p = FIRSTS[ldr % 2], rates(2, locations)
        want = ref.sampled_words(eff, SEED0, first, SAMPLES, p)
        assert 1000 < np.count_nonzero(want.any(axis=1)) < SAMPLES and (want >> np.uint64(63)).any()
        with device_circuit(eff) as (ctx, circ):
            assert np.array_equal(stored_words(ctx.circuit_outcomes_dev, circ, SEED0, first, p, ldr), want), (ldr, locations)


# ---- circuit_kernel's decode and histogram epilogues at every key layout ------------------------------------------------------------

@pytest.mark.parametrize("case", DECODE_CASES, ids=lambda c: "r%d-%d" % c)
def test_every_decode_layout(case):
    r1, r2 = case
    for locations, eff, tables, first, p, words, want in decode_reference(case):
        assert (eff.nbytes <= STAGE_LIMIT) == (locations == 60)
        assert all(0 < v < SAMPLES for v in want), (case, locations, want)
        with device_circuit(eff) as (ctx, circ):
            got = ctx.mc_circuit_decode(circ, *tables, SEED0, first, SAMPLES, *p)
            assert got.tolist() == want, (case, locations, got.tolist(), want)
            hist_z, hist_x = ctx.mc_circuit_run(circ, r1, r2, SEED0, first, SAMPLES, *p, _native.HIST_WEIGHT)
            want_z, want_x = weight_histograms(words, r1, r2)
            assert np.array_equal(hist_z, want_z) and np.array_equal(hist_x, want_x), (case, locations)
            assert int(hist_z.sum()) == int(hist_x.sum()) == SAMPLES and np.count_nonzero(hist_z) > 2 and np.count_nonzero(hist_x) > 2
