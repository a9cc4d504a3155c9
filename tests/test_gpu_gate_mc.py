"""
The direct Monte-Carlo under gate-level faults on the GPU (DESIGN.md section 5e "Direct Monte-Carlo under gate-level faults"):
gate_mc_kernel (csrc/gf2_gate_mc.hip) through gf2_mc_ec_decode_gate / gf2_mc_ft_decode_gate, ECCircuit / FTProgram.gate_error_rates
and CSSCode.error_correct_gate_error_rates / logical_program_gate_error_rates.  Every comparison of counts is exact.

  host statement  the device against gf2_gate_outcomes_host followed by gf2_ec_tally_host / gf2_ft_tally_host
  instantiations  every (LDR, rule, staged) of the kernel on synthetic effect and site tables, classes of several segments wherever
                  the form allows them (a staged table has at most 426 locations: one segment per class)
  counts add      sample ranges in pieces past 2^40, more samples than one pass of the grid, p = 1 on 20 sites, p = 0
  state           the same counts after the workspace was filled, into a dirty counts_out, and after gf2_mc_ec_decode ran in
                  between with other rates
  statistics      2^30 samples: tiny gadgets against the brute-force sum, the Steane cycle against the merged strata
  entry points    the public methods; every argument error of the two entry points, one by one

Seeds are 20261020 + the case's index.  Every test runs under a time limit of its own, none provokes a fault.
"""
import faulthandler
import math

import numpy as np
import pytest

from oracle import exact_dist as ed
from quantum_css_codes_amd import _native, ec_noise, ft_noise, montecarlo
from quantum_css_codes_amd.montecarlo import GateStrata
from tests import gate_strata_ref as gsr
from tests.state_check import Layout
from tests.test_gate_mc import INDICATORS, TINY, TINY_P1, TINY_P2, brute_force, tiny_cycle
from tests.test_gpu_gate_strata import CYCLE_CASES, PROGRAM_CASES, synthetic_cycle, synthetic_program
from tests.test_gpu_strata import make_code

pytestmark = pytest.mark.gpu

SEED = 20261020
TIME_LIMIT = 600                                                             # seconds per test
EC, FT = ec_noise.EC_FIELDS, ft_noise.FT_FIELDS
STAGE_LIMIT = 20480                                                          # bytes: effect tables up to this size are staged in LDS
SAMPLES = 3001                                                               # no multiple of the 256 lanes of a workgroup
FIRST = 12345


@pytest.fixture(autouse=True)
def own_time_limit():
    faulthandler.dump_traceback_later(TIME_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def cycle(rounds):
    return ec_noise.circuit_for(make_code("steane"), rounds)


def program(name, ops):
    return ft_noise.program_for(make_code(name), ops)


# ---- 1: the device against the host statement ------------------------------------------------------------------------------------

GADGETS = {"cycle-1": lambda: cycle(1), "cycle-5": lambda: cycle(5), "steane-gate-free": lambda: program("steane", "")}
LAYOUT = {"cycle-1": (3, True), "cycle-5": (8, False), "steane-gate-free": (8, False)}


@pytest.mark.parametrize("case, name", list(enumerate(GADGETS)))
def test_device_counts_are_the_host_statement(case, name):
    gadget = GADGETS[name]()
    ldr, staged = LAYOUT[name]
    assert gadget.ldr == ldr and (gadget.effects.nbytes <= STAGE_LIMIT) == staged
    for p in (1e-3, 0.05, 0.5):
        got = gadget.gate_error_rates(SAMPLES, p, 1.5 * p, seed=SEED + case, first_sample=FIRST)
        want = gadget.gate_error_rates(SAMPLES, p, 1.5 * p, seed=SEED + case, first_sample=FIRST, host=True)
        assert got == want and got['samples'] == SAMPLES, (p, got, want)
        assert 0 < got['accepted'] or p > 0.01
    assert 0 < gadget.gate_error_rates(SAMPLES, 1e-3, 1.5e-3, seed=SEED + case, first_sample=FIRST)['accepted'] < SAMPLES


# ---- 2: every instantiation on synthetic effect and site tables --------------------------------------------------------------------

#                 locations: (n1, n2) with n1 + 2 n2 = locations; the rates of the two classes
CYCLE_SITES = {40: ((12, 14), (0.03, 0.04)), 1537: ((513, 512), (2e-3, 1e-3)), 2051: ((1, 1025), (0.5, 2e-3))}
PROGRAM_SITES = {1537: ((513, 512), (2e-3, 1e-3)), 2051: ((1, 1025), (0.5, 2e-3))}


def test_cases_cover_the_kernel_instantiations():
    staged = {(1 + r + f, 2 * loc * (1 + r + f) * 8 <= STAGE_LIMIT) for r, f in CYCLE_CASES for loc in CYCLE_SITES}
    assert staged == {(ldr, s) for ldr in range(3, 9) for s in (True, False)}
    assert {s + f for s, _, f in PROGRAM_CASES} == set(range(8, ft_noise.MAX_LDR + 1))
    assert all(n1 + 2 * n2 == loc for sites in (CYCLE_SITES, PROGRAM_SITES) for loc, ((n1, n2), _) in sites.items())
    assert STAGE_LIMIT // (2 * 8 * 3) < 512                                   # a staged table: one segment per class at most


def check_synthetic(device_fn, host_tally, nfields, eff, sites, rates, seed):
    got = device_fn(seed, FIRST, SAMPLES, *rates)
    want = montecarlo.host_gate_counts(eff, sites, host_tally, nfields, SAMPLES, *rates, seed, FIRST)
    assert got.shape == want.shape == (nfields,) and np.array_equal(got, want), (got.tolist(), want.tolist())
    return got


@pytest.mark.parametrize("index, case", list(enumerate(CYCLE_CASES)), ids=lambda c: str(c))
def test_every_cycle_instantiation(index, case):
    rounds, nflag = case
    ctx = _native.default_context()
    seed = SEED + 100 + index
    rng = np.random.default_rng(seed)
    r1, r2 = 5, 4
    for locations, ((n1, n2), rates) in CYCLE_SITES.items():
        eff, tables = synthetic_cycle(rng, r1, r2, rounds, nflag, locations)
        sites = (gsr.synthetic_sites(n1, n2, rng), n1, n2)
        circ = ctx.circuit_create(eff)
        args = (rounds, r1, tables[0], tables[1], r2, tables[2], tables[3])
        got = check_synthetic(lambda *tail: ctx.mc_ec_decode_gate(circ, *args, *sites, *tail),
                              lambda words: _native.ec_tally_host(words, *args), len(EC), eff, sites, rates, seed)
        assert 0 < got[0] < SAMPLES and got[3] > 0 and got[6:].sum() > 0, (case, locations, got.tolist())
        circ.free()


@pytest.mark.parametrize("index, case", list(enumerate(PROGRAM_CASES)), ids=lambda c: str(c))
def test_every_measurement_instantiation(index, case):
    nsteps, mask, nflag = case
    ctx = _native.default_context()
    seed = SEED + 200 + index
    rng = np.random.default_rng(seed)
    r1, r2 = 4, 5
    for locations, ((n1, n2), rates) in PROGRAM_SITES.items():
        eff, tables = synthetic_program(rng, r1, r2, nsteps, mask, nflag, locations)
        sites = (gsr.synthetic_sites(n1, n2, rng), n1, n2)
        circ = ctx.ft_circuit_create(eff)
        args = (nsteps, mask, r1, tables[0], tables[1], r2, tables[2], tables[3])
        got = check_synthetic(lambda *tail: ctx.mc_ft_decode_gate(circ, *args, *sites, *tail),
                              lambda words: _native.ft_tally_host(words, *args), len(FT), eff, sites, rates, seed)
        assert 0 < got[0] < SAMPLES and got[1] > 0 and got[5] > 0, (case, locations, got.tolist())
        circ.free()


# ---- 3: counts add -------------------------------------------------------------------------------------------------------------------

def test_counts_add():
    first, total = (1 << 40) + 777, 1 << 21                                  # 2^21 samples: every lane of the launch takes several
    for index, gadget in enumerate((cycle(2), program("steane", "X"))):
        seed = SEED + 300 + index
        whole = gadget.gate_error_rates(total, 2e-3, 3e-3, seed=seed, first_sample=first)
        cuts = ((first, 1), (first + 1, 40000), (first + 40001, total - 40001), (first + total, 0))
        parts = [gadget.gate_error_rates(n, 2e-3, 3e-3, seed=seed, first_sample=start) for start, n in cuts]
        for name in whole:
            assert sum(part[name] for part in parts) == whole[name], name
        assert 0 < whole['accepted'] < total
        assert parts[1] == gadget.gate_error_rates(40000, 2e-3, 3e-3, seed=seed, first_sample=first + 1, host=True)
        clean = gadget.gate_error_rates(SAMPLES, 0.0, 0.0, seed=seed)                                    # p = 0: accepted, nothing wrong
        assert clean['accepted'] == SAMPLES and not any(v for name, v in clean.items() if name not in ('accepted', 'samples'))


def test_every_site_faulty():
    """p = 1 on a table of 20 sites: every site is picked in every sample, Floyd's fallback at its limit."""
    n1, n2 = 9, 11
    ctx = _native.default_context()
    seed = SEED + 310
    rng = np.random.default_rng(seed)
    eff, tables = synthetic_cycle(rng, 3, 3, 1, 1, n1 + 2 * n2)
    eff[:, :, 2] = 0                                                          # no flags: every sample is accepted
    sites = (gsr.synthetic_sites(n1, n2, rng), n1, n2)
    circ = ctx.circuit_create(eff)
    args = (1, 3, tables[0], tables[1], 3, tables[2], tables[3])
    for rates in ((1.0, 1.0), (1.0, 0.0), (0.0, 1.0)):
        got = check_synthetic(lambda *tail: ctx.mc_ec_decode_gate(circ, *args, *sites, *tail),
                              lambda words: _native.ec_tally_host(words, *args), len(EC), eff, sites, rates, seed)
        assert got[0] == SAMPLES
    circ.free()


# ---- 4: state between calls --------------------------------------------------------------------------------------------------------

def test_counts_do_not_depend_on_what_earlier_calls_left():
    """The same call after the context's workspace was filled with 0xFF and with 0x00 and after gf2_mc_ec_decode made the context's
    segment tables for other rates, its counts_out a window of a dirty parent (tests/state_check.py): the promised F words equal the
    reference, the guards are untouched."""
    ctx = _native.Context(0)
    for index, (gadget, fields) in enumerate(((cycle(1), EC), (program("steane", ""), FT))):
        seed = SEED + 400 + index
        got = gadget.gate_error_rates(SAMPLES, 3e-3, 2e-3, seed=seed, first_sample=5, host=True)
        want = np.array([[got[name] for name in fields]], dtype=np.uint64)
        circ = ctx.circuit_create(gadget.effects) if fields is EC else ctx.ft_circuit_create(gadget.effects)
        site_loc, n1, n2, _ = gadget.gate_sites()
        keep, (t1, t2) = _native._enumerate_tables(*[gadget._tables()[k] for k in (1, 2, 4, 5)])
        head = (gadget.rounds,) if fields is EC else (gadget.nsteps, gadget.measure_mask)
        fn = _native.lib().gf2_mc_ec_decode_gate if fields is EC else _native.lib().gf2_mc_ft_decode_gate
        layout = Layout(1, len(fields))
        other = cycle(2)
        other_circ = ctx.circuit_create(other.effects)
        for fill in (None, 0xFF, 0x00, "other rates"):
            if fill == "other rates":
                ctx.mc_ec_decode(other_circ, other.rounds, *other._tables(), seed, 0, SAMPLES, 0.02, 0.01, 0.03)
            elif fill is not None:
                ctx.fill_workspace(fill)
            image = layout.image()
            _native.check(fn(ctx.handle, circ.handle, *head, gadget.code.r_1, *t1, gadget.code.r_2, *t2, site_loc.ctypes.data, n1, n2, seed, 5,
                             SAMPLES, 3e-3, 2e-3, image.ctypes.data + layout.lead))
            layout.check(image, want, what="counts_out after %r" % (fill,))
        other_circ.free()
        circ.free()
    ctx.close()


# ---- 5: statistics on the device -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case, table", list(enumerate(TINY)), ids=lambda v: str(v))
def test_tiny_gadget_is_exact_on_the_device(case, table):
    """2^30 samples of a tiny synthetic cycle at p1 = 0.2, p2 = 0.3 against the brute-force sum over every configuration
    (tests/test_gate_mc.py): z-test per indicator field, p >= 10^-6 two-sided."""
    n1, n2 = table
    eff, args, sites = tiny_cycle(case, n1, n2)
    want, _ = brute_force(eff, args, sites)
    ctx = _native.default_context()
    circ = ctx.circuit_create(eff)
    n = 1 << 30
    got = ctx.mc_ec_decode_gate(circ, *args, *sites, SEED + 500 + case, 0, n, TINY_P1, TINY_P2)
    circ.free()
    for col, name in enumerate(EC):
        if name in INDICATORS:
            f = min(1.0, max(0.0, want[col]))
            ed.assert_z("device %r %s" % (table, name), int(got[col]), n * f, n * f * (1.0 - f))


def test_steane_cycle_agrees_with_the_merged_strata():
    """The one-round Steane cycle at p1 = p2 = 1e-3: logical_any / accepted of 2^30 direct samples against the exact strata 0 .. 2
    merged with every sampled (a, b), 3 <= a + b <= 8, at 2^24 samples each; z = difference / sqrt(se_direct^2 + se_merged^2),
    p >= 10^-6 two-sided.  What the merge leaves out beyond weight 8 is below 1e-11, read from its own bounds."""
    code = make_code("steane")
    p = 1e-3
    n = 1 << 30
    direct = code.error_correct_gate_error_rates(n, p, p, rounds=1, seed=SEED + 510)
    strata = [(a, w - a) for w in range(3, 9) for a in range(w + 1)]
    merged = code.error_correct_gate_strata_exact([0, 1, 2]).merged(code.error_correct_gate_strata(strata, 1 << 24, rounds=1, seed=SEED + 511))
    odds = GateStrata.depolarising_odds(p, p)
    rate = merged.rate(odds, 'logical_any')
    d_low, d_high = merged.acceptance(odds)
    missing = (rate.upper - rate.lower) * d_high                              # T = (upper - lower) (D + T)
    assert 0.0 <= missing < 1e-11 and d_high - d_low < 1e-11, (missing, d_low, d_high)
    r = direct['logical_any'] / direct['accepted']
    se_direct = math.sqrt(r * (1.0 - r) / direct['accepted'])
    z = (r - rate.estimate) / math.sqrt(se_direct**2 + rate.stderr**2)
    ed.report("direct %.6e +- %.1e against merged %.6e +- %.1e (z)" % (r, se_direct, rate.estimate, rate.stderr), z, 1, ed.z_to_p(z), ed.z_to_p(z))
    assert ed.z_to_p(z) >= ed.P_LIMIT, (r, se_direct, rate.estimate, rate.stderr, z)
    # ... and the acceptance: the sampled strata hold 2e-3 of the probability at 2^24 samples each, so the merged value's own error
    # (about 2e-7) is a few percent of the direct one's standard error (about 1e-5) and is left out of the variance
    a = direct['accepted'] / n
    za = (a - d_low) / math.sqrt(d_low * (1.0 - d_low) / n)
    ed.report("direct acceptance %.8f against merged %.8f (z)" % (a, d_low), za, 1, ed.z_to_p(za), ed.z_to_p(za))
    assert ed.z_to_p(za) >= ed.P_LIMIT, (a, d_low, za)


# ---- 6: public entry points ----------------------------------------------------------------------------------------------------------

def test_public_entry_points():
    code = make_code("steane")
    for index, (got, gadget, fields) in enumerate((
            (code.error_correct_gate_error_rates(1 << 15, 2e-3, 3e-3, rounds=2, seed=SEED + 600, first_sample=9), ec_noise.circuit_for(code, 2), EC),
            (code.logical_program_gate_error_rates('X', 1 << 15, 2e-3, 3e-3, seed=SEED + 600, first_sample=9), ft_noise.program_for(code, 'X'), FT))):
        assert list(got) == list(fields) + ['samples'] and got['samples'] == 1 << 15 and 0 < got['accepted'] < 1 << 15
        assert got == gadget.gate_error_rates(1 << 15, 2e-3, 3e-3, seed=SEED + 600, first_sample=9, host=True)
        alone = montecarlo.gate_error_rates_sharded(gadget, 1 << 15, 2e-3, 3e-3, seed=SEED + 600, first_sample=9)   # no process group: one shard
        assert alone == got
    assert code.error_correct_gate_error_rates(100, 1e-3, 1e-3, host=True)['samples'] == 100


# ---- 7: refusals -----------------------------------------------------------------------------------------------------------------------

NAN = float("nan")


def test_refusals_of_the_cycle_entry_point():
    code = make_code("steane")
    ctx = _native.default_context()
    circ = ec_noise.circuit_for(code, 1)
    r1, keys1, flips1, r2, keys2, flips2 = tables = circ._tables()
    site_loc, n1, n2, _ = circ.gate_sites()
    dev = circ.device()

    def call(circuit=dev, rounds=1, tables=tables, sites=(site_loc, n1, n2), first=0, count=10, p1=0.01, p2=0.01):
        return ctx.mc_ec_decode_gate(circuit, rounds, *tables, *sites, SEED, first, count, p1, p2)

    rng = np.random.default_rng(SEED + 700)
    five = rng.integers(0, 1 << 62, (30, 2, 5)).astype("<u8")              # the Monte-Carlo layout is no cycle: its effects leave the layout
    five_dev = ctx.circuit_create(five)
    program_dev = ft_noise.program_for(code, "XXX").device()                 # 11 words
    overlap = site_loc.copy()
    overlap[1] = overlap[0]
    for fn, text in ((lambda: call(tables=(32, keys1, flips1, r2, keys2, flips2)), "<= 31"), (lambda: call(tables=(r1, keys1, flips1, 0, keys2, flips2)), "<= 31"),
                     (lambda: call(rounds=0), "rounds <= 6"), (lambda: call(rounds=7), "rounds <= 6"),
                     (lambda: call(program_dev, rounds=6), "ldr <= 8"), (lambda: call(rounds=2), "rounds need"),
                     (lambda: call(five_dev, rounds=2), "beyond"),
                     (lambda: call(tables=(r1, np.append(keys1, keys1[:1]), np.append(flips1, 0), r2, keys2, flips2)), "twice"),
                     (lambda: call(sites=(overlap, n1, n2)), "no partition"), (lambda: call(sites=(site_loc[1:], n1 - 1, n2)), "no partition"),
                     (lambda: call(p1=-1e-9), "0 <= p_1, p_2 <= 1"), (lambda: call(p1=1.0 + 1e-9), "0 <= p_1, p_2 <= 1"),
                     (lambda: call(p1=NAN), "0 <= p_1, p_2 <= 1"), (lambda: call(p2=-1.0), "0 <= p_1, p_2 <= 1"),
                     (lambda: call(p2=1.5), "0 <= p_1, p_2 <= 1"), (lambda: call(p2=NAN), "0 <= p_1, p_2 <= 1"),
                     (lambda: call(count=-1), "count >= 0"), (lambda: call(first=-1), "first_sample >= 0")):
        with pytest.raises(_native.GF2Error, match=text) as err:
            fn()
        assert err.value.code == _native.GF2_E_ARG and "gf2_mc_ec_decode_gate:" in err.value.message, text
    five_dev.free()
    assert call(count=0).shape == (8,) and not call(count=0).any()
    for bad in (lambda: circ.gate_error_rates(10, 1.5, 0.1), lambda: circ.gate_error_rates(-1, 0.1, 0.1), lambda: circ.gate_error_rates(10, 0.1, 0.1, first_sample=-1)):
        with pytest.raises(_native.GF2Error):
            bad()


def test_refusals_of_the_measurement_entry_point():
    code = make_code("steane")
    ctx = _native.default_context()
    prog = ft_noise.program_for(code, "")
    r1, keys1, flips1, r2, keys2, flips2 = tables = prog._tables()
    site_loc, n1, n2, _ = prog.gate_sites()
    dev = prog.device()

    def call(circuit=dev, nsteps=prog.nsteps, mask=prog.measure_mask, tables=tables, sites=(site_loc, n1, n2), first=0, count=10, p1=0.01, p2=0.01):
        return ctx.mc_ft_decode_gate(circuit, nsteps, mask, *tables, *sites, SEED, first, count, p1, p2)

    assert (prog.ldr, prog.nsteps, prog.measure_mask) == (8, 6, 0b010101)
    cycle_dev = ec_noise.circuit_for(code, 1).device()                       # the cycle's 3 words are no program
    rng = np.random.default_rng(SEED + 701)
    wide = ctx.ft_circuit_create(rng.integers(0, 1 << 62, (30, 2, 8)).astype("<u8"))
    swapped = site_loc.copy()
    swapped[[0, n1]] = swapped[[n1, 0]]                                      # a CNOT where a one-operand gate was: its two locations overlap
    for fn, text in ((lambda: call(tables=(r1, keys1, flips1, 32, keys2, flips2)), "<= 31"), (lambda: call(cycle_dev, nsteps=2, mask=0b01), "8 <= ldr"),
                     (lambda: call(nsteps=0, mask=0), "nsteps >= 1"), (lambda: call(nsteps=8, mask=0b010101), "F >= 1"),
                     (lambda: call(mask=1 << 6), "at or above nsteps"), (lambda: call(mask=0b010100), "odd number"),
                     (lambda: call(wide), "beyond"),
                     (lambda: call(tables=(r1, keys1, flips1, r2, np.append(keys2, keys2[:1]), np.append(flips2, 0))), "twice"),
                     (lambda: call(sites=(swapped, n1, n2)), "no partition"), (lambda: call(sites=(site_loc, n1 + 1, n2 - 1)), "no partition"),
                     (lambda: call(p1=-1e-9), "0 <= p_1, p_2 <= 1"), (lambda: call(p1=2.0), "0 <= p_1, p_2 <= 1"),
                     (lambda: call(p1=NAN), "0 <= p_1, p_2 <= 1"), (lambda: call(p2=-1e-9), "0 <= p_1, p_2 <= 1"),
                     (lambda: call(p2=1.0 + 1e-9), "0 <= p_1, p_2 <= 1"), (lambda: call(p2=NAN), "0 <= p_1, p_2 <= 1"),
                     (lambda: call(count=-1), "count >= 0"), (lambda: call(first=-1), "first_sample >= 0")):
        with pytest.raises(_native.GF2Error, match=text) as err:
            fn()
        assert err.value.code == _native.GF2_E_ARG and "gf2_mc_ft_decode_gate:" in err.value.message, text
    wide.free()
    assert call(count=0).shape == (7,) and not call(count=0).any()
