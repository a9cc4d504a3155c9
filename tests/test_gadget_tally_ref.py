"""
tests/gadget_tally_ref.py tied to what exists, without a GPU, so that tests/test_gpu_sampler_instantiations.py does not stand on one leg.
Every comparison is exact.

  real gadgets     on the restatements' outcome words of the Steane one-round and five-round cycles, the Reed-Muller one-round cycle and
                   the Steane and Reed-Muller gate-free programs under the oracle sampler's faults, ec_tally / ft_tally with the
                   gadget's own tables give the counts of ec_ref.tally / ft_ref.tally (vectors of known errors, the code's table dicts)
  synthetic words  on the sampled words of every synthetic case of tests/test_gpu_sampler_instantiations.py, ec_tally / ft_tally give
                   the counts of gf2_ec_tally_host / gf2_ft_tally_host, and every case meets the conditions the GPU tests put on its
                   reference counts
  sampled_words    on a real cycle's effect table it gives the words of forward propagation
"""
import functools

import numpy as np
import pytest

from oracle import cpu_ref
from quantum_css_codes_amd import _native, ec_noise, ft_noise
from tests import ec_ref, ft_ref, gadget_tally_ref as ref, stream_ref
from tests import test_gpu_sampler_instantiations as gpu_cases
from tests.test_ft import STEANE, rm15_checks

SEED0 = 20261018 + 1300
#          code, rounds or logical gates, (p_x, p_y, p_z), samples
CYCLES = [("steane", 1, (0.004, 0.002, 0.004), 4096), ("steane", 5, (0.0008, 0.0004, 0.0008), 4096), ("rm15", 1, (0.001, 0.0005, 0.001), 4096)]
PROGRAMS = [("steane", "", (0.0004, 0.0002, 0.0004), 4096), ("rm15", "", (0.00024, 0.00012, 0.00024), 4096)]


@functools.lru_cache(maxsize=None)
def oracle_code(name):
    return cpu_ref.CSSCode(STEANE, STEANE) if name == "steane" else cpu_ref.CSSCode(*rm15_checks())


def restated_words(gadget, seed, p, count):
    faults = stream_ref.sampled_faults(gadget.locations, seed, 11, count, p)
    return gadget.outcome_words(*stream_ref.dense_faults(gadget.locations, *faults))


def test_field_names():
    assert ref.EC_FIELDS == ec_noise.EC_FIELDS == ec_ref.FIELDS and ref.FT_FIELDS == ft_noise.FT_FIELDS == ft_ref.FIELDS


@pytest.mark.parametrize("name, rounds, p, count", CYCLES, ids=lambda v: str(v) if isinstance(v, (str, int)) else "")
def test_cycle_rule_on_real_gadgets(name, rounds, p, count):
    code = oracle_code(name)
    circ, gadget = ec_noise.ECCircuit(code, rounds), ec_ref.Cycle(code, rounds)
    words = restated_words(gadget, SEED0 + rounds, p, count)
    want, _ = gadget.tally(words)
    print("\n%s-%d: %s" % (name, rounds, dict(zip(ref.EC_FIELDS, want))))
    assert 100 <= want[0] <= count - 100 and want[3] > 0 and (name == "steane" or want[4] + want[5] > 0)
    assert ref.ec_tally(words, rounds, *circ._tables()) == want
    # ... and the sampled words of the gadget's own effect table are the words of forward propagation
    assert np.array_equal(ref.sampled_words(circ.effects, SEED0 + rounds, 11, count, p), words)


@pytest.mark.parametrize("name, ops, p, count", PROGRAMS, ids=lambda v: str(v) if isinstance(v, str) else "")
def test_measurement_rule_on_real_gadgets(name, ops, p, count):
    code = oracle_code(name)
    prog, gadget = ft_noise.FTProgram(code, ops), ft_ref.Rewritten(code, ops)
    words = restated_words(gadget, SEED0 + 7, p, count)
    want, _ = gadget.tally(words)
    print("\n%s-%r: %s" % (name, ops, dict(zip(ref.FT_FIELDS, want))))
    # (wrong trials of the Reed-Muller program are some 60 in 2^18 samples: what it adds here is its unmatched x keys)
    assert 100 <= want[0] <= count - 100 and (want[2] > 0 if name == "steane" else want[5] > 0)
    assert ref.ft_tally(words, prog.nsteps, prog.measure_mask, *prog._tables()) == want


@pytest.mark.parametrize("case", gpu_cases.CYCLE_CASES, ids=lambda c: "rounds%d-ldr%d" % (c[0], 1 + c[0] + c[1]))
def test_cycle_rule_on_synthetic_words(case):
    for locations, eff, args, first, p, words, counts in gpu_cases.cycle_reference(case):
        gpu_cases.assert_not_vacuous(counts, ref.EC_FIELDS)
        assert _native.ec_tally_host(words, *args).tolist() == counts, (case, locations)


@pytest.mark.parametrize("case", gpu_cases.PROGRAM_CASES, ids=lambda c: "steps%d-ldr%d" % (c[0], c[0] + c[2]))
def test_measurement_rule_on_synthetic_words(case):
    one_trial = bin(case[1]).count("1") == 1
    for locations, eff, args, first, p, words, counts in gpu_cases.program_reference(case):
        gpu_cases.assert_not_vacuous(counts, ref.FT_FIELDS, one_trial)
        assert counts[6] > 0 and (counts[4] == 0) == one_trial
        assert _native.ft_tally_host(words, *args).tolist() == counts, (case, locations)


@pytest.mark.parametrize("name", list(gpu_cases.DENSE))
def test_dense_synthetic_words(name):
    eff, args, first, p, words, counts, faults = gpu_cases.dense_reference(name)
    print("\ndense %s: %.1f faults a sample, accepted %d of %d" % (name, faults, counts[0], gpu_cases.SAMPLES))
    gpu_cases.assert_dense(name, counts, faults)
    host = _native.ec_tally_host if gpu_cases.DENSE[name][0] else _native.ft_tally_host
    assert host(words, *args).tolist() == counts


@pytest.mark.parametrize("case", gpu_cases.DECODE_CASES, ids=lambda c: "r%d-%d" % c)
def test_decode_cases_are_not_vacuous(case):
    for locations, eff, tables, first, p, words, counts in gpu_cases.decode_reference(case):
        print("\ndecode %s at %d locations: %s" % (case, locations, counts))
        assert all(0 < v < gpu_cases.SAMPLES for v in counts)
        hist_z, hist_x = gpu_cases.weight_histograms(words, *case)
        assert int(hist_z.sum()) == int(hist_x.sum()) == gpu_cases.SAMPLES and hist_z[0] < gpu_cases.SAMPLES
