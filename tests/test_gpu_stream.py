"""
The streamed route on the GPU (quantum_css_codes_amd/stream_noise.py, csrc/gf2_stream.hip).  Every comparison
is exact.

Where the resident kernels accept the size, the streamed kernel must give their words and their counts on the same (seed,
first_sample): the sampler is the same, draw for draw.  Beyond their limits the reference is the restatement alone (tests/ec_ref.py,
tests/ft_ref.py behind tests/stream_ref.py): the faults of the oracle's sampler over the L locations, forward propagation,
quil_classical_correct on vectors of known errors.  A case's reference is computed once and shared by its tests.

The cases are the smallest shapes at which stream_kernel takes another path: a block boundary inside a sampler segment (Steane, 330
locations per block) and blocks that span several segments (Reed-Muller, 804); tables staged in LDS below and above 64 KB and read
through L2 (the Reed-Muller program's six types, 190 KB); one, two and three flag words, flag rows that straddle a word; NONE, EC, MEASURE and FINAL steps; several faults per
segment (Floyd's map) with nearly every sample rejected; no fault at all; and a run of 1000 rounds, 645 segments.
"""
import functools

import numpy as np
import pytest

from quantum_css_codes_amd import _native, ec_noise, ft_noise, stream_noise
from quantum_css_codes_amd.css_code import CSSCode
from tests import stream_ref
from tests.test_gpu_ec import checks_of

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def make_code(name):
    h1, h2, cap = checks_of(name)
    return CSSCode(h1, h2, max_table_weight=cap)


@functools.lru_cache(maxsize=None)
def streamed(name, what, key):
    return stream_noise.stream_for(make_code(name), what, key)


@functools.lru_cache(maxsize=None)
def restated(name, what, key):
    code = make_code(name)
    return stream_ref.cycle_reference(code, *key) if what == "cycle" else stream_ref.program_reference(code, key)


#        code, what, key, (p_x, p_y, p_z), samples, seed, first_sample
RESIDENT_CASES = {
    "steane-2": ("steane", "cycle", (2, False), (0.002, 0.001, 0.002), 100003, 2, 5),       # a block boundary inside the second segment
    "steane-5": ("steane", "cycle", (5, False), (0.001, 0.0005, 0.001), 100000, 4, 1 << 33),
    "rm15-3": ("rm15", "cycle", (3, False), (0.001, 0.0005, 0.001), 100000, 6, 7),          # a block spans two or three segments
    "program": ("steane", "program", (), (0.001, 0.0005, 0.001), 100000, 7, 0),             # three types, 30 KB: staged
    "program-XY": ("steane", "program", ("X", "Y"), (0.0008, 0.0004, 0.0008), 100000, 8, 3),  # five types, 62 KB: staged above 64 KB of LDS
}
BEYOND_CASES = {
    "steane-7": ("steane", "cycle", (7, False), (0.0008, 0.0004, 0.0008), 100000, 1, 0),    # two flag words
    "steane-12": ("steane", "cycle", (12, False), (0.0004, 0.0002, 0.0004), 100000, 2, 1 << 33),   # three flag words
    "rm15-5": ("rm15", "cycle", (5, False), (0.0003, 0.0002, 0.0003), 100000, 3, 7),        # refused by the resident route
    "X*8": ("steane", "program", tuple("X" * 8), (0.0004, 0.0002, 0.0004), 100000, 4, 0),   # refused by the resident route
    "rm15-XYZ": ("rm15", "program", ("X", "Y", "Z"), (0.0003, 0.0002, 0.0003), 50000, 6, 0),   # six types, 190 KB: read through L2
    "steane-7-dense": ("steane", "cycle", (7, False), (0.01, 0.0, 0.02), 100000, 5, 0),     # several faults per segment, nearly all rejected
}


def resident_of(name, what, key):
    code = make_code(name)
    return ec_noise.circuit_for(code, *key) if what == "cycle" else ft_noise.program_for(code, key)


@pytest.mark.parametrize("case", sorted(RESIDENT_CASES))
def test_words_and_counts_equal_the_resident_kernels(case):
    name, what, key, p, count, seed, first = RESIDENT_CASES[case]
    gadget, resident = streamed(name, what, key), resident_of(name, what, key)
    assert (gadget.num_locations, gadget.ldw) == (resident.num_locations, resident.ldr)
    want_words = resident.outcomes(count, *p, seed=seed, first_sample=first)
    got_words = gadget.outcomes(count, *p, seed=seed, first_sample=first)
    got_words = gadget.to_cycle_layout(got_words) if what == "cycle" else gadget.to_program_layout(got_words)
    assert got_words.shape == want_words.shape and np.array_equal(got_words, want_words)
    want = resident.logical_error_rates(count, *p, seed=seed, first_sample=first) if what == "cycle" else \
        resident.measurement_error_rates(count, *p, seed=seed, first_sample=first)
    print("\n%s: %s" % (case, want))
    assert want['accepted'] >= 500 and count - want['accepted'] >= 500
    assert (want['logical_x'] >= 10 and want['logical_z'] >= 10) if what == "cycle" else (want['trial_wrong'] >= 10 and want['wrong'] >= 1)
    assert gadget.error_rates(count, *p, seed=seed, first_sample=first) == want


@functools.lru_cache(maxsize=None)
def reference(case):
    """(stream-layout words, the dict of counts) of a case under the restatement alone; computed once, never modified."""
    name, what, key, p, count, seed, first = BEYOND_CASES[case]
    ref = restated(name, what, key)
    words = ref.words(seed, first, count, p)
    words.setflags(write=False)
    return words, ref.tally(words)


@pytest.mark.parametrize("case", sorted(BEYOND_CASES))
def test_words_beyond_the_resident_limits_equal_the_restatement(case):
    name, what, key, p, count, seed, first = BEYOND_CASES[case]
    gadget, ref = streamed(name, what, key), restated(name, what, key)
    assert (gadget.num_locations, gadget.ldw) == (ref.locations, ref.ldw)
    want, _ = reference(case)
    got = gadget.outcomes(count, *p, seed=seed, first_sample=first)
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("case", sorted(BEYOND_CASES))
def test_counts_beyond_the_resident_limits_equal_the_restatement(case):
    name, what, key, p, count, seed, first = BEYOND_CASES[case]
    gadget = streamed(name, what, key)
    _, want = reference(case)
    print("\n%s: %s" % (case, want))
    if case.endswith("dense"):
        assert want['accepted'] <= count // 100, "the dense case must reject nearly everything"
    else:
        flips = want['logical_any'] if what == "cycle" else want['trial_wrong']
        assert want['accepted'] >= 500 and count - want['accepted'] >= 500 and flips >= 10
    assert gadget.error_rates(count, *p, seed=seed, first_sample=first) == want


def test_cases_cover_the_kernel_paths():
    assert [streamed("steane", "cycle", (r, False)).flag_words for r in (2, 5, 7, 12)] == [1, 2, 2, 3]
    assert streamed("steane", "cycle", (2, False)).types[0].num_locations == 330 and streamed("rm15", "cycle", (3, False)).types[0].num_locations == 804
    fixed = 2 * 513 * 8 + 256 * 17 * 4 + 64                                          # the CDF tables, the taken maps, the counts
    sizes = {case: streamed(*RESIDENT_CASES[case][:3]).type_eff.nbytes for case in RESIDENT_CASES}
    sizes.update({case: streamed(*BEYOND_CASES[case][:3]).type_eff.nbytes for case in BEYOND_CASES})
    assert sizes["steane-2"] + fixed < sizes["program"] + fixed < 64 * 1024 < sizes["program-XY"] + fixed < 160 * 1024     # staged, below and above 64 KB
    assert sizes["rm15-3"] + fixed < 160 * 1024 < sizes["rm15-XYZ"] and len(streamed("steane", "program", ("X", "Y")).types) == 5
    for name, rounds in (("steane", 7), ("steane", 12), ("rm15", 5)):                 # the resident route refuses these
        with pytest.raises(ValueError):
            ec_noise.error_correct_gates(make_code(name), rounds)
    with pytest.raises(ValueError, match="more than 16"):
        ft_noise.program_gates(make_code("steane"), "X" * 8)


def test_no_faults_no_failures():
    for name, what, key in (("steane", "cycle", (7, False)), ("rm15", "cycle", (5, False)), ("steane", "program", tuple("X" * 8))):
        gadget = streamed(name, what, key)
        assert [int(v) for v in gadget.counts(5000, 0.0, 0.0, 0.0, seed=3)] == [5000] + [0] * 11
        assert not gadget.outcomes(300, 0.0, 0.0, 0.0, seed=3).any()


def test_shards_add_up_and_tiny_counts():
    name, what, key, p, count, seed, first = BEYOND_CASES["steane-12"]               # first_sample = 1 << 33
    gadget, ref = streamed(name, what, key), restated(name, what, key)
    words, want = reference("steane-12")
    parts = [gadget.error_rates(n, *p, seed=seed, first_sample=first + start) for start, n in ((0, 40001), (40001, 30000), (70001, count - 70001))]
    assert {f: sum(part[f] for part in parts) for f in want} == want
    assert [int(v) for v in gadget.counts(0, *p, seed=seed)] == [0] * 12
    for i in range(3):                                                               # count = 1, sample by sample
        assert gadget.error_rates(1, *p, seed=seed, first_sample=first + i) == ref.tally(words[i:i + 1])
    assert np.array_equal(gadget.outcomes(1, *p, seed=seed, first_sample=first + 2), words[2:3])
    assert gadget.outcomes(0, *p).shape == (0, gadget.ldw)


def test_code_level_entry_points():
    code = make_code("steane")
    name, what, key, p, count, seed, first = BEYOND_CASES["steane-7"]
    assert code.error_correct_streamed_error_rates(count, *p, rounds=7, seed=seed, first_sample=first) == reference("steane-7")[1]
    name, what, key, p, count, seed, first = BEYOND_CASES["X*8"]
    assert code.logical_program_streamed_error_rates("X" * 8, count, *p, seed=seed, first_sample=first) == reference("X*8")[1]
    idle = code.error_correct_streamed_error_rates(20000, 0.002, 0.001, 0.002, rounds=1, seed=9, idle_data=True)
    assert idle == code.error_correct_logical_error_rates(20000, 0.002, 0.001, 0.002, rounds=1, seed=9, idle_data=True) and 0 < idle['accepted'] < 20000
    # the device tally is the host rule applied to the device's own words
    gadget = streamed("steane", "cycle", (7, False))
    assert gadget.tally_host(gadget.outcomes(20000, 0.0008, 0.0004, 0.0008, seed=1)) == gadget.error_rates(20000, 0.0008, 0.0004, 0.0008, seed=1)


LONG = ("steane", "cycle", (1000, False), (3e-6, 5e-7, 5e-7), 4096, 11, 0)


@functools.lru_cache(maxsize=None)
def long_reference():
    """The long run under the host statements alone: the oracle's sampler, gf2_stream_words_host, gf2_stream_tally_host (each checked
    against the restatement in tests/test_stream.py)."""
    name, what, key, p, count, seed, first = LONG
    gadget = streamed(name, what, key)
    words = gadget.words_of_faults(*stream_ref.sampled_faults(gadget.num_locations, seed, first, count, p))
    return words, gadget.tally_host(words), gadget.tally_host(words, fields=True)


def test_long_run_equals_the_host_statements():
    name, what, key, p, count, seed, first = LONG
    gadget = streamed(name, what, key)
    assert (gadget.num_locations, (gadget.num_locations + 511) // 512, gadget.nsteps) == (330000, 645, 1001)
    words, want, fields = long_reference()
    print("\nlong run: %s" % want)
    assert count - want['accepted'] >= 100 and want['accepted'] >= 1000 and want['logical_any'] >= 10, "equality must not be vacuous"
    assert gadget.error_rates(count, *p, seed=seed, first_sample=first) == want
    assert [int(v) for v in gadget.counts(count, *p, seed=seed, first_sample=first)] == [int(v) for v in fields]
    assert np.array_equal(gadget.outcomes(64, *p, seed=seed, first_sample=first), words[:64])


def test_argument_errors():
    ctx = _native.default_context()
    gadget = streamed("steane", "cycle", (2, False))
    r1, keys1, flips1, r2, keys2, flips2 = gadget._tables()
    run = lambda a=r1, b=r2, k1=keys1, first=0, count=10, p=0.01: ctx.mc_stream_decode(gadget.device(), a, k1, flips1, b, keys2, flips2, 0, first, count, p, 0.0, 0.0)
    assert int(run()[0]) <= 10
    for kwargs, text in ((dict(a=32), "r_1, r_2 <= 31"), (dict(b=0), "r_1, r_2 <= 31"), (dict(a=2), "bits beyond the layout"), (dict(first=-1), "negative range"),
                         (dict(count=-1), "negative range"), (dict(p=1.5), "probabilities"),
                         (dict(k1=np.array([1, 1], dtype=np.uint64)), "occurs twice")):
        with pytest.raises(_native.GF2Error, match=text):
            run(**kwargs)
    buf = ctx.alloc(10 * gadget.ldw * 8)
    with pytest.raises(_native.GF2Error, match="ldo must be at least the sequence's nsteps . F = 4 words"):
        ctx.stream_outcomes_dev(gadget.device(), 0, 0, 10, 0.01, 0.0, 0.0, buf, 3)
    buf.free()
    eff, locs, flags, types, kinds = gadget._sequence()
    for kwargs, text in ((dict(flags=[65]), "at most 64"), (dict(types=[0, -1, 0], kinds=[1, 3, 1]), "must be the last step"),
                         (dict(types=[0, 0], kinds=[1, 1]), "no FINAL step and 0 MEASURE steps")):
        with pytest.raises(_native.GF2Error, match=text):
            ctx.stream_create(kwargs.get("eff", eff), locs, kwargs.get("flags", flags), kwargs.get("types", types), kwargs.get("kinds", kinds))
    tiny = np.zeros((60, 2, 3), dtype=np.uint64)                                     # nine blocks of 60 locations in one segment
    with pytest.raises(_native.GF2Error, match="overlap 9 blocks, more than 8"):
        ctx.stream_create(tiny, [60], [0], [0] * 9 + [-1], [1] * 9 + [3])
    ctx.stream_create(tiny, [60], [0], [0] * 7 + [-1], [1] * 7 + [3]).free()         # seven and the FINAL step: eight
