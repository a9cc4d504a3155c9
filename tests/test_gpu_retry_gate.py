"""
The repeat-until-success sampler under gate-level faults on the device (csrc/gf2_retry_gate.hip, DESIGN.md section 5d
"Repeat-until-success under gate-level faults"): the stored words and the fourteen counts bit for bit against the host statement
(itself checked against tests/retry_gate_ref.py in tests/test_retry_gate.py) on every path of the kernel, the exact distributions of
tests/test_retry_gate.py at 2^26 samples, and the rates against the post-selected gate sampler's (csrc/gf2_gate_mc.hip).
Statistical verdicts are oracle/exact_dist.py's, thresholds as they are.
"""
import functools

import numpy as np
import pytest

from oracle import exact_dist
from quantum_css_codes_amd import _native, ec_noise, ft_noise, stream_noise
from tests import retry_gate_ref, retry_ref
from tests.state_check import DirtyBuffer, Layout
from tests.test_gpu_stream import make_code, streamed
from tests.test_retry_gate import ONE_ROUND_P

pytestmark = pytest.mark.gpu

BIG = 1 << 26


@functools.lru_cache(maxsize=None)
def prepare_final():
    code = make_code("steane")
    block = stream_noise.BlockType(code, "prepare data", stream_noise.NONE, stream_noise._emit_prepare)
    return stream_noise.StreamedGadget(code, "cycle", [block], [0, -1], [stream_noise.NONE, stream_noise.FINAL])


def host_counts(gadget, words):
    """The fourteen counts the host statement gives: gf2_stream_tally_host on the first nsteps + F words, the exhausted, the attempts."""
    fields = [int(v) for v in gadget.tally_host(words[:, :gadget.ldw], fields=True)]
    return fields + [len(words) - fields[0], int(words[:, -1].sum(dtype=np.uint64))]


#        code, what, key, p1, p2, max_attempts, seed, first_sample
CASES = {
    "steane-2": ("steane", "cycle", (2, False), 3e-3, 3e-3, 256, 1, 0),                  # 16 KB of tables: staged
    "rm15-3": ("rm15", "cycle", (3, False), 1e-3, 1e-3, 256, 2, 5),                      # staged
    "rm15-XYZ": ("rm15", "program", ("X", "Y", "Z"), 1e-3, 1e-3, 256, 3, 0),             # six types, 190 KB: read through L2
    "program": ("steane", "program", (), 2e-3, 2e-3, 256, 4, 0),                         # a NONE block, MEASURE steps
    "program-XY": ("steane", "program", ("X", "Y"), 2e-3, 2e-3, 256, 5, 3),              # regions of 3 and 5 idle gates in front
    "idle": ("steane", "cycle", (2, True), 3e-3, 3e-3, 256, 6, 0),
    "one attempt": ("steane", "cycle", (2, False), 3e-3, 3e-3, 1, 7, 0),                 # exhausted lanes inside accepted wavefronts
    "two attempts": ("steane", "cycle", (2, False), 6e-3, 6e-3, 2, 8, 0),
    "no noise": ("steane", "cycle", (3, False), 0.0, 0.0, 256, 9, 0),
    "no one-operand faults": ("steane", "cycle", (2, False), 0.0, 6e-3, 256, 11, 0),
    "no CNOT faults": ("steane", "cycle", (2, False), 6e-3, 0.0, 256, 12, 0),
    "first 2^33": ("steane", "cycle", (2, False), 3e-3, 3e-3, 256, 10, 1 << 33),
}
COUNT = 4096


@pytest.mark.parametrize("case", sorted(CASES))
def test_words_and_counts_equal_the_host_statement(case):
    name, what, key, p1, p2, max_attempts, seed, first = CASES[case]
    gadget = streamed(name, what, key)
    want, _ = gadget.retry_gate_words_host(COUNT, p1, p2, seed=seed, first_sample=first, max_attempts=max_attempts)
    words = gadget.retry_gate_outcomes(COUNT, p1, p2, seed=seed, first_sample=first, max_attempts=max_attempts)
    assert np.array_equal(words, want)
    counts = host_counts(gadget, want)
    assert [int(v) for v in gadget.retry_gate_counts(COUNT, p1, p2, seed=seed, first_sample=first, max_attempts=max_attempts)] == counts
    if case == "rm15-XYZ":
        assert gadget.type_eff.nbytes + gadget.type_site_loc.nbytes > 160 * 1024
    if case in ("one attempt", "two attempts"):
        # both kinds of lanes in the wavefronts: (0.806 x 0.827)^2 = 44 % are accepted with one attempt at 3e-3, and
        # ((1 - 0.349^2)(1 - 0.315^2))^2 = 63 % with two at 6e-3
        assert COUNT // 100 < counts[12] < COUNT - COUNT // 100 and COUNT // 100 < counts[0]
    elif case == "no noise":
        assert counts == [COUNT] + [0] * 12 + [COUNT * gadget.preparations] and not words[:, :-1].any()
    else:
        assert counts[12] == 0 and counts[13] * 20 > COUNT * gadget.preparations * 21 and sum(counts[1:12]) > 0
    rates_dict = gadget.retry_gate_error_rates(COUNT, p1, p2, seed=seed, first_sample=first, max_attempts=max_attempts)
    assert rates_dict['accepted'] == counts[0] and rates_dict['exhausted'] == counts[12] and rates_dict['attempts'] == counts[13]
    assert rates_dict['samples'] == COUNT and rates_dict['preparations'] == gadget.preparations


def test_tiny_counts_pitch_and_code_level_entry_points():
    ctx = _native.default_context()
    gadget, p = streamed("steane", "cycle", (2, False)), 3e-3
    want, _ = gadget.retry_gate_words_host(300, p, p, seed=12)
    assert [int(v) for v in gadget.retry_gate_counts(0, p, p, seed=12)] == [0] * 14
    assert gadget.retry_gate_outcomes(0, p, p).shape == (0, gadget.ldw + 1)
    for i in range(3):                                                               # count = 1, sample by sample
        assert np.array_equal(gadget.retry_gate_outcomes(1, p, p, seed=12, first_sample=i), want[i:i + 1])
        assert [int(v) for v in gadget.retry_gate_counts(1, p, p, seed=12, first_sample=i)] == host_counts(gadget, want[i:i + 1])
    buf = DirtyBuffer(ctx, Layout(300, gadget.ldw + 4, 264))                         # a wider pitch at an address that is 8 mod 16
    ctx.retry_gate_outcomes_dev(gadget.retry_gate_device(), 12, 0, 300, p, p, 256, buf.view, gadget.ldw + 4)
    buf.check(want, preserved=True, what="gf2_retry_gate_outcomes_dev")              # the padding is left as it was
    buf.free()
    code = make_code("steane")
    got = code.error_correct_retried_gate_error_rates(COUNT, p, p, rounds=2, seed=1)
    assert got == gadget.retry_gate_error_rates(COUNT, p, p, seed=1) and got['accepted'] == COUNT
    program = streamed("steane", "program", ("X", "Y"))
    assert code.logical_program_retried_gate_error_rates("XY", COUNT, 2e-3, 2e-3, seed=5, first_sample=3) == \
        program.retry_gate_error_rates(COUNT, 2e-3, 2e-3, seed=5, first_sample=3)
    assert set(program.retry_gate_error_rates(16, p, p)) == {'accepted', 'wrong', 'trial_wrong', 'first_trial_wrong', 'split_vote', 'unmatched_x',
                                                             'unmatched_z', 'samples', 'exhausted', 'attempts', 'preparations'}


def test_long_run_accepts_every_sample():
    gadget, p = streamed("steane", "cycle", (1000, False)), 1e-3
    assert (gadget.nsteps, gadget.preparations) == (1001, 2000)
    want, _ = gadget.retry_gate_words_host(COUNT, p, p, seed=13)
    counts = host_counts(gadget, want)
    assert counts[0] == COUNT and counts[12] == 0 and counts[3] > 0
    assert [int(v) for v in gadget.retry_gate_counts(COUNT, p, p, seed=13)] == counts
    assert np.array_equal(gadget.retry_gate_outcomes(64, p, p, seed=13), want[:64])


def test_shards_add_up_and_no_state_between_calls():
    gadget, p = streamed("steane", "cycle", (3, False)), 2e-3
    cycle = ec_noise.circuit_for(make_code("steane"), 3)
    whole = gadget.retry_gate_counts(8 * 5000 + 7, p, p, seed=14, first_sample=100)
    parts = [gadget.retry_gate_counts(5000 + (7 if k == 7 else 0), p, p, seed=14, first_sample=100 + 5000 * k) for k in range(8)]
    assert [int(v) for v in whole] == [int(sum(int(part[f]) for part in parts)) for f in range(14)]
    # unrelated calls in between: the location version, the resident cycle, the gate sampler with other rates, other limits
    gadget.retry_counts(3000, 5e-3, 5e-3, 5e-3, seed=2, max_attempts=3)
    cycle.logical_error_rates(3000, 4e-3, 4e-3, 4e-3, seed=3)
    cycle.gate_error_rates(3000, 7e-3, 9e-3, seed=4)
    streamed("rm15", "cycle", (3, False)).retry_gate_counts(3000, 1e-3, 2e-3, seed=1)
    gadget.retry_gate_counts(3000, 5e-3, 1e-3, seed=2, max_attempts=3)
    gadget.retry_gate_outcomes(100, 1e-2, 1e-2, seed=4)
    assert np.array_equal(gadget.retry_gate_counts(8 * 5000 + 7, p, p, seed=14, first_sample=100), whole)


def test_the_two_retried_samplers_are_other_streams():
    # a smoke check of the slot separation, not a statistical claim: with one class switched off the gate route still draws other
    # words than the location route of the same seed
    gadget = streamed("steane", "cycle", (2, False))
    location = gadget.retry_outcomes(COUNT, 1e-3, 1e-3, 1e-3, seed=4)
    for p1, p2 in ((3e-3, 0.0), (0.0, 3e-3)):
        gate = gadget.retry_gate_outcomes(COUNT, p1, p2, seed=4)
        assert (gate[:, :gadget.nsteps] != location[:, :gadget.nsteps]).any(axis=1).sum() > COUNT // 10


# -- exact distributions at 2^26 samples -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [1e-3, 3e-3])
def test_attempts_follow_the_geometric_law(p):
    gadget = streamed("steane", "cycle", (1, False))
    counts = gadget.retry_gate_counts(BIG, p, p, seed=31)
    assert int(counts[12]) == 0 and int(counts[0]) == BIG                            # (truncation at 256 attempts: below 1e-100)
    mean, var = retry_gate_ref.attempts_mean_var(gadget, p, p)
    exact_dist.assert_z("gate faults: attempts of steane at p = %g, sum of 1/q = %.4f" % (p, mean), int(counts[13]), BIG * mean, BIG * var)


def histogram(gadget, p, seed, cells, bins, chunk=1 << 22):
    out = np.zeros(bins, dtype=np.int64)
    for start in range(0, BIG, chunk):
        words = gadget.retry_gate_outcomes(chunk, p, p, seed=seed, first_sample=start)
        assert not words[:, gadget.nsteps:gadget.ldw].any()
        out += np.bincount(cells(words, 3, 3), minlength=bins)
    return out


def test_prepared_frame_follows_the_conditional_distribution():
    gadget, p = prepare_final(), 3e-3
    exact = retry_gate_ref.prepare_final_distribution(gadget, p, p, 3, 3)
    exact_dist.assert_chi2("gate faults: T of [prepare, FINAL] given flags = 0, device", histogram(gadget, p, 32, retry_ref.prepare_final_cells, 256),
                           exact, BIG)


def test_one_round_follows_the_convolution_of_the_regions():
    gadget, p = streamed("steane", "cycle", (1, False)), ONE_ROUND_P
    exact = retry_gate_ref.one_round_distribution(gadget, p, p, 3, 3)
    assert retry_gate_ref.sparse_share(exact, BIG) <= exact_dist.MAX_REST_MASS
    exact_dist.assert_chi2("gate faults: (round word, T) of one Steane round, device", histogram(gadget, p, 33, retry_ref.one_round_cells, 1 << 14),
                           exact, BIG)


# -- against the post-selected gate sampler ------------------------------------------------------------------------------------------

def assert_rates_agree(what, retried, selected, fields):
    n_1, n_2 = float(retried['accepted']), float(selected['accepted'])
    for field in fields:
        a, b = retried[field], selected[field]
        pooled = (a + b) / (n_1 + n_2)
        var = pooled * (1.0 - pooled) * (1.0 / n_1 + 1.0 / n_2)                      # of the difference of the two rates under the pooled rate
        print("RATES %s %s: retried %d / %d, post-selected %d / %d" % (what, field, a, int(n_1), b, int(n_2)))
        exact_dist.assert_z("%s: %s per accepted sample, retried - post-selected" % (what, field), a / n_1 - b / n_2, 0.0, var)


def test_rates_equal_the_post_selected_gate_sampler_steane_cycle():
    gadget, p = streamed("steane", "cycle", (1, False)), 1e-3
    retried = gadget.retry_gate_error_rates(BIG, p, p, seed=41)
    selected = ec_noise.circuit_for(make_code("steane"), 1).gate_error_rates(1 << 28, p, p, seed=42)
    assert retried['exhausted'] == 0 and retried['accepted'] == BIG and 0 < selected['accepted'] < 1 << 28
    assert_rates_agree("one Steane round at 1e-3", retried, selected, ('logical_x', 'logical_z', 'logical_any', 'round_unmatched_x', 'round_unmatched_z'))


def test_rates_equal_the_post_selected_gate_sampler_reed_muller_program():
    """2^24 retried samples against 2^30 post-selected ones (about 9 x 10^6 accepted) of the Reed-Muller program with no gate at
    p1 = p2 = 3e-3, the fields that are one event per sample."""
    gadget, p = streamed("rm15", "program", ()), 3e-3
    retried = gadget.retry_gate_error_rates(1 << 24, p, p, seed=43)
    selected = ft_noise.program_for(make_code("rm15"), ()).gate_error_rates(1 << 30, p, p, seed=44)
    assert retried['exhausted'] == 0 and retried['accepted'] == 1 << 24 and 5000000 < selected['accepted'] < 15000000
    assert_rates_agree("Reed-Muller program at 3e-3", retried, selected, ('wrong', 'first_trial_wrong', 'split_vote'))


def test_argument_errors():
    ctx = _native.default_context()
    gadget = streamed("steane", "cycle", (2, False))
    r1, keys1, flips1, r2, keys2, flips2 = gadget._tables()
    run = lambda a=r1, first=0, count=10, p1=0.01, p2=0.01, limit=256: ctx.mc_retry_gate_decode(gadget.retry_gate_device(), a, keys1, flips1, r2, keys2,
                                                                                                 flips2, 0, first, count, p1, p2, limit)
    assert int(run()[0]) + int(run()[12]) == 10
    for kwargs, text in ((dict(a=32), "r_1, r_2 <= 31"), (dict(a=2), "bits beyond the layout"),
                         (dict(first=-1), r"gf2_mc_retry_gate_decode: negative range \(needs count >= 0 and first_sample >= 0\)"),
                         (dict(count=-1), "negative range"), (dict(p1=1.5), "gf2_mc_retry_gate_decode: needs 0 <= p_1, p_2 <= 1"),
                         (dict(p2=float("nan")), "needs 0 <= p_1, p_2 <= 1"),
                         (dict(limit=0), "gf2_mc_retry_gate_decode: needs 1 <= max_attempts <= 65536, got 0"),
                         (dict(limit=65537), "needs 1 <= max_attempts <= 65536, got 65537")):
        with pytest.raises(_native.GF2Error, match=text):
            run(**kwargs)
    buf = ctx.alloc(10 * (gadget.ldw + 1) * 8)
    with pytest.raises(_native.GF2Error, match=r"gf2_retry_gate_outcomes_dev: ldo must be at least the sequence's nsteps \+ F \+ 1 = 5 words"):
        ctx.retry_gate_outcomes_dev(gadget.retry_gate_device(), 0, 0, 10, 0.01, 0.01, 256, buf, 4)
    with pytest.raises(_native.GF2Error, match="gf2_retry_gate_outcomes_dev: needs 1 <= max_attempts"):
        ctx.retry_gate_outcomes_dev(gadget.retry_gate_device(), 0, 0, 10, 0.01, 0.01, 0, buf, 5)
    buf.free()
    sequence = gadget._retry_sequence()
    loc, counts = gadget.type_site_loc, gadget.type_site_regions
    swapped = loc.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    outside = loc.copy()
    outside[0] = 148
    for site_loc, site_regions, text in ((np.resize(loc, 229), [[55, 47], [7, 7], [51, 41], [14, 7]], "gf2_retry_gate_create: region 0 of block type 0 has n_1 \\+ 2 n_2 = 55"),
                                         (outside, counts, "gf2_retry_gate_create: the sites of region 0 of block type 0 do not partition its locations"),
                                         (swapped, counts, "gf2_retry_gate_create: the one-operand sites of region 0 of block type 0 are not ascending")):
        with pytest.raises(_native.GF2Error, match=text):
            ctx.retry_gate_create(*sequence, site_loc, np.asarray(site_regions))
    with pytest.raises(_native.GF2Error, match="gf2_retry_gate_create: region 2 of block type 0 .* is not retried but its locations set a flag bit"):
        ctx.retry_gate_create(*gadget._sequence(), np.array([(0, 148, 1), (148, 21, 0), (169, 133, 0), (302, 28, 0)]), [4], loc, counts)
