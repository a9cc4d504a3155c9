"""
The repeat-until-success sampler on the device (csrc/gf2_retry.hip, DESIGN.md section 5d "Repeat-until-success"): the stored words
and the fourteen counts bit for bit against the host statement (itself checked against tests/retry_ref.py in tests/test_retry.py) on
every path of the kernel, the exact distributions of tests/test_retry.py at 2^26 samples, and the rates against the post-selected
streamed route's.  Statistical verdicts are oracle/exact_dist.py's, thresholds as they are.
"""
import functools

import numpy as np
import pytest

from oracle import exact_dist
from quantum_css_codes_amd import _native, stream_noise
from tests import retry_ref
from tests.state_check import DirtyBuffer, Layout
from tests.test_gpu_stream import RESIDENT_CASES, make_code, streamed
from tests.test_retry import ONE_ROUND_P, rates

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


#        code, what, key, p_kind, max_attempts, seed, first_sample
CASES = {
    "steane-2": ("steane", "cycle", (2, False), 3e-3, 256, 1, 0),                    # 16 KB of tables: staged
    "rm15-3": ("rm15", "cycle", (3, False), 1e-3, 256, 2, 5),                        # staged; segments of 369 and 330 locations
    "rm15-XYZ": ("rm15", "program", ("X", "Y", "Z"), 1e-3, 256, 3, 0),               # six types, 190 KB: read through L2
    "program": ("steane", "program", (), 2e-3, 256, 4, 0),                           # a NONE block, MEASURE steps
    "program-XY": ("steane", "program", ("X", "Y"), 2e-3, 256, 5, 3),                # regions of 3 and 5 idle locations in front
    "idle": ("steane", "cycle", (2, True), 3e-3, 256, 6, 0),
    "one attempt": ("steane", "cycle", (2, False), 3e-3, 1, 7, 0),                   # exhausted lanes inside accepted wavefronts
    "two attempts": ("steane", "cycle", (2, False), 3e-3, 2, 8, 0),
    "no noise": ("steane", "cycle", (3, False), 0.0, 256, 9, 0),
    "first 2^33": ("steane", "cycle", (2, False), 3e-3, 256, 10, 1 << 33),
}
COUNT = 4096


@pytest.mark.parametrize("case", sorted(CASES))
def test_words_and_counts_equal_the_host_statement(case):
    name, what, key, p_kind, max_attempts, seed, first = CASES[case]
    gadget, p = streamed(name, what, key), rates(p_kind)
    want, _ = gadget.retry_words_host(COUNT, *p, seed=seed, first_sample=first, max_attempts=max_attempts)
    words = gadget.retry_outcomes(COUNT, *p, seed=seed, first_sample=first, max_attempts=max_attempts)
    assert np.array_equal(words, want)
    counts = host_counts(gadget, want)
    assert [int(v) for v in gadget.retry_counts(COUNT, *p, seed=seed, first_sample=first, max_attempts=max_attempts)] == counts
    if case == "rm15-XYZ":
        assert gadget.type_eff.nbytes > 160 * 1024
    if case in ("one attempt", "two attempts"):
        # both kinds of lanes in the wavefronts: (0.392 x 0.442)^2 = 3.0 % are accepted with one attempt, 1 - 0.80 = 20 % with two
        assert COUNT // 100 < counts[12] < COUNT - COUNT // 100
    elif case == "no noise":
        assert counts == [COUNT] + [0] * 12 + [COUNT * gadget.preparations] and not words[:, :-1].any()
    else:
        assert counts[12] == 0 and counts[13] * 20 > COUNT * gadget.preparations * 21 and sum(counts[1:12]) > 0
    rates_dict = gadget.retry_error_rates(COUNT, *p, seed=seed, first_sample=first, max_attempts=max_attempts)
    assert rates_dict['accepted'] == counts[0] and rates_dict['exhausted'] == counts[12] and rates_dict['attempts'] == counts[13]
    assert rates_dict['samples'] == COUNT and rates_dict['preparations'] == gadget.preparations


def test_tiny_counts_pitch_and_code_level_entry_points():
    ctx = _native.default_context()
    gadget, p = streamed("steane", "cycle", (2, False)), rates(3e-3)
    want, _ = gadget.retry_words_host(300, *p, seed=12)
    assert [int(v) for v in gadget.retry_counts(0, *p, seed=12)] == [0] * 14
    assert gadget.retry_outcomes(0, *p).shape == (0, gadget.ldw + 1)
    for i in range(3):                                                               # count = 1, sample by sample
        assert np.array_equal(gadget.retry_outcomes(1, *p, seed=12, first_sample=i), want[i:i + 1])
        assert [int(v) for v in gadget.retry_counts(1, *p, seed=12, first_sample=i)] == host_counts(gadget, want[i:i + 1])
    buf = DirtyBuffer(ctx, Layout(300, gadget.ldw + 4, 264))                         # a wider pitch at an address that is 8 mod 16
    ctx.retry_outcomes_dev(gadget.retry_device(), 12, 0, 300, *p, 256, buf.view, gadget.ldw + 4)
    buf.check(want, preserved=True, what="gf2_retry_outcomes_dev")                   # the padding is left as it was
    buf.free()
    code = make_code("steane")
    got = code.error_correct_retried_error_rates(COUNT, *p, rounds=2, seed=1)
    assert got == gadget.retry_error_rates(COUNT, *p, seed=1) and got['accepted'] == COUNT
    program = streamed("steane", "program", ("X", "Y"))
    assert code.logical_program_retried_error_rates("XY", COUNT, *rates(2e-3), seed=5, first_sample=3) == program.retry_error_rates(COUNT, *rates(2e-3), seed=5, first_sample=3)
    assert set(program.retry_error_rates(16, *p)) == {'accepted', 'wrong', 'trial_wrong', 'first_trial_wrong', 'split_vote', 'unmatched_x', 'unmatched_z',
                                                      'samples', 'exhausted', 'attempts', 'preparations'}


def test_long_run_accepts_what_post_selection_rejects():
    gadget, p = streamed("steane", "cycle", (1000, False)), rates(1e-3)
    assert (gadget.nsteps, gadget.preparations) == (1001, 2000)
    want, _ = gadget.retry_words_host(COUNT, *p, seed=13)
    counts = host_counts(gadget, want)
    assert counts[0] == COUNT and counts[12] == 0 and counts[3] > 0
    assert [int(v) for v in gadget.retry_counts(COUNT, *p, seed=13)] == counts
    assert np.array_equal(gadget.retry_outcomes(64, *p, seed=13), want[:64])
    assert int(gadget.counts(COUNT, *p, seed=13)[0]) == 0                            # the post-selected route keeps (0.728 x 0.758)^1000 of them


def test_shards_add_up_and_no_state_between_calls():
    gadget, p = streamed("steane", "cycle", (3, False)), rates(2e-3)
    selected = gadget.counts(3000, *rates(4e-3), seed=3)
    whole = gadget.retry_counts(8 * 5000 + 7, *p, seed=14, first_sample=100)
    parts = [gadget.retry_counts(5000 + (7 if k == 7 else 0), *p, seed=14, first_sample=100 + 5000 * k) for k in range(8)]
    assert [int(v) for v in whole] == [int(sum(int(part[f]) for part in parts)) for f in range(14)]
    # unrelated calls in between -- other rates, another sequence, the streamed route (the context's cached tables), other limits
    streamed("rm15", "cycle", (3, False)).retry_counts(3000, *rates(1e-3), seed=1)
    gadget.retry_counts(3000, *rates(5e-3), seed=2, max_attempts=3)
    gadget.counts(3000, *rates(4e-3), seed=3)
    gadget.retry_outcomes(100, *rates(1e-2), seed=4)
    assert np.array_equal(gadget.retry_counts(8 * 5000 + 7, *p, seed=14, first_sample=100), whole)
    assert np.array_equal(gadget.counts(3000, *rates(4e-3), seed=3), selected)      # ... whose cached tables no retry call has touched


# -- exact distributions at 2^26 samples -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,p_kind", [("steane", 1e-3), ("steane", 3e-3), ("rm15", 1e-3)])
def test_attempts_follow_the_geometric_law(name, p_kind):
    gadget, p = streamed(name, "cycle", (1, False)), rates(p_kind)
    counts = gadget.retry_counts(BIG, *p, seed=31)
    assert int(counts[12]) == 0 and int(counts[0]) == BIG                            # (truncation at 256 attempts: below 1e-50)
    mean, var = retry_ref.attempts_mean_var(gadget, p)
    exact_dist.assert_z("attempts of %s at p = %g, sum of 1/q = %.4f" % (name, p_kind, mean), int(counts[13]), BIG * mean, BIG * var)


def histogram(gadget, p, seed, cells, bins, chunk=1 << 22):
    out = np.zeros(bins, dtype=np.int64)
    for start in range(0, BIG, chunk):
        words = gadget.retry_outcomes(chunk, *p, seed=seed, first_sample=start)
        assert not words[:, gadget.nsteps:gadget.ldw].any()
        out += np.bincount(cells(words, 3, 3), minlength=bins)
    return out


def test_prepared_frame_follows_the_conditional_distribution():
    gadget, p = prepare_final(), rates(3e-3)
    exact = retry_ref.prepare_final_distribution(gadget, p, 3, 3)
    exact_dist.assert_chi2("T of [prepare, FINAL] given flags = 0, device", histogram(gadget, p, 32, retry_ref.prepare_final_cells, 256), exact, BIG)


def test_one_round_follows_the_convolution_of_the_regions():
    gadget, p = streamed("steane", "cycle", (1, False)), rates(ONE_ROUND_P)
    exact = retry_ref.one_round_distribution(gadget, p, 3, 3)
    exact_dist.assert_chi2("(round word, T) of one Steane round, device", histogram(gadget, p, 33, retry_ref.one_round_cells, 1 << 14), exact, BIG)


def test_rates_equal_the_post_selected_route():
    name, what, key, p, _, _, _ = RESIDENT_CASES["steane-5"]
    gadget = streamed(name, what, key)
    retried = gadget.retry_error_rates(BIG, *p, seed=41)
    selected = gadget.error_rates(1 << 28, *p, seed=42)
    assert retried['exhausted'] == 0 and retried['accepted'] == BIG and 0 < selected['accepted'] < 1 << 28
    n_1, n_2 = float(retried['accepted']), float(selected['accepted'])
    for field in ('logical_x', 'logical_z', 'logical_any', 'round_unmatched_x', 'round_unmatched_z'):
        a, b = retried[field], selected[field]
        pooled = (a + b) / (n_1 + n_2)
        var = pooled * (1.0 - pooled) * (1.0 / n_1 + 1.0 / n_2)                      # of the difference of the two rates under the pooled rate
        exact_dist.assert_z("%s per accepted sample, retried - post-selected" % field, a / n_1 - b / n_2, 0.0, var)


def test_argument_errors():
    ctx = _native.default_context()
    gadget = streamed("steane", "cycle", (2, False))
    r1, keys1, flips1, r2, keys2, flips2 = gadget._tables()
    run = lambda a=r1, first=0, count=10, p=0.01, limit=256: ctx.mc_retry_decode(gadget.retry_device(), a, keys1, flips1, r2, keys2, flips2, 0, first, count,
                                                                                 p, 0.0, 0.0, limit)
    assert int(run()[0]) + int(run()[12]) == 10
    for kwargs, text in ((dict(a=32), "r_1, r_2 <= 31"), (dict(a=2), "bits beyond the layout"), (dict(first=-1), "gf2_mc_retry_decode: negative range"),
                         (dict(count=-1), "negative range"), (dict(p=1.5), "probabilities"), (dict(limit=0), "gf2_mc_retry_decode: needs 1 <= max_attempts <= 65536, got 0"),
                         (dict(limit=65537), "needs 1 <= max_attempts <= 65536, got 65537")):
        with pytest.raises(_native.GF2Error, match=text):
            run(**kwargs)
    buf = ctx.alloc(10 * (gadget.ldw + 1) * 8)
    with pytest.raises(_native.GF2Error, match=r"gf2_retry_outcomes_dev: ldo must be at least the sequence's nsteps \+ F \+ 1 = 5 words"):
        ctx.retry_outcomes_dev(gadget.retry_device(), 0, 0, 10, 0.01, 0.0, 0.0, 256, buf, 4)
    with pytest.raises(_native.GF2Error, match="gf2_retry_outcomes_dev: needs 1 <= max_attempts"):
        ctx.retry_outcomes_dev(gadget.retry_device(), 0, 0, 10, 0.01, 0.0, 0.0, 0, buf, 5)
    buf.free()
    sequence = gadget._sequence()
    for regions, text in (([(0, 148, 1), (148, 21, 0), (169, 133, 0), (302, 28, 0)], "gf2_retry_create: region 2 of block type 0 .* is not retried but its locations set a flag bit"),
                          ([(0, 148, 1), (148, 20, 0), (169, 133, 1), (302, 28, 0)], "gf2_retry_create: the regions of block type 0 do not partition its 330 locations in order"),
                          ([(0, 100, 1), (100, 69, 1), (169, 133, 1), (302, 28, 0)], "gf2_retry_create: the flag masks of regions 0 and 1 of block type 0 intersect")):
        with pytest.raises(_native.GF2Error, match=text):
            ctx.retry_create(*sequence, np.array(regions), [4])
    sizes = np.arange(1, _native.RETRY_MAX_SIZES + 2)
    regions = np.stack([np.cumsum(sizes) - sizes, sizes, np.zeros_like(sizes)], axis=1)
    with pytest.raises(_native.GF2Error, match="gf2_retry_create: the regions have more than GF2_RETRY_MAX_SIZES = 16 distinct segment sizes"):
        ctx.retry_create(np.zeros((int(sizes.sum()), 2, 3), dtype=np.uint64), [int(sizes.sum())], [0], [0, -1], [1, 3], regions, [len(sizes)])
    eff, locs, flags, types, kinds = sequence
    with pytest.raises(_native.GF2Error, match="gf2_retry_create: the FINAL step must be the last step"):
        ctx.retry_create(eff, locs, flags, [0, -1, 0], [1, 3, 1], gadget.type_regions, gadget.type_nregions)
