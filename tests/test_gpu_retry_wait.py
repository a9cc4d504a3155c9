"""
The repeat-until-success sampler with waiting faults on the device (csrc/gf2_retry_wait.hip, DESIGN.md section 5d "Repeat-until-success
with waiting faults"): the stored words and the fifteen counts bit for bit against the host statement (itself checked against
tests/retry_wait_ref.py in tests/test_retry_wait.py) on every path of the kernel, consequences 1 and 2 against the plain retried
kernel, the exact distributions of tests/test_retry_wait.py at 2^26 samples, consequence 3 against the post-selected streamed route
on block types that hold the waiting IDLEs as ordinary locations, and a run of a thousand rounds.  Statistical verdicts are
oracle/exact_dist.py's, thresholds as they are.
"""
import numpy as np
import pytest

from oracle import exact_dist
from quantum_css_codes_amd import _native
from tests import retry_ref, retry_wait_ref
from tests.state_check import DirtyBuffer, Layout
from tests.test_gpu_stream import make_code, streamed
from tests.test_retry import rates
from tests.test_retry_wait import ONE_ROUND_P, ONE_ROUND_Q, WAIT_Z_P, WAIT_Z_Q, HandMade, waited_cycle

pytestmark = pytest.mark.gpu

BIG = 1 << 26
COUNT = 4096


def host_counts(gadget, words):
    """The fifteen counts the host statement gives: gf2_stream_tally_host on the first nsteps + F words, the exhausted, the attempts,
    the wait faults."""
    fields = [int(v) for v in gadget.tally_host(words[:, :gadget.ldw], fields=True)]
    return fields + [len(words) - fields[0], int(words[:, -2].sum(dtype=np.uint64)), int(words[:, -1].sum(dtype=np.uint64))]


#        code, what, key, p_kind, q_kind, wait_steps, max_attempts, seed, first_sample
CASES = {
    "steane-2": ("steane", "cycle", (2, False), 3e-3, 3e-3, 1, 256, 1, 0),                  # 16 KB of tables: staged
    "rm15-3": ("rm15", "cycle", (3, False), 1e-3, 2e-3, 1, 256, 2, 5),                      # staged; 15 wait rows per preparation
    "rm15-XYZ": ("rm15", "program", ("X", "Y", "Z"), 1e-3, 1e-3, 1, 256, 3, 0),             # six types, 190 KB: read through L2
    "program-XY": ("steane", "program", ("X", "Y"), 2e-3, 2e-3, 1, 256, 5, 3),              # a NONE block without wait rows, MEASURE steps
    "idle": ("steane", "cycle", (2, True), 3e-3, 3e-3, 1, 256, 6, 0),
    "two wait steps": ("steane", "cycle", (2, False), 3e-3, 3e-3, 2, 256, 7, 0),
    "one attempt": ("steane", "cycle", (2, False), 3e-3, 3e-3, 1, 1, 8, 0),                 # exhausted lanes inside accepted wavefronts
    "three attempts": ("steane", "cycle", (2, False), 3e-3, 3e-3, 1, 3, 9, 0),
    "no gate noise": ("steane", "cycle", (3, False), 0.0, 3e-3, 1, 256, 10, 0),             # p = 0 with q > 0: waiting faults alone
    "no wait noise": ("steane", "cycle", (2, False), 3e-3, 0.0, 1, 256, 11, 0),             # q = 0
    "first 2^33": ("steane", "cycle", (2, False), 3e-3, 3e-3, 1, 256, 12, 1 << 33),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_words_and_counts_equal_the_host_statement(case):
    name, what, key, p_kind, q_kind, steps, max_attempts, seed, first = CASES[case]
    gadget, p, q = streamed(name, what, key), rates(p_kind), rates(q_kind)
    more = dict(seed=seed, first_sample=first, wait_steps=steps, max_attempts=max_attempts)
    want, _ = gadget.retry_wait_words_host(COUNT, *p, *q, **more)
    words = gadget.retry_wait_outcomes(COUNT, *p, *q, **more)
    assert words.shape == (COUNT, gadget.ldw + 2) and np.array_equal(words, want)
    counts = host_counts(gadget, want)
    assert [int(v) for v in gadget.retry_wait_counts(COUNT, *p, *q, **more)] == counts
    if case == "rm15-XYZ":
        assert gadget.type_eff.nbytes > 160 * 1024
    if case in ("one attempt", "three attempts"):
        assert COUNT // 100 < counts[12] < COUNT - COUNT // 100                        # both kinds of lanes in the wavefronts
    elif case == "no gate noise":
        assert counts[0] == COUNT and counts[13] == COUNT * gadget.preparations and counts[14] > 0 and sum(counts[1:12]) > 0
    else:
        assert counts[12] == 0 and counts[13] * 20 > COUNT * gadget.preparations * 21 and sum(counts[1:12]) > 0
    assert (counts[14] == 0) == (case == "no wait noise")
    got = gadget.retry_wait_error_rates(COUNT, *p, *q, **more)
    assert got['accepted'] == counts[0] and got['exhausted'] == counts[12] and got['attempts'] == counts[13] and got['wait_faults'] == counts[14]
    assert got['samples'] == COUNT and got['preparations'] == gadget.preparations and got['wait_locations'] == gadget.wait_locations(steps)


@pytest.mark.parametrize("ntypes", [1, 11], ids=["512 rows", "11 x 512 rows"])
def test_sequences_made_by_hand(ntypes):
    """A region of 512 wait rows at q_kind = 0.01 (K = 15 per attempt: Floyd's rule); eleven of them are 180 KB of wait rows, which
    the kernel reads through L2."""
    ctx = _native.default_context()
    hand, p, q = HandMade(ntypes=ntypes, seed=ntypes), rates(1e-2), rates(1e-2)
    assert (hand.wait_eff.nbytes > 160 * 1024) == (ntypes == 11)
    tables = streamed("steane", "cycle", (1, False))._tables()
    device = ctx.retry_wait_create(*hand.arguments())
    want, _ = hand.words_host(COUNT, p, q, seed=21, first=3)
    words = ctx.outcomes(ctx.retry_wait_outcomes_dev, device, 21, 3, COUNT, *p, hand.ldw + 2, *q, 256)
    assert np.array_equal(words, want)
    fields = [int(v) for v in _native.stream_tally_host(want[:, :hand.ldw], hand.block_kind, 1, *tables)]
    counts = fields + [COUNT - fields[0], int(want[:, -2].sum(dtype=np.uint64)), int(want[:, -1].sum(dtype=np.uint64))]
    assert [int(v) for v in ctx.mc_retry_wait_decode(device, *tables, 21, 3, COUNT, *p, *q, 256)] == counts
    assert counts[14] > COUNT * ntypes * 512 * 0.03 and counts[13] > COUNT * ntypes * 1.25
    device.free()


def test_tiny_counts_pitch_and_code_level_entry_points():
    ctx = _native.default_context()
    gadget, p, q = streamed("steane", "cycle", (2, False)), rates(3e-3), rates(2e-3)
    want, _ = gadget.retry_wait_words_host(300, *p, *q, seed=12)
    assert [int(v) for v in gadget.retry_wait_counts(0, *p, *q, seed=12)] == [0] * 15
    assert gadget.retry_wait_outcomes(0, *p, *q).shape == (0, gadget.ldw + 2)
    for i in range(3):                                                               # count = 1, sample by sample
        assert np.array_equal(gadget.retry_wait_outcomes(1, *p, *q, seed=12, first_sample=i), want[i:i + 1])
        assert [int(v) for v in gadget.retry_wait_counts(1, *p, *q, seed=12, first_sample=i)] == host_counts(gadget, want[i:i + 1])
    buf = DirtyBuffer(ctx, Layout(300, gadget.ldw + 5, 264))                         # a wider pitch at an address that is 8 mod 16
    ctx.retry_wait_outcomes_dev(gadget.retry_wait_device(), 12, 0, 300, *p, *q, 256, buf.view, gadget.ldw + 5)
    buf.check(want, preserved=True, what="gf2_retry_wait_outcomes_dev")              # the padding is left as it was
    buf.free()
    code = make_code("steane")
    got = code.error_correct_retried_wait_error_rates(COUNT, *p, *q, rounds=2, seed=1)
    assert got == gadget.retry_wait_error_rates(COUNT, *p, *q, seed=1) and got['accepted'] == COUNT and got['wait_locations'] == 28
    assert code.error_correct_retried_wait_error_rates(COUNT, *p, *q, rounds=2, seed=1, idle_data=True, wait_steps=2) == \
        streamed("steane", "cycle", (2, True)).retry_wait_error_rates(COUNT, *p, *q, seed=1, wait_steps=2)
    program = streamed("steane", "program", ("X", "Y"))
    assert code.logical_program_retried_wait_error_rates("XY", COUNT, *p, *q, seed=5, first_sample=3) == program.retry_wait_error_rates(COUNT, *p, *q, seed=5, first_sample=3)
    assert set(program.retry_wait_error_rates(16, *p, *q)) == {'accepted', 'wrong', 'trial_wrong', 'first_trial_wrong', 'split_vote', 'unmatched_x', 'unmatched_z',
                                                               'samples', 'exhausted', 'attempts', 'preparations', 'wait_faults', 'wait_locations'}


# -- consequences 1 and 2 against the plain retried kernel -------------------------------------------------------------------------

@pytest.mark.parametrize("name,what,key,p_kind,limit", [("steane", "cycle", (2, False), 3e-3, 256), ("steane", "cycle", (2, False), 3e-3, 3),
                                                        ("rm15", "program", ("X", "Y", "Z"), 1e-3, 256)])
def test_consequences_1_and_2_against_the_plain_retried_kernel(name, what, key, p_kind, limit):
    gadget, p = streamed(name, what, key), rates(p_kind)
    plain = gadget.retry_outcomes(COUNT, *p, seed=15, first_sample=9, max_attempts=limit)
    plain_counts = [int(v) for v in gadget.retry_counts(COUNT, *p, seed=15, first_sample=9, max_attempts=limit)]
    for steps in (1, 2):                                                             # 1: q = 0 is the plain route, bit for bit
        words = gadget.retry_wait_outcomes(COUNT, *p, *rates(0.0), seed=15, first_sample=9, wait_steps=steps, max_attempts=limit)
        assert np.array_equal(words[:, :-1], plain) and not words[:, -1].any()
        counts = gadget.retry_wait_counts(COUNT, *p, *rates(0.0), seed=15, first_sample=9, wait_steps=steps, max_attempts=limit)
        assert [int(v) for v in counts] == plain_counts + [0]
    q = (2e-2, 0.0, 1e-2)                                                            # 2: any q leaves the attempts and the exhausted as they are
    words = gadget.retry_wait_outcomes(COUNT, *p, *q, seed=15, first_sample=9, max_attempts=limit)
    assert np.array_equal(words[:, gadget.nsteps:gadget.ldw + 1], plain[:, gadget.nsteps:])      # the flag words and the attempts
    assert (words[:, :gadget.nsteps] != plain[:, :gadget.nsteps]).any() and words[:, -1].any()
    counts = [int(v) for v in gadget.retry_wait_counts(COUNT, *p, *q, seed=15, first_sample=9, max_attempts=limit)]
    assert counts[0] == plain_counts[0] and counts[12:14] == plain_counts[12:14] and (counts[12] > 0) == (limit == 3)


def test_shards_add_up_and_no_state_between_calls():
    gadget, p, q = streamed("steane", "cycle", (3, False)), rates(2e-3), rates(1e-3)
    whole = gadget.retry_wait_counts(2 * 20000 + 7, *p, *q, seed=14, first_sample=100)
    parts = [gadget.retry_wait_counts(20000 + 7 * k, *p, *q, seed=14, first_sample=100 + 20000 * k) for k in range(2)]
    assert [int(v) for v in whole] == [int(parts[0][f]) + int(parts[1][f]) for f in range(15)]
    # unrelated calls in between -- other rates, other wait steps, another sequence, the plain retried route
    streamed("rm15", "cycle", (3, False)).retry_wait_counts(3000, *rates(1e-3), *rates(1e-3), seed=1)
    gadget.retry_wait_counts(3000, *rates(5e-3), *rates(1e-2), seed=2, wait_steps=3, max_attempts=3)
    gadget.retry_counts(3000, *rates(4e-3), seed=3)
    assert np.array_equal(gadget.retry_wait_counts(2 * 20000 + 7, *p, *q, seed=14, first_sample=100), whole)


# -- exact distributions at 2^26 samples -------------------------------------------------------------------------------------------

def test_wait_faults_follow_their_exact_mean_and_variance():
    gadget, p, q = streamed("steane", "cycle", (1, False)), rates(WAIT_Z_P), rates(WAIT_Z_Q)
    mean, var, once, _ = retry_wait_ref.wait_faults_mean_var(gadget, p, q)
    assert abs(mean - once) * BIG > 5.0 * (BIG * var) ** 0.5
    counts = gadget.retry_wait_counts(BIG, *p, *q, seed=34)
    assert int(counts[12]) == 0 and int(counts[0]) == BIG                            # (truncation at 256 attempts: below 1e-50)
    exact_dist.assert_z("wait faults of one Steane round at p = q = %g, device, mean %.4f per sample" % (WAIT_Z_P, mean), int(counts[14]),
                        BIG * mean, BIG * var)


def test_one_round_follows_the_convolution_with_the_wait_noise():
    gadget, p, q = streamed("steane", "cycle", (1, False)), rates(ONE_ROUND_P), rates(ONE_ROUND_Q)
    exact = retry_wait_ref.one_round_distribution(gadget, p, q, 3, 3)
    got = np.zeros(1 << 14, dtype=np.int64)
    for start in range(0, BIG, 1 << 22):
        words = gadget.retry_wait_outcomes(1 << 22, *p, *q, seed=35, first_sample=start)
        assert not words[:, gadget.nsteps:gadget.ldw].any()
        got += np.bincount(retry_ref.one_round_cells(words, 3, 3), minlength=1 << 14)
    exact_dist.assert_chi2("(round word, T) of one Steane round with waiting faults, device", got, exact, BIG)


def test_consequence_3_one_attempt_is_post_selection_of_the_waited_block_types():
    """max_attempts = 1 and q = p: the accepted samples have the distribution of the post-selected streamed route run on the block
    type with the waiting IDLEs as ordinary locations (one-round Steane at p_kind = 1e-3: post-selection keeps 55 %)."""
    gadget, waited, p = streamed("steane", "cycle", (1, False)), waited_cycle(make_code("steane")), rates(1e-3)
    assert waited.num_locations == gadget.num_locations + gadget.wait_locations()
    retried = gadget.retry_wait_error_rates(BIG, *p, *p, seed=41, max_attempts=1)
    selected = waited.error_rates(BIG, *p, seed=42)
    n_1, n_2 = float(retried['accepted']), float(selected['accepted'])
    assert retried['accepted'] + retried['exhausted'] == BIG and BIG // 2 < retried['accepted'] < BIG and BIG // 2 < selected['accepted'] < BIG
    pooled = (n_1 + n_2) / (2.0 * BIG)
    exact_dist.assert_z("accepted fraction, one attempt - post-selected", n_1 / BIG - n_2 / BIG, 0.0, pooled * (1.0 - pooled) * 2.0 / BIG)
    for field in ('logical_x', 'logical_z', 'logical_any', 'round_unmatched_x', 'round_unmatched_z'):
        a, b = retried[field], selected[field]
        pooled = (a + b) / (n_1 + n_2)
        var = pooled * (1.0 - pooled) * (1.0 / n_1 + 1.0 / n_2)                      # of the difference of the two rates under the pooled rate
        exact_dist.assert_z("%s per accepted sample, one attempt with waiting faults - post-selected" % field, a / n_1 - b / n_2, 0.0, var)


def test_a_thousand_rounds():
    gadget, p, q = streamed("steane", "cycle", (1000, False)), rates(1e-3), rates(1e-3)
    assert (gadget.nsteps, gadget.preparations, gadget.wait_locations()) == (1001, 2000, 14000)
    want, _ = gadget.retry_wait_words_host(COUNT, *p, *q, seed=13)
    counts = host_counts(gadget, want)
    assert counts[0] == COUNT and counts[12] == 0 and counts[3] > 0                  # every sample accepted
    assert [int(v) for v in gadget.retry_wait_counts(COUNT, *p, *q, seed=13)] == counts
    assert np.array_equal(gadget.retry_wait_outcomes(64, *p, *q, seed=13), want[:64])
    mean, var, _, attempts = retry_wait_ref.wait_faults_mean_var(gadget, p, q)
    scale = COUNT * gadget.wait_locations() * retry_wait_ref.quantised_total(q)      # wait faults per unit of attempts per preparation
    print("\nattempts per preparation: %.5f from the wait faults, %.5f exact" % (counts[14] / scale, attempts))
    assert abs(COUNT * mean / scale - attempts) < 1e-9
    exact_dist.assert_z("wait faults / (samples x wait locations x q_t) against the attempts per preparation, 1000 rounds", counts[14] / scale,
                        attempts, COUNT * var / scale ** 2)


def test_argument_errors():
    ctx = _native.default_context()
    gadget = streamed("steane", "cycle", (2, False))
    r1, keys1, flips1, r2, keys2, flips2 = gadget._tables()
    device = gadget.retry_wait_device()
    run = lambda a=r1, first=0, count=10, p=0.01, q=0.01, limit=256: ctx.mc_retry_wait_decode(device, a, keys1, flips1, r2, keys2, flips2, 0, first, count,
                                                                                               p, 0.0, 0.0, q, 0.0, 0.0, limit)
    assert int(run()[0]) + int(run()[12]) == 10
    for kwargs, text in ((dict(a=32), "r_1, r_2 <= 31"), (dict(a=2), "bits beyond the layout"), (dict(first=-1), "gf2_mc_retry_wait_decode: negative range"),
                         (dict(p=1.5), "probabilities"), (dict(q=1.5), "gf2_mc_retry_wait_decode: the waiting probabilities must be non-negative and sum to at most 1"),
                         (dict(q=-0.1), "the waiting probabilities"), (dict(limit=0), "gf2_mc_retry_wait_decode: needs 1 <= max_attempts <= 65536, got 0")):
        with pytest.raises(_native.GF2Error, match=text):
            run(**kwargs)
    buf = ctx.alloc(10 * (gadget.ldw + 2) * 8)
    with pytest.raises(_native.GF2Error, match=r"gf2_retry_wait_outcomes_dev: ldo must be at least the sequence's nsteps \+ F \+ 2 = 6 words"):
        ctx.retry_wait_outcomes_dev(device, 0, 0, 10, 0.01, 0.0, 0.0, 0.01, 0.0, 0.0, 256, buf, 5)
    with pytest.raises(_native.GF2Error, match="gf2_retry_wait_outcomes_dev: the waiting probabilities"):
        ctx.retry_wait_outcomes_dev(device, 0, 0, 10, 0.01, 0.0, 0.0, 0.7, 0.7, 0.0, 256, buf, 6)
    buf.free()
    hand = HandMade()
    blank = lambda rows: np.zeros((rows, 2, 2), dtype=np.uint64)
    for kwargs, text in ((dict(wait_eff=blank(513), wait_count=[513, 0]), "gf2_retry_wait_create: region 0 of block type 0 has 513 wait rows"),
                         (dict(wait_eff=blank(7), wait_count=[0, 7]), "gf2_retry_wait_create: region 1 of block type 0 is not retried but has 7 wait rows")):
        with pytest.raises(_native.GF2Error, match=text):
            ctx.retry_wait_create(*hand.arguments(**kwargs))
    wide = np.array(hand.wait_eff)                                                   # a wait row with a bit outside the layout of r = 3
    wide[5, 0, 0] |= np.uint64(1 << 20)
    device = ctx.retry_wait_create(*hand.arguments(wait_eff=wide))
    with pytest.raises(_native.GF2Error, match="gf2_mc_retry_wait_decode: the effects set bits beyond the layout"):
        ctx.mc_retry_wait_decode(device, r1, keys1, flips1, r2, keys2, flips2, 0, 0, 10, 0.01, 0.0, 0.0, 0.01, 0.0, 0.0, 256)
    device.free()
