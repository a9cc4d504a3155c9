"""
The repeat-until-success sampler under gate-level faults with waiting faults on the device (csrc/gf2_retry_gate_wait.hip, DESIGN.md
section 5d "Repeat-until-success with waiting faults under gate-level faults"): the stored words and the fifteen counts bit for bit
against the host statement (itself checked against tests/retry_gate_wait_ref.py in tests/test_retry_gate_wait.py) on every path of
the kernel, consequences 1 and 2 against the gate-level retried kernel, consequence 5 against the location version's wait kernel,
the exact distributions of tests/test_retry_gate_wait.py at 2^26 samples, consequence 3 against gate-level post-selection of block
types that hold the waiting IDLEs as ordinary gates, and a run of a thousand rounds.  Statistical verdicts are oracle/exact_dist.py's,
thresholds as they are.
"""
import numpy as np
import pytest

from oracle import exact_dist
from quantum_css_codes_amd import _native
from tests import retry_gate_ref, retry_gate_wait_ref, retry_ref, retry_wait_ref
from tests.state_check import DirtyBuffer, Layout
from tests.test_gpu_stream import make_code, streamed
from tests.test_retry import rates
from tests.test_retry_gate_wait import ONE_ROUND_P, ONE_ROUND_Q, WAIT_Z_P, WAIT_Z_Q, HandMadeGate, many_wait_sizes, one_round_exact
from tests.test_retry_wait import waited_cycle

pytestmark = pytest.mark.gpu

BIG = 1 << 26
COUNT = 4096


def host_counts(gadget, words):
    """The fifteen counts the host statement gives: gf2_stream_tally_host on the first nsteps + F words, the exhausted, the attempts,
    the wait faults."""
    fields = [int(v) for v in gadget.tally_host(words[:, :gadget.ldw], fields=True)]
    return fields + [len(words) - fields[0], int(words[:, -2].sum(dtype=np.uint64)), int(words[:, -1].sum(dtype=np.uint64))]


#        code, what, key, p1, p2, q_kind, wait_steps, max_attempts, seed, first_sample
CASES = {
    "steane-2": ("steane", "cycle", (2, False), 3e-3, 3e-3, 3e-3, 1, 256, 1, 0),              # 16 KB of tables: staged
    "rm15-3": ("rm15", "cycle", (3, False), 2e-3, 2e-3, 2e-3, 1, 256, 2, 5),                  # staged; 15 wait rows per preparation
    "rm15-XYZ": ("rm15", "program", ("X", "Y", "Z"), 1e-3, 1e-3, 1e-3, 1, 256, 3, 0),         # six types, 190 KB: read through L2
    "program-XY": ("steane", "program", ("X", "Y"), 2e-3, 2e-3, 2e-3, 1, 256, 5, 3),          # a NONE block without wait rows, MEASURE steps
    "idle": ("steane", "cycle", (2, True), 3e-3, 3e-3, 3e-3, 1, 256, 6, 0),
    "two wait steps": ("steane", "cycle", (2, False), 3e-3, 3e-3, 3e-3, 2, 256, 7, 0),
    "one attempt": ("steane", "cycle", (2, False), 3e-3, 3e-3, 3e-3, 1, 1, 8, 0),             # exhausted lanes inside accepted wavefronts
    "three attempts": ("steane", "cycle", (2, False), 1e-2, 1e-2, 3e-3, 1, 3, 9, 0),
    "no gate noise": ("steane", "cycle", (3, False), 0.0, 0.0, 3e-3, 1, 256, 10, 0),          # p = 0 with q > 0: waiting faults alone
    "no wait noise": ("steane", "cycle", (2, False), 3e-3, 3e-3, 0.0, 1, 256, 11, 0),         # q = 0
    "no one-operand faults": ("steane", "cycle", (2, False), 0.0, 6e-3, 3e-3, 1, 256, 13, 0),
    "no CNOT faults": ("steane", "cycle", (2, False), 6e-3, 0.0, 3e-3, 1, 256, 14, 0),
    "first 2^33": ("steane", "cycle", (2, False), 3e-3, 3e-3, 3e-3, 1, 256, 12, 1 << 33),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_words_and_counts_equal_the_host_statement(case):
    name, what, key, p1, p2, q_kind, steps, max_attempts, seed, first = CASES[case]
    gadget, q = streamed(name, what, key), rates(q_kind)
    more = dict(seed=seed, first_sample=first, wait_steps=steps, max_attempts=max_attempts)
    want, _ = gadget.retry_gate_wait_words_host(COUNT, p1, p2, *q, **more)
    words = gadget.retry_gate_wait_outcomes(COUNT, p1, p2, *q, **more)
    assert words.shape == (COUNT, gadget.ldw + 2) and np.array_equal(words, want)
    counts = host_counts(gadget, want)
    assert [int(v) for v in gadget.retry_gate_wait_counts(COUNT, p1, p2, *q, **more)] == counts
    if case == "rm15-XYZ":
        assert gadget.type_eff.nbytes + gadget.type_site_loc.nbytes > 160 * 1024
    if case in ("one attempt", "three attempts"):
        assert COUNT // 100 < counts[12] < COUNT - COUNT // 100 and COUNT // 100 < counts[0]   # both kinds of lanes in the wavefronts
    elif case == "no gate noise":
        assert counts[0] == COUNT and counts[13] == COUNT * gadget.preparations and counts[14] > 0 and sum(counts[1:12]) > 0
    else:
        assert counts[12] == 0 and counts[13] * 20 > COUNT * gadget.preparations * 21 and sum(counts[1:12]) > 0
    assert (counts[14] == 0) == (case == "no wait noise")
    got = gadget.retry_gate_wait_error_rates(COUNT, p1, p2, *q, **more)
    assert got['accepted'] == counts[0] and got['exhausted'] == counts[12] and got['attempts'] == counts[13] and got['wait_faults'] == counts[14]
    assert got['samples'] == COUNT and got['preparations'] == gadget.preparations and got['wait_locations'] == gadget.wait_locations(steps)


@pytest.mark.parametrize("ntypes", [1, 11], ids=["512 rows", "11 x 512 rows"])
def test_sequences_made_by_hand(ntypes):
    """A region of 512 wait rows at q_kind = 0.01 (K = 15 per attempt: Floyd's rule); eleven of them are 180 KB of wait rows, which
    the kernel reads through L2 while the block tables stay staged."""
    ctx = _native.default_context()
    hand, q = HandMadeGate(ntypes=ntypes, seed=ntypes), rates(1e-2)
    assert (hand.wait_eff.nbytes > 160 * 1024) == (ntypes == 11) and hand.sequence[0].nbytes < 32 * 1024
    tables = streamed("steane", "cycle", (1, False))._tables()
    device = ctx.retry_gate_wait_create(*hand.arguments())
    want, _ = hand.words_host(COUNT, 2e-2, 2e-2, q, seed=21, first=3)
    buf = ctx.alloc(COUNT * (hand.ldw + 2) * 8)
    ctx.retry_gate_wait_outcomes_dev(device, 21, 3, COUNT, 2e-2, 2e-2, *q, 256, buf, hand.ldw + 2)
    words = buf.download((COUNT, hand.ldw + 2), np.uint64)
    buf.free()
    assert np.array_equal(words, want)
    fields = [int(v) for v in _native.stream_tally_host(want[:, :hand.ldw], hand.block_kind, 1, *tables)]
    counts = fields + [COUNT - fields[0], int(want[:, -2].sum(dtype=np.uint64)), int(want[:, -1].sum(dtype=np.uint64))]
    assert [int(v) for v in ctx.mc_retry_gate_wait_decode(device, *tables, 21, 3, COUNT, 2e-2, 2e-2, *q, 256)] == counts
    assert counts[14] > COUNT * ntypes * 512 * 0.03 and counts[13] > COUNT * ntypes * 1.25
    device.free()


def test_tiny_counts_pitch_and_code_level_entry_points():
    ctx = _native.default_context()
    gadget, p, q = streamed("steane", "cycle", (2, False)), 3e-3, rates(2e-3)
    want, _ = gadget.retry_gate_wait_words_host(300, p, p, *q, seed=12)
    assert [int(v) for v in gadget.retry_gate_wait_counts(0, p, p, *q, seed=12)] == [0] * 15
    assert gadget.retry_gate_wait_outcomes(0, p, p, *q).shape == (0, gadget.ldw + 2)
    for i in range(3):                                                               # count = 1, sample by sample
        assert np.array_equal(gadget.retry_gate_wait_outcomes(1, p, p, *q, seed=12, first_sample=i), want[i:i + 1])
        assert [int(v) for v in gadget.retry_gate_wait_counts(1, p, p, *q, seed=12, first_sample=i)] == host_counts(gadget, want[i:i + 1])
    buf = DirtyBuffer(ctx, Layout(300, gadget.ldw + 5, 264))                         # a wider pitch at an address that is 8 mod 16
    ctx.retry_gate_wait_outcomes_dev(gadget.retry_gate_wait_device(), 12, 0, 300, p, p, *q, 256, buf.view, gadget.ldw + 5)
    buf.check(want, preserved=True, what="gf2_retry_gate_wait_outcomes_dev")         # the padding is left as it was, whatever it held
    buf.free()
    code = make_code("steane")
    got = code.error_correct_retried_gate_wait_error_rates(COUNT, p, p, *q, rounds=2, seed=1)
    assert got == gadget.retry_gate_wait_error_rates(COUNT, p, p, *q, seed=1) and got['accepted'] == COUNT and got['wait_locations'] == 28
    assert code.error_correct_retried_gate_wait_error_rates(COUNT, p, p, *q, rounds=2, seed=1, idle_data=True, wait_steps=2) == \
        streamed("steane", "cycle", (2, True)).retry_gate_wait_error_rates(COUNT, p, p, *q, seed=1, wait_steps=2)
    program = streamed("steane", "program", ("X", "Y"))
    assert code.logical_program_retried_gate_wait_error_rates("XY", COUNT, p, p, *q, seed=5, first_sample=3) == \
        program.retry_gate_wait_error_rates(COUNT, p, p, *q, seed=5, first_sample=3)
    assert set(program.retry_gate_wait_error_rates(16, p, p, *q)) == {'accepted', 'wrong', 'trial_wrong', 'first_trial_wrong', 'split_vote', 'unmatched_x',
                                                                      'unmatched_z', 'samples', 'exhausted', 'attempts', 'preparations', 'wait_faults',
                                                                      'wait_locations'}


# -- consequences 1, 2 and 5 against the kernels of the two routes this one joins -------------------------------------------------------

@pytest.mark.parametrize("name,what,key,p,limit", [("steane", "cycle", (2, False), 3e-3, 256), ("steane", "cycle", (2, False), 1e-2, 3),
                                                   ("rm15", "program", ("X", "Y", "Z"), 1e-3, 256)])
def test_consequences_1_and_2_against_the_gate_level_retried_kernel(name, what, key, p, limit):
    gadget = streamed(name, what, key)
    plain = gadget.retry_gate_outcomes(COUNT, p, p, seed=15, first_sample=9, max_attempts=limit)
    plain_counts = [int(v) for v in gadget.retry_gate_counts(COUNT, p, p, seed=15, first_sample=9, max_attempts=limit)]
    for steps in (1, 2):                                                             # 1: q = 0 is the gate-level route, bit for bit
        words = gadget.retry_gate_wait_outcomes(COUNT, p, p, *rates(0.0), seed=15, first_sample=9, wait_steps=steps, max_attempts=limit)
        assert np.array_equal(words[:, :-1], plain) and not words[:, -1].any()
        counts = gadget.retry_gate_wait_counts(COUNT, p, p, *rates(0.0), seed=15, first_sample=9, wait_steps=steps, max_attempts=limit)
        assert [int(v) for v in counts] == plain_counts + [0]
    q = (2e-2, 0.0, 1e-2)                                                            # 2: any q leaves the attempts and the exhausted as they are
    words = gadget.retry_gate_wait_outcomes(COUNT, p, p, *q, seed=15, first_sample=9, max_attempts=limit)
    assert np.array_equal(words[:, gadget.nsteps:gadget.ldw + 1], plain[:, gadget.nsteps:])      # the flag words and the attempts
    assert (words[:, :gadget.nsteps] != plain[:, :gadget.nsteps]).any() and words[:, -1].any()
    counts = [int(v) for v in gadget.retry_gate_wait_counts(COUNT, p, p, *q, seed=15, first_sample=9, max_attempts=limit)]
    assert counts[0] == plain_counts[0] and counts[12:14] == plain_counts[12:14] and (counts[12] > 0) == (limit == 3)


@pytest.mark.parametrize("name,what,key,steps", [("steane", "cycle", (2, False), 1), ("steane", "program", ("X", "Y"), 2)])
def test_consequence_5_without_gate_faults_the_two_wait_kernels_agree(name, what, key, steps):
    gadget, q = streamed(name, what, key), (0.02, 0.005, 0.01)
    more = dict(seed=16, first_sample=4, wait_steps=steps)
    words = gadget.retry_gate_wait_outcomes(COUNT, 0.0, 0.0, *q, **more)
    assert np.array_equal(words, gadget.retry_wait_outcomes(COUNT, *rates(0.0), *q, **more)) and words[:, -1].any()
    counts = [int(v) for v in gadget.retry_gate_wait_counts(COUNT, 0.0, 0.0, *q, **more)]
    assert counts == [int(v) for v in gadget.retry_wait_counts(COUNT, *rates(0.0), *q, **more)] and counts[14] > 0 and sum(counts[1:12]) > 0


def test_shards_add_up_and_no_state_between_calls():
    gadget, p, q = streamed("steane", "cycle", (3, False)), 2e-3, rates(1e-3)
    whole = gadget.retry_gate_wait_counts(2 * 20000 + 7, p, p, *q, seed=14, first_sample=100)
    first = gadget.retry_gate_wait_counts(20000, p, p, *q, seed=14, first_sample=100)
    # unrelated calls in between -- other rates, other wait steps, another sequence, the two routes this one joins
    streamed("rm15", "cycle", (3, False)).retry_gate_wait_counts(3000, 1e-3, 1e-3, *rates(1e-3), seed=1)
    gadget.retry_gate_wait_counts(3000, 5e-3, 5e-3, *rates(1e-2), seed=2, wait_steps=3, max_attempts=3)
    gadget.retry_gate_counts(3000, 4e-3, 4e-3, seed=3)
    gadget.retry_wait_counts(3000, *rates(4e-3), *rates(4e-3), seed=3)
    second = gadget.retry_gate_wait_counts(20007, p, p, *q, seed=14, first_sample=20100)
    assert [int(v) for v in whole] == [int(first[f]) + int(second[f]) for f in range(15)]
    assert np.array_equal(gadget.retry_gate_wait_counts(2 * 20000 + 7, p, p, *q, seed=14, first_sample=100), whole)


def test_results_do_not_depend_on_what_the_buffer_held():
    ctx = _native.default_context()
    gadget, p, q = streamed("steane", "cycle", (2, False)), 1e-2, rates(3e-3)
    want, _ = gadget.retry_gate_wait_words_host(500, p, p, *q, seed=17, max_attempts=3)
    assert want[:, gadget.nsteps:gadget.ldw].any()                                   # exhausted samples: their step words are written as zero
    buf = DirtyBuffer(ctx, Layout(500, gadget.ldw + 2))
    ctx.retry_gate_wait_outcomes_dev(gadget.retry_gate_wait_device(), 17, 0, 500, p, p, *q, 3, buf.view, gadget.ldw + 2)
    buf.check(want, preserved=True, what="gf2_retry_gate_wait_outcomes_dev, exact pitch")
    buf.free()


# -- exact distributions at 2^26 samples -------------------------------------------------------------------------------------------

def test_wait_faults_follow_their_exact_mean_and_variance():
    gadget, p, q = streamed("steane", "cycle", (1, False)), WAIT_Z_P, rates(WAIT_Z_Q)
    mean, var, once, _ = retry_gate_wait_ref.wait_faults_mean_var(gadget, p, p, q)
    assert abs(mean - once) * BIG > 5.0 * (BIG * var) ** 0.5
    counts = gadget.retry_gate_wait_counts(BIG, p, p, *q, seed=34)
    assert int(counts[12]) == 0 and int(counts[0]) == BIG                            # (truncation at 256 attempts: below 1e-100)
    exact_dist.assert_z("gate faults: wait faults of one Steane round at p = %g, device, mean %.4f per sample" % (WAIT_Z_P, mean), int(counts[14]),
                        BIG * mean, BIG * var)


def test_one_round_follows_the_convolution_with_the_wait_noise():
    gadget, p, q = streamed("steane", "cycle", (1, False)), ONE_ROUND_P, rates(ONE_ROUND_Q)
    exact = one_round_exact()
    assert retry_gate_ref.sparse_share(exact, BIG) < exact_dist.MAX_REST_MASS
    got = np.zeros(1 << 14, dtype=np.int64)
    for start in range(0, BIG, 1 << 22):
        words = gadget.retry_gate_wait_outcomes(1 << 22, p, p, *q, seed=35, first_sample=start)
        assert not words[:, gadget.nsteps:gadget.ldw].any()
        got += np.bincount(retry_ref.one_round_cells(words, 3, 3), minlength=1 << 14)
    exact_dist.assert_chi2("gate faults: (round word, T) of one Steane round with waiting faults, device", got, exact, BIG)


def test_consequence_3_one_attempt_is_gate_level_post_selection_of_the_waited_block_types():
    """max_attempts = 1 and q_kind = p1 / 3: the accepted samples have the distribution of the gate-level retried route with one
    attempt on the block type with the waiting IDLEs as ordinary one-operand gates."""
    gadget, waited, p = streamed("steane", "cycle", (1, False)), waited_cycle(make_code("steane")), 1e-3
    assert waited.num_locations == gadget.num_locations + gadget.wait_locations()
    retried = gadget.retry_gate_wait_error_rates(BIG, p, p, *rates(p / 3.0), seed=41, max_attempts=1)
    selected = waited.retry_gate_error_rates(BIG, p, p, seed=42, max_attempts=1)
    n_1, n_2 = float(retried['accepted']), float(selected['accepted'])
    assert retried['accepted'] + retried['exhausted'] == BIG and BIG // 2 < retried['accepted'] < BIG and BIG // 2 < selected['accepted'] < BIG
    pooled = (n_1 + n_2) / (2.0 * BIG)
    exact_dist.assert_z("gate faults: accepted fraction, one attempt - post-selected", n_1 / BIG - n_2 / BIG, 0.0, pooled * (1.0 - pooled) * 2.0 / BIG)
    for field in ('logical_x', 'logical_z', 'logical_any', 'round_unmatched_x', 'round_unmatched_z'):
        a, b = retried[field], selected[field]
        pooled = (a + b) / (n_1 + n_2)
        var = pooled * (1.0 - pooled) * (1.0 / n_1 + 1.0 / n_2)                      # of the difference of the two rates under the pooled rate
        exact_dist.assert_z("gate faults: %s per accepted sample, one attempt with waiting faults - post-selected" % field, a / n_1 - b / n_2, 0.0, var)


def test_a_thousand_rounds():
    gadget, p, q = streamed("steane", "cycle", (1000, False)), 1e-3, rates(1e-3 / 3.0)
    assert (gadget.nsteps, gadget.preparations, gadget.wait_locations()) == (1001, 2000, 14000)
    want, _ = gadget.retry_gate_wait_words_host(COUNT, p, p, *q, seed=13)
    counts = host_counts(gadget, want)
    assert counts[0] == COUNT and counts[12] == 0 and counts[3] > 0                  # every sample accepted
    assert [int(v) for v in gadget.retry_gate_wait_counts(COUNT, p, p, *q, seed=13)] == counts
    assert np.array_equal(gadget.retry_gate_wait_outcomes(64, p, p, *q, seed=13), want[:64])
    _, var, _, _ = retry_gate_wait_ref.wait_faults_mean_var(gadget, p, p, q)
    attempts = retry_gate_ref.attempts_mean_var(gadget, p, p)[0] / gadget.preparations
    scale = COUNT * gadget.wait_locations() * retry_wait_ref.quantised_total(q)      # wait faults per unit of attempts per preparation
    print("\nattempts per preparation: %.5f from the wait faults, %.5f exact" % (counts[14] / scale, attempts))
    exact_dist.assert_z("gate faults: wait faults / (samples x wait locations x q_t) against the attempts per preparation, 1000 rounds",
                        counts[14] / scale, attempts, COUNT * var / scale ** 2)


def test_argument_errors():
    ctx = _native.default_context()
    gadget = streamed("steane", "cycle", (2, False))
    r1, keys1, flips1, r2, keys2, flips2 = gadget._tables()
    device = gadget.retry_gate_wait_device()
    run = lambda a=r1, first=0, count=10, p1=0.01, p2=0.01, q=0.01, limit=256: ctx.mc_retry_gate_wait_decode(device, a, keys1, flips1, r2, keys2, flips2, 0,
                                                                                                             first, count, p1, p2, q, 0.0, 0.0, limit)
    assert int(run()[0]) + int(run()[12]) == 10
    who = "gf2_mc_retry_gate_wait_decode: "
    for kwargs, text in ((dict(a=32), "r_1, r_2 <= 31"), (dict(a=2), "bits beyond the layout"), (dict(first=-1), who + "negative range"),
                         (dict(p1=1.5), who + "needs 0 <= p_1, p_2 <= 1"), (dict(p2=-0.5), who + "needs 0 <= p_1, p_2 <= 1"),
                         (dict(q=1.5), who + "the waiting probabilities must be non-negative and sum to at most 1"),
                         (dict(q=-0.1), "the waiting probabilities"), (dict(limit=0), who + "needs 1 <= max_attempts <= 65536, got 0")):
        with pytest.raises(_native.GF2Error, match=text):
            run(**kwargs)
    buf = ctx.alloc(10 * (gadget.ldw + 2) * 8)
    with pytest.raises(_native.GF2Error, match=r"gf2_retry_gate_wait_outcomes_dev: ldo must be at least the sequence's nsteps \+ F \+ 2 = 6 words"):
        ctx.retry_gate_wait_outcomes_dev(device, 0, 0, 10, 0.01, 0.01, 0.01, 0.0, 0.0, 256, buf, 5)
    with pytest.raises(_native.GF2Error, match="gf2_retry_gate_wait_outcomes_dev: the waiting probabilities"):
        ctx.retry_gate_wait_outcomes_dev(device, 0, 0, 10, 0.01, 0.01, 0.7, 0.7, 0.0, 256, buf, 6)
    buf.free()
    hand = HandMadeGate()
    blank = lambda rows: np.zeros((rows, 2, 2), dtype=np.uint64)
    for kwargs, text in ((dict(wait_eff=blank(513), wait_count=[513, 0]), "gf2_retry_gate_wait_create: region 0 of block type 0 has 513 wait rows"),
                         (dict(wait_eff=blank(7), wait_count=[0, 7]), "gf2_retry_gate_wait_create: region 1 of block type 0 is not retried but has 7 wait rows")):
        with pytest.raises(_native.GF2Error, match=text):
            ctx.retry_gate_wait_create(*hand.arguments(**kwargs))
    with pytest.raises(_native.GF2Error, match="gf2_retry_gate_wait_create: the regions have more than GF2_RETRY_GATE_WAIT_MAX_SIZES = 3 distinct wait sizes"):
        ctx.retry_gate_wait_create(*many_wait_sizes([1, 2, 3, 4]))                   # host and device refuse alike
    ctx.retry_gate_wait_create(*many_wait_sizes([1, 2, 3, 2])).free()                # ... and the cap itself is accepted
    wide = np.array(hand.wait_eff)                                                   # a wait row with a bit outside the layout of r = 3
    wide[5, 0, 0] |= np.uint64(1 << 20)
    device = ctx.retry_gate_wait_create(*hand.arguments(wait_eff=wide))
    with pytest.raises(_native.GF2Error, match="gf2_mc_retry_gate_wait_decode: the effects set bits beyond the layout"):
        ctx.mc_retry_gate_wait_decode(device, r1, keys1, flips1, r2, keys2, flips2, 0, 0, 10, 0.01, 0.01, 0.01, 0.0, 0.0, 256)
    device.free()
