"""
The repeat-until-success sampler under gate-level faults with waiting faults (DESIGN.md section 5d "Repeat-until-success with waiting
faults under gate-level faults") without a GPU: the refusals of the shared argument check, gf2_retry_gate_wait_words_host against the
NumPy restatement tests/retry_gate_wait_ref.py bit for bit, consequences 1, 2 and 5 of the definition against the two routes it
joins, and the host statement's samples against exact distributions (oracle/exact_dist.py, its thresholds as they are).
"""
import functools

import numpy as np
import pytest

from oracle import exact_dist
from quantum_css_codes_amd import _native
from tests import retry_gate_ref, retry_gate_wait_ref, retry_ref
from tests.test_retry import rates
from tests.test_retry_gate import prepare_final
from tests.test_retry_wait import EC, FINAL, HandMade
from tests.test_stream import streamed


# -- a sequence made by hand, with a site table --------------------------------------------------------------------------------------

class HandMadeGate(HandMade):
    """tests/test_retry_wait.py's HandMade with sites: the retried region of 30 locations is 10 one-operand sites and 10 CNOTs, the
    other of 10 locations 4 one-operand sites and 3 CNOTs; site locations are type-local."""

    def __init__(self, wait_rows=512, ntypes=1, seed=0):
        super().__init__(wait_rows, ntypes, seed)
        one = np.concatenate([np.arange(10), 10 + 2 * np.arange(10), 30 + np.arange(4), 34 + 2 * np.arange(3)])
        self.site_loc = np.tile(one, ntypes).astype(np.int32)
        self.site_regions = np.array([(10, 10), (4, 3)] * ntypes, dtype=np.int64)

    def arguments(self, wait_eff=None, wait_count=None):
        return self.sequence + (self.regions, self.nregions, self.site_loc, self.site_regions, self.wait_eff if wait_eff is None else wait_eff,
                                self.wait_count if wait_count is None else wait_count)

    def words_host(self, count, p1, p2, q, seed=0, first=0, max_attempts=256, **kwargs):
        return _native.retry_gate_wait_words_host(*self.arguments(**kwargs), seed, first, count, p1, p2, *q, max_attempts, self.ldw + 2,
                                                  self.preparations)

    def restated(self, count, p1, p2, q, seed=0, first=0, max_attempts=256):
        eff = self.sequence[0]
        types = [(eff[40 * t:40 * t + 40], self.regions[:2], 5, self.site_loc[:27], self.site_regions[:2]) for t in range(self.preparations)]
        rows = len(self.wait_eff) // self.preparations
        waits = [(self.wait_eff[rows * t:rows * (t + 1)], self.wait_count[:2]) for t in range(self.preparations)]
        return retry_gate_wait_ref.retry_gate_wait_words(types, self.sequence[3], self.sequence[4], waits, seed, first, count, p1, p2, q, max_attempts)


def many_wait_sizes(sizes):
    """A type of len(sizes) retried one-location regions, each one one-operand site with a flag row of its own and sizes[k] wait
    rows: the arguments up to wait_count, and the pitch of its words."""
    sizes = np.asarray(sizes, dtype=np.int64)
    n = len(sizes)
    eff = np.zeros((n, 2, 3), dtype=np.uint64)
    eff[:, :, 2] = (np.uint64(1) << np.arange(n, dtype=np.uint64))[:, None]
    regions = np.stack([np.arange(n), np.ones(n, dtype=np.int64), np.ones(n, dtype=np.int64)], axis=1)
    sites = np.stack([np.ones(n, dtype=np.int64), np.zeros(n, dtype=np.int64)], axis=1)
    return (eff, [n], [n], [0, -1], [EC, FINAL], regions, [n], np.arange(n, dtype=np.int32), sites,
            np.zeros((int(sizes.sum()), 2, 2), dtype=np.uint64), sizes)


# -- refusals ----------------------------------------------------------------------------------------------------------------------

def test_refusals():
    who = "gf2_retry_gate_wait_words_host: "
    hand, q = HandMadeGate(), rates(1e-2)
    blank = lambda rows: np.zeros((rows, 2, 2), dtype=np.uint64)
    for kwargs, text in ((dict(wait_eff=blank(513), wait_count=[513, 0]), "region 0 of block type 0 has 513 wait rows, a region holds 0 <= wait rows <= 512"),
                         (dict(wait_eff=blank(0), wait_count=[-1, 0]), "region 0 of block type 0 has -1 wait rows, a region holds 0 <= wait rows <= 512"),
                         (dict(wait_eff=blank(7), wait_count=[0, 7]), "region 1 of block type 0 is not retried but has 7 wait rows")):
        with pytest.raises(_native.GF2Error) as err:
            hand.words_host(1, 1e-2, 1e-2, q, **kwargs)
        assert who + text in str(err.value), str(err.value)
    words, attempts = hand.words_host(4, 1e-2, 1e-2, q)                          # 512 rows pass
    assert words.shape == (4, hand.ldw + 2) and attempts.shape == (4, 1)
    # the distinct wait sizes: one more than the cap is refused, the cap itself passes
    cap = _native.RETRY_GATE_WAIT_MAX_SIZES
    assert cap == 3
    with pytest.raises(_native.GF2Error) as err:
        _native.retry_gate_wait_words_host(*many_wait_sizes(np.arange(1, cap + 2)), 0, 0, 1, 1e-2, 1e-2, *q, 256, 5, cap + 1)
    assert who + "the regions have more than GF2_RETRY_GATE_WAIT_MAX_SIZES = 3 distinct wait sizes, one inverse-CDF table each" in str(err.value)
    words, _ = _native.retry_gate_wait_words_host(*many_wait_sizes([1, 2, 3, 2]), 0, 0, 3, 0.0, 0.0, *q, 256, 5, 4)   # three sizes on four regions
    assert words.shape == (3, 5) and not words[:, :3].any() and np.all(words[:, 3] == 4)
    # the q rates go through gf2_retry_wait_check_rates, p_1, p_2 and the range through gf2_gate_check_mc
    for bad in ((-1e-3, 0.0, 0.0), (0.5, 0.5, 0.5), (float("nan"), 0.0, 0.0)):
        with pytest.raises(_native.GF2Error) as err:
            hand.words_host(1, 1e-2, 1e-2, bad)
        assert who + "the waiting probabilities must be non-negative and sum to at most 1" in str(err.value), str(err.value)
    for p1, p2 in ((1.5, 1e-2), (1e-2, -0.1), (float("nan"), 1e-2)):
        with pytest.raises(_native.GF2Error) as err:
            hand.words_host(1, p1, p2, q)
        assert who + "needs 0 <= p_1, p_2 <= 1, got p_1 = " in str(err.value), str(err.value)
    with pytest.raises(_native.GF2Error) as err:
        hand.words_host(1, 1e-2, 1e-2, q, first=-1)
    assert who + "negative range (needs count >= 0 and first_sample >= 0)" in str(err.value)
    # gf2_retry_gate_plan's rules come first, named for this entry point
    with pytest.raises(_native.GF2Error, match=who + "needs 1 <= max_attempts <= 65536, got 0"):
        hand.words_host(1, 1e-2, 1e-2, q, max_attempts=0)
    args = list(hand.arguments())
    args[8] = np.array([(11, 10), (4, 3)])
    with pytest.raises(_native.GF2Error) as err:
        _native.retry_gate_wait_words_host(*args[:7], np.resize(hand.site_loc, 28), *args[8:], 0, 0, 1, 1e-2, 1e-2, *q, 256, 5, 1)
    assert who + "region 0 of block type 0 has n_1 + 2 n_2 = 11 + 2 * 10 sites' locations, not its 30 locations" in str(err.value)
    with pytest.raises(_native.GF2Error, match=who + r"ldw must be at least the sequence's nsteps \+ F \+ 2 = 5 words"):
        _native.retry_gate_wait_words_host(*hand.arguments(), 0, 0, 1, 1e-2, 1e-2, *q, 256, 4, 1)
    with pytest.raises(ValueError, match="one wait count per region"):
        hand.words_host(1, 1e-2, 1e-2, q, wait_count=[512])


def test_the_location_route_keeps_its_own_cap_and_message():
    """gf2_retry_wait_plan and gf2_retry_gate_wait_plan share the wait rules; the location route still takes 16 sizes."""
    args = many_wait_sizes([1, 2, 3, 4])
    location = args[:7] + args[9:]
    words, _ = _native.retry_wait_words_host(*location, 0, 0, 2, *rates(0.0), *rates(1e-2), 256, 5, 4)
    assert words.shape == (2, 5) and np.all(words[:, 3] == 4)


# -- the host statement against the restatement ------------------------------------------------------------------------------------

#             gadget, p1 = p2, q_kind, count, seed, first_sample, max_attempts, wait_steps
HOST_CASES = {"steane 2 rounds": (lambda: streamed("steane", "cycle", (2, False)), 3e-3, 1e-3, 3000, 5, 1 << 40, 256, 1),
              "rm15 1 round": (lambda: streamed("rm15", "cycle", (1, False)), 2e-3, 2e-3, 1000, 6, 0, 256, 1),
              "steane XY": (lambda: streamed("steane", "program", "XY"), 2e-3, 1e-3, 1500, 7, 3, 256, 1),
              "prepare, FINAL": (prepare_final, 1e-2, 3e-3, 3000, 8, 11, 256, 1),
              "steane 2 rounds, 3 attempts": (lambda: streamed("steane", "cycle", (2, False)), 3e-3, 3e-3, 3000, 9, 0, 3, 1),
              "steane 2 rounds, 2 wait steps": (lambda: streamed("steane", "cycle", (2, False)), 3e-3, 3e-3, 3000, 10, 0, 256, 2)}


@pytest.mark.parametrize("case", sorted(HOST_CASES))
def test_host_statement_equals_the_restatement(case):
    make, p, q_kind, count, seed, first, max_attempts, wait_steps = HOST_CASES[case]
    gadget, q = make(), rates(q_kind)
    words, attempts = gadget.retry_gate_wait_words_host(count, p, p, *q, seed=seed, first_sample=first, wait_steps=wait_steps, max_attempts=max_attempts)
    want_words, want_attempts = retry_gate_wait_ref.retry_gate_wait_words(*retry_gate_wait_ref.tables_of(gadget, wait_steps), seed, first, count, p, p, q,
                                                                          max_attempts)
    assert words.shape == (count, gadget.ldw + 2) and attempts.shape == (count, gadget.preparations)
    assert np.array_equal(words, want_words) and np.array_equal(attempts, want_attempts)
    assert np.array_equal(words[:, -2], attempts.sum(axis=1, dtype=np.uint64))
    assert (attempts > 1).any(axis=1).sum() * 4 >= count                        # not vacuous: a quarter of the samples took a retry
    exhausted = words[:, gadget.nsteps:gadget.ldw].any(axis=1)
    assert exhausted.any() == (max_attempts == 3)
    faults = int(words[:, -1].sum(dtype=np.uint64))
    if case == "prepare, FINAL":
        assert faults == 0 and gadget.wait_locations() == 0                      # the data block is what is being prepared
    else:                                                                        # not vacuous: wait faults in a twentieth of the samples at least
        assert (words[:, -1] > 0).sum() * 20 >= count and (words[exhausted, -1] > 0).any() == exhausted.any()
        plain, _ = gadget.retry_gate_words_host(count, p, p, seed=seed, first_sample=first, max_attempts=max_attempts)
        assert (words[:, :gadget.nsteps] != plain[:, :gadget.nsteps]).any(axis=1).sum() * 30 >= count   # ... and they reach the step words


def test_floyds_rule_on_a_region_of_512_wait_rows():
    hand, q = HandMadeGate(), rates(1e-2)
    words, attempts = hand.words_host(1500, 2e-2, 2e-2, q, seed=11, first=5)
    want_words, want_attempts = hand.restated(1500, 2e-2, 2e-2, q, seed=11, first=5)
    assert np.array_equal(words, want_words) and np.array_equal(attempts, want_attempts)
    assert words[:, -1].sum() > 1500 * 512 * 0.03 and (attempts > 1).mean() > 0.25   # K = 15 per attempt on average, retries in a quarter at least
    several = HandMadeGate(wait_rows=100, ntypes=3, seed=1)
    words, attempts = several.words_host(500, 2e-2, 2e-2, q, seed=12)
    want_words, want_attempts = several.restated(500, 2e-2, 2e-2, q, seed=12)
    assert np.array_equal(words, want_words) and np.array_equal(attempts, want_attempts)


def test_wider_pitch_and_no_attempts_array():
    gadget = streamed("steane", "cycle", (2, False))
    words, _ = gadget.retry_gate_wait_words_host(50, 3e-3, 3e-3, *rates(3e-3), seed=1)
    wide = np.full((50, gadget.ldw + 4), 0xABCD, dtype="<u8")
    seq = _native._stream_sequence(*gadget._sequence())[1]
    regions = _native._retry_regions(gadget.type_regions, gadget.type_nregions, 1)[1]
    keep_sites, sites = _native._retry_sites(gadget.type_site_loc, gadget.type_site_regions, 4)
    keep, waits = _native._retry_waits(*gadget._retry_wait_sequence()[-2:], 4)
    _native.check(_native.lib().gf2_retry_gate_wait_words_host(*seq, *regions, *sites, *waits, 1, 0, 50, 3e-3, 3e-3, 3e-3, 3e-3, 3e-3, 256,
                                                               wide.ctypes.data, gadget.ldw + 4, None))
    assert np.array_equal(wide[:, :gadget.ldw + 2], words) and np.all(wide[:, gadget.ldw + 2:] == 0xABCD)
    assert gadget.retry_gate_wait_words_host(0, 3e-3, 3e-3, *rates(3e-3))[0].shape == (0, gadget.ldw + 2)


# -- consequences 1, 2 and 5 -------------------------------------------------------------------------------------------------------

COUNT = 4096


@pytest.mark.parametrize("make", [lambda: streamed("steane", "cycle", (2, False)), lambda: streamed("steane", "program", "XY"), prepare_final],
                         ids=["cycle", "program", "prepare"])
def test_consequence_1_no_waiting_faults_is_the_gate_level_retried_route(make):
    gadget, p = make(), 3e-3
    for q, steps, limit in ((rates(0.0), 1, 256), (rates(0.0), 2, 3)) + (((rates(1e-2), 1, 256),) if gadget.wait_locations() == 0 else ()):
        plain, plain_attempts = gadget.retry_gate_words_host(COUNT, p, p, seed=3, first_sample=7, max_attempts=limit)
        words, attempts = gadget.retry_gate_wait_words_host(COUNT, p, p, *q, seed=3, first_sample=7, wait_steps=steps, max_attempts=limit)
        assert np.array_equal(words[:, :-1], plain) and not words[:, -1].any() and np.array_equal(attempts, plain_attempts)
        assert np.array_equal(gadget.tally_host(words[:, :gadget.ldw], fields=True), gadget.tally_host(plain[:, :gadget.ldw], fields=True))


@pytest.mark.parametrize("limit", [256, 3])
def test_consequence_2_the_attempts_are_those_of_the_gate_level_retried_route(limit):
    gadget, p = streamed("steane", "cycle", (2, False)), 3e-3
    plain, plain_attempts = gadget.retry_gate_words_host(COUNT, p, p, seed=4, max_attempts=limit)
    for q in (rates(3e-3), (0.02, 0.0, 0.01)):
        words, attempts = gadget.retry_gate_wait_words_host(COUNT, p, p, *q, seed=4, max_attempts=limit)
        assert np.array_equal(words[:, -2], plain[:, -1]) and np.array_equal(attempts, plain_attempts)
        flags, plain_flags = words[:, gadget.nsteps:gadget.ldw], plain[:, gadget.nsteps:gadget.ldw]
        assert np.array_equal(flags, plain_flags) and flags.any(axis=1).any() == (limit == 3)
        assert (words[:, :gadget.nsteps] != plain[:, :gadget.nsteps]).any()      # ... while the step words do differ


@pytest.mark.parametrize("make,steps", [(lambda: streamed("steane", "cycle", (2, False)), 1), (lambda: streamed("steane", "program", "XY"), 2)],
                         ids=["cycle", "program"])
def test_consequence_5_without_gate_faults_the_two_wait_routes_are_one(make, steps):
    gadget, q = make(), (0.02, 0.005, 0.01)
    words, attempts = gadget.retry_gate_wait_words_host(COUNT, 0.0, 0.0, *q, seed=6, first_sample=2, wait_steps=steps)
    location, location_attempts = gadget.retry_wait_words_host(COUNT, *rates(0.0), *q, seed=6, first_sample=2, wait_steps=steps)
    assert np.array_equal(words, location) and np.array_equal(attempts, location_attempts) and np.all(attempts == 1)
    assert (words[:, -1] > 0).sum() * 4 >= COUNT and words[:, :gadget.nsteps].any()   # not vacuous


# -- exact distributions -----------------------------------------------------------------------------------------------------------

SAMPLES = 200000
# The 14-bit joint at p1 = p2 = 1e-3, q_kind = 5e-4, the rates the definition's author started from: the share of the exact mass in
# cells that expect fewer than 10 of 2 x 10^5 samples is computed in the test and must stay below pooled_chi2's 1 %.
ONE_ROUND_P, ONE_ROUND_Q = 1e-3, 5e-4
# One Steane round: at p1 = p2 = 3e-3 the preparations pass with 0.81 and 0.83, so fewer than a quarter of them take a second attempt;
# p is raised to 5e-3, where they pass with about 0.70 and 0.73 (asserted from region_pass_probability in the test).
WAIT_Z_P, WAIT_Z_Q = 5e-3, 3e-3


@functools.lru_cache(maxsize=None)
def one_round_exact():
    return retry_gate_wait_ref.one_round_distribution(streamed("steane", "cycle", (1, False)), ONE_ROUND_P, ONE_ROUND_P, rates(ONE_ROUND_Q), 3, 3)


def test_wait_faults_follow_their_exact_mean_and_variance():
    gadget, p, q = streamed("steane", "cycle", (1, False)), WAIT_Z_P, rates(WAIT_Z_Q)
    block = gadget.types[0]
    passes = [retry_gate_ref.region_pass_probability(block, r, p, p) for r, row in enumerate(block.regions.tolist()) if row[2]]
    assert len(passes) == 2 and all(1.0 - s > 0.25 for s in passes), passes       # more than a quarter of the preparations take a second attempt
    mean, var, once, _ = retry_gate_wait_ref.wait_faults_mean_var(gadget, p, p, q)
    assert abs(mean - once) * SAMPLES > 5.0 * (SAMPLES * var) ** 0.5             # waits on every attempt are told from waits on the accepted one
    words, _ = gadget.retry_gate_wait_words_host(SAMPLES, p, p, *q, seed=24)
    assert not words[:, gadget.nsteps:gadget.ldw].any()                         # (truncation at 256 attempts: below 1e-100)
    exact_dist.assert_z("gate faults: wait faults of one Steane round at p = %g, mean %.4f per sample (%.4f if only the accepted attempt waited)"
                        % (WAIT_Z_P, mean, once), int(words[:, -1].sum(dtype=np.uint64)), SAMPLES * mean, SAMPLES * var)


def test_one_round_follows_the_convolution_with_the_wait_noise():
    gadget, p, q = streamed("steane", "cycle", (1, False)), ONE_ROUND_P, rates(ONE_ROUND_Q)
    exact = one_round_exact()
    assert exact.shape == (1 << 14,)
    share = retry_gate_ref.sparse_share(exact, SAMPLES)                           # from the exact distribution, not from the samples
    assert share < exact_dist.MAX_REST_MASS, share
    words, _ = gadget.retry_gate_wait_words_host(SAMPLES, p, p, *q, seed=25)
    assert not words[:, 2].any()
    plain, _ = gadget.retry_gate_words_host(SAMPLES, p, p, seed=25)              # not vacuous: the wait noise moves a percent of the samples
    assert (retry_ref.one_round_cells(words, 3, 3) != retry_ref.one_round_cells(plain, 3, 3)).mean() > 0.01
    exact_dist.assert_chi2("gate faults: (round word, T) of one Steane round with waiting faults",
                           np.bincount(retry_ref.one_round_cells(words, 3, 3), minlength=1 << 14), exact, SAMPLES)
