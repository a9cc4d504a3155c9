"""
The repeat-until-success sampler with waiting faults (DESIGN.md section 5d "Repeat-until-success with waiting faults") without a GPU:
the wait rows of the block types, the refusals of the shared argument check, gf2_retry_wait_words_host against the NumPy restatement
tests/retry_wait_ref.py bit for bit, consequences 1 and 2 of the definition against the plain retried route, and the host
statement's samples against exact distributions (oracle/exact_dist.py, its thresholds as they are).
"""
import numpy as np
import pytest

from oracle import exact_dist
from quantum_css_codes_amd import _native, stream_noise
from quantum_css_codes_amd.ec_noise import GATE_CNOT, GATE_H, GATE_IDLE, ROW_ROUND
from tests import retry_ref, retry_wait_ref
from tests.test_retry import prepare_final, rates
from tests.test_stream import oracle_code, streamed

EC, MEASURE, FINAL = stream_noise.EC, stream_noise.MEASURE, stream_noise.FINAL


# -- block types with the waiting IDLEs as ordinary locations ----------------------------------------------------------------------

def emit_ec_waited(wait_steps=1):
    """GadgetBuilder.error_correct with one IDLE per data qubit, wait_steps times, immediately before either preparation."""
    def emit(build):
        r_1, r_2 = build.r_1, build.r_2
        idle = lambda: build.gates.extend((GATE_IDLE, q, 0) for _ in range(wait_steps) for q in build.data)
        idle()
        build.prep(build.anc_1, 'plus', 1)
        build.gates.extend((GATE_CNOT, d, a) for d, a in zip(build.data, build.anc_1))
        build.measure(build.anc_1, build.h_2, ROW_ROUND, 1, [r_2 - 1 - i for i in range(r_2)])
        idle()
        build.prep(build.anc_1, 'zero', 1)
        build.gates.extend((GATE_CNOT, a, d) for d, a in zip(build.data, build.anc_1))
        build.gates.extend((GATE_H, a, 0) for a in build.anc_1)
        build.measure(build.anc_1, build.h_1, ROW_ROUND, 1, [32 + r_1 - 1 - i for i in range(r_1)])
    return emit


def emit_measure_waited(build):
    build.gates.extend((GATE_IDLE, q, 0) for q in build.data)
    stream_noise._emit_measure(build)


def waited_cycle(name, rounds=1):
    """The cycle whose EC block has the waiting IDLEs as ordinary locations: what post-selection sees of the waiting faults."""
    code = oracle_code(name) if isinstance(name, str) else name
    block = stream_noise.BlockType(code, "EC, waited", EC, emit_ec_waited())
    return stream_noise.StreamedGadget(code, "cycle", [block], [0] * rounds + [-1], [EC] * rounds + [FINAL])


# -- wait rows ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["steane", "rm15"])
def test_wait_rows_of_the_block_types(name):
    n = 7 if name == "steane" else 15
    code = oracle_code(name)
    program = streamed(name, "program", "X")
    types = {t.name: t for t in program.types}
    ec = streamed(name, "cycle", (1, False)).types[0]
    for block, want in ((ec, [n, 0, n, 0]), (types["EC"], [n, 0, n, 0]), (types["MEASURE trial"], [n, 0]), (types["prepare data"], [0]),
                        (streamed(name, "cycle", (1, True)).types[0], [0, n, 0, n, 0])):
        wait_eff, wait_count = block.waits()
        assert wait_count.tolist() == want and wait_eff.shape == (sum(want), 2, 2) and wait_eff.dtype == np.uint64
        assert all((w > 0) <= bool(retried) for w, (_, _, retried) in zip(want, block.regions.tolist()))
        triple, count3 = block.waits(wait_steps=3)
        assert count3.tolist() == [3 * w for w in want]
        at = 0
        for w in want:                                                           # a region's rows, three times over
            assert np.array_equal(triple[3 * at:3 * (at + w)], np.tile(wait_eff[at:at + w], (3, 1, 1)))
            at += w
        assert block.waits() is block.waits(1)                                   # cached per wait_steps
    # a wait row is the row of the same IDLE in a block type built with the IDLEs as ordinary locations, and sets no flag row
    waited = stream_noise.BlockType(code, "EC, waited", EC, emit_ec_waited())
    on_data = lambda block: (block.gates[block.locations[:, 0], 0] == GATE_IDLE) & (block.locations[:, 1] < n)   # (a measurement idles ancillas only)
    rows = waited.effects[on_data(waited)]
    assert waited.locations[on_data(waited), 1].tolist() == 2 * list(range(n))
    assert not rows[:, :, 2].any() and np.array_equal(rows[:, :, :2], ec.waits()[0]) and ec.waits()[0].any()
    trial = stream_noise.BlockType(code, "MEASURE trial, waited", MEASURE, emit_measure_waited)
    assert not trial.effects[:n, :, 2].any() and np.array_equal(trial.effects[:n, :, :2], types["MEASURE trial"].waits()[0])
    twice = stream_noise.BlockType(code, "EC, waited twice", EC, emit_ec_waited(2))
    assert np.array_equal(twice.effects[on_data(twice)][:, :, :2], ec.waits(2)[0])
    with pytest.raises(ValueError, match="wait_steps must be at least 1"):
        ec.waits(0)
    with pytest.raises(ValueError, match="wait rows, more than the 512 of one sampler segment"):
        ec.waits(512 // n + 1)
    gadget = streamed(name, "program", "X")
    assert gadget.wait_locations() == n * (gadget.preparations - 1) and gadget.wait_locations(2) == 2 * n * (gadget.preparations - 1)


# -- a sequence made by hand -------------------------------------------------------------------------------------------------------

class HandMade(object):
    """`ntypes` EC types of two regions each -- 30 retried locations that own five flag rows, then 10 that are not retried -- with
    wait_rows wait rows on the retried one; every type once, then the FINAL step.  The words' bits are those of r_1 = r_2 = 3."""

    def __init__(self, wait_rows=512, ntypes=1, seed=0):
        rng = np.random.default_rng(seed)
        keys, frame = np.uint64(retry_ref.key_mask(3, 3)), np.uint64(retry_ref.frame_mask(3, 3))
        draw = lambda shape: rng.integers(0, 1 << 64, shape, dtype=np.uint64)
        eff = np.zeros((40 * ntypes, 2, 3), dtype=np.uint64)
        eff[:, :, 0], eff[:, :, 1] = draw((40 * ntypes, 2)) & keys, draw((40 * ntypes, 2)) & frame
        for t in range(ntypes):
            eff[40 * t:40 * t + 30, :, 2] = draw((30, 2)) & draw((30, 2)) & np.uint64(31)
        self.wait_eff = np.zeros((wait_rows * ntypes, 2, 2), dtype=np.uint64)
        self.wait_eff[:, :, 0], self.wait_eff[:, :, 1] = draw((wait_rows * ntypes, 2)) & keys, draw((wait_rows * ntypes, 2)) & frame
        self.wait_count = np.array([wait_rows, 0] * ntypes, dtype=np.int64)
        self.sequence = (eff, [40] * ntypes, [5] * ntypes, list(range(ntypes)) + [-1], [EC] * ntypes + [FINAL])
        self.regions, self.nregions = np.array([(0, 30, 1), (30, 10, 0)] * ntypes, dtype=np.int64), [2] * ntypes
        self.nsteps, self.ldw, self.preparations = ntypes + 1, ntypes + 2, ntypes
        self.block_kind = self.sequence[4]

    def arguments(self, wait_eff=None, wait_count=None):
        return self.sequence + (self.regions, self.nregions, self.wait_eff if wait_eff is None else wait_eff,
                                self.wait_count if wait_count is None else wait_count)

    def words_host(self, count, p, q, seed=0, first=0, max_attempts=256, **kwargs):
        return _native.retry_wait_words_host(*self.arguments(**kwargs), seed, first, count, *p, *q, max_attempts, self.ldw + 2, self.preparations)

    def restated(self, count, p, q, seed=0, first=0, max_attempts=256):
        eff = self.sequence[0]
        types = [(eff[40 * t:40 * t + 40], self.regions[:2], 5) for t in range(self.preparations)]
        rows = len(self.wait_eff) // self.preparations
        waits = [(self.wait_eff[rows * t:rows * (t + 1)], self.wait_count[:2]) for t in range(self.preparations)]
        return retry_wait_ref.retry_wait_words(types, self.sequence[3], self.sequence[4], waits, seed, first, count, p, q, max_attempts)


# -- refusals ----------------------------------------------------------------------------------------------------------------------

def test_refusals():
    who = "gf2_retry_wait_words_host: "
    hand, p = HandMade(), rates(1e-2)
    blank = lambda rows: np.zeros((rows, 2, 2), dtype=np.uint64)
    for kwargs, text in ((dict(wait_eff=blank(513), wait_count=[513, 0]), "region 0 of block type 0 has 513 wait rows, a region holds 0 <= wait rows <= 512"),
                         (dict(wait_eff=blank(0), wait_count=[-1, 0]), "region 0 of block type 0 has -1 wait rows, a region holds 0 <= wait rows <= 512"),
                         (dict(wait_eff=blank(7), wait_count=[0, 7]), "region 1 of block type 0 is not retried but has 7 wait rows")):
        with pytest.raises(_native.GF2Error) as err:
            hand.words_host(1, p, p, **kwargs)
        assert who + text in str(err.value), str(err.value)
    words, attempts = hand.words_host(4, p, p)                                   # 512 rows pass
    assert words.shape == (4, hand.ldw + 2) and attempts.shape == (4, 1)
    for q, text in (((-1e-3, 0.0, 0.0), "the waiting probabilities must be non-negative and sum to at most 1"),
                    ((0.5, 0.5, 0.5), "the waiting probabilities must be non-negative and sum to at most 1")):
        with pytest.raises(_native.GF2Error) as err:
            hand.words_host(1, p, q)
        assert who + text in str(err.value), str(err.value)
    with pytest.raises(_native.GF2Error, match="probabilities must be non-negative and sum to at most 1"):
        hand.words_host(1, (0.5, 0.5, 0.5), rates(0.0))
    # gf2_retry_plan's rules come first, named for this entry point
    with pytest.raises(_native.GF2Error, match=who + "needs 1 <= max_attempts <= 65536, got 0"):
        hand.words_host(1, p, p, max_attempts=0)
    with pytest.raises(_native.GF2Error, match=who + r"ldw must be at least the sequence's nsteps \+ F \+ 2 = 5 words"):
        _native.retry_wait_words_host(*hand.arguments(), 0, 0, 1, *p, *p, 256, 4, 1)
    with pytest.raises(_native.GF2Error, match=who + "negative range"):
        hand.words_host(1, p, p, first=-1)
    # distinct wait sizes: a type of 17 retried one-location regions, each with a flag row and 1, 2, ..., 17 wait rows
    sizes = np.arange(1, _native.RETRY_MAX_SIZES + 2)
    eff = np.zeros((len(sizes), 2, 3), dtype=np.uint64)
    eff[:, :, 2] = (np.uint64(1) << np.arange(len(sizes), dtype=np.uint64))[:, None]
    regions = np.stack([np.arange(len(sizes)), np.ones_like(sizes), np.ones_like(sizes)], axis=1)
    many = (eff, [len(sizes)], [len(sizes)], [0, -1], [EC, FINAL], regions, [len(sizes)])
    with pytest.raises(_native.GF2Error) as err:
        _native.retry_wait_words_host(*many, blank(int(sizes.sum())), sizes, 0, 0, 1, *p, *p, 256, 5, len(sizes))
    assert who + "the regions have more than GF2_RETRY_MAX_SIZES = 16 distinct wait sizes" in str(err.value)
    sizes[-1] = 16                                                               # 16 sizes pass
    words, _ = _native.retry_wait_words_host(*many, blank(int(sizes.sum())), sizes, 0, 0, 3, *rates(0.0), *p, 256, 5, len(sizes))
    assert words.shape == (3, 5) and not words[:, :3].any() and np.all(words[:, 3] == len(sizes))
    with pytest.raises(ValueError, match="one wait count per region"):
        hand.words_host(1, p, p, wait_count=[512])
    assert _native.RETRY_WAIT_FIELDS_COUNT == 15 and _native.RETRY_WAIT_MAX_ROWS == 512


# -- the host statement against the restatement ------------------------------------------------------------------------------------

#             gadget, p_kind, q_kind, count, seed, first_sample, max_attempts, wait_steps
HOST_CASES = {"steane 2 rounds": (lambda: streamed("steane", "cycle", (2, False)), 3e-3, 3e-3, 3000, 5, 1 << 40, 256, 1),
              "rm15 1 round": (lambda: streamed("rm15", "cycle", (1, False)), 1e-3, 2e-3, 1000, 6, 0, 256, 1),
              "steane XY": (lambda: streamed("steane", "program", "XY"), 2e-3, 1e-3, 1500, 7, 3, 256, 1),
              "prepare, FINAL": (prepare_final, 3e-3, 3e-3, 3000, 8, 11, 256, 1),
              "steane 2 rounds, 3 attempts": (lambda: streamed("steane", "cycle", (2, False)), 3e-3, 3e-3, 3000, 9, 0, 3, 1),
              "steane 2 rounds, 2 wait steps": (lambda: streamed("steane", "cycle", (2, False)), 3e-3, 3e-3, 3000, 10, 0, 256, 2)}


@pytest.mark.parametrize("case", sorted(HOST_CASES))
def test_host_statement_equals_the_restatement(case):
    make, p_kind, q_kind, count, seed, first, max_attempts, wait_steps = HOST_CASES[case]
    gadget, p, q = make(), rates(p_kind), rates(q_kind)
    words, attempts = gadget.retry_wait_words_host(count, *p, *q, seed=seed, first_sample=first, wait_steps=wait_steps, max_attempts=max_attempts)
    want_words, want_attempts = retry_wait_ref.retry_wait_words(*retry_wait_ref.tables_of(gadget, wait_steps), seed, first, count, p, q, max_attempts)
    assert words.shape == (count, gadget.ldw + 2) and attempts.shape == (count, gadget.preparations)
    assert np.array_equal(words, want_words) and np.array_equal(attempts, want_attempts)
    assert np.array_equal(words[:, -2], attempts.sum(axis=1, dtype=np.uint64))
    exhausted = words[:, gadget.nsteps:gadget.ldw].any(axis=1)
    assert exhausted.any() == (max_attempts == 3)
    faults = int(words[:, -1].sum(dtype=np.uint64))
    if case == "prepare, FINAL":
        assert faults == 0 and gadget.wait_locations() == 0                      # the data block is what is being prepared
    else:                                                                        # not vacuous: wait faults in a fifth of the samples at least
        assert (words[:, -1] > 0).sum() * 5 >= count and (words[exhausted, -1] > 0).any() == exhausted.any()
        plain, _ = gadget.retry_words_host(count, *p, seed=seed, first_sample=first, max_attempts=max_attempts)
        assert (words[:, :gadget.nsteps] != plain[:, :gadget.nsteps]).any(axis=1).sum() * 10 >= count   # ... and they reach the step words


def test_floyds_rule_on_a_region_of_512_wait_rows():
    hand, p, q = HandMade(), rates(1e-2), rates(1e-2)
    words, attempts = hand.words_host(1500, p, q, seed=11, first=5)
    want_words, want_attempts = hand.restated(1500, p, q, seed=11, first=5)
    assert np.array_equal(words, want_words) and np.array_equal(attempts, want_attempts)
    assert words[:, -1].sum() > 1500 * 512 * 0.03 and (attempts > 1).mean() > 0.25   # K = 15 per attempt on average, retries in a quarter at least
    several = HandMade(wait_rows=100, ntypes=3, seed=1)
    words, attempts = several.words_host(500, p, q, seed=12)
    want_words, want_attempts = several.restated(500, p, q, seed=12)
    assert np.array_equal(words, want_words) and np.array_equal(attempts, want_attempts)


def test_wider_pitch_and_no_attempts_array():
    gadget = streamed("steane", "cycle", (2, False))
    words, _ = gadget.retry_wait_words_host(50, *rates(3e-3), *rates(3e-3), seed=1)
    wide = np.full((50, gadget.ldw + 4), 0xABCD, dtype="<u8")
    seq = _native._stream_sequence(*gadget._sequence())[1]
    regions = _native._retry_regions(gadget.type_regions, gadget.type_nregions, 1)[1]
    keep, waits = _native._retry_waits(*gadget._retry_wait_sequence()[-2:], 4)
    _native.check(_native.lib().gf2_retry_wait_words_host(*seq, *regions, *waits, 1, 0, 50, 3e-3, 3e-3, 3e-3, 3e-3, 3e-3, 3e-3, 256, wide.ctypes.data,
                                                          gadget.ldw + 4, None))
    assert np.array_equal(wide[:, :gadget.ldw + 2], words) and np.all(wide[:, gadget.ldw + 2:] == 0xABCD)
    assert gadget.retry_wait_words_host(0, *rates(3e-3), *rates(3e-3))[0].shape == (0, gadget.ldw + 2)


# -- consequences 1 and 2 ----------------------------------------------------------------------------------------------------------

COUNT = 4096


@pytest.mark.parametrize("make", [lambda: streamed("steane", "cycle", (2, False)), lambda: streamed("steane", "program", "XY"), prepare_final],
                         ids=["cycle", "program", "prepare"])
def test_consequence_1_no_waiting_faults_is_the_plain_retried_route(make):
    gadget, p = make(), rates(3e-3)
    for q, steps, limit in ((rates(0.0), 1, 256), (rates(0.0), 2, 3)) + (((rates(1e-2), 1, 256),) if gadget.wait_locations() == 0 else ()):
        plain, plain_attempts = gadget.retry_words_host(COUNT, *p, seed=3, first_sample=7, max_attempts=limit)
        words, attempts = gadget.retry_wait_words_host(COUNT, *p, *q, seed=3, first_sample=7, wait_steps=steps, max_attempts=limit)
        assert np.array_equal(words[:, :-1], plain) and not words[:, -1].any() and np.array_equal(attempts, plain_attempts)
        assert np.array_equal(gadget.tally_host(words[:, :gadget.ldw], fields=True), gadget.tally_host(plain[:, :gadget.ldw], fields=True))


@pytest.mark.parametrize("limit", [256, 3])
def test_consequence_2_the_attempts_are_those_of_the_plain_retried_route(limit):
    gadget, p = streamed("steane", "cycle", (2, False)), rates(3e-3)
    plain, plain_attempts = gadget.retry_words_host(COUNT, *p, seed=4, max_attempts=limit)
    for q in (rates(3e-3), (0.02, 0.0, 0.01)):
        words, attempts = gadget.retry_wait_words_host(COUNT, *p, *q, seed=4, max_attempts=limit)
        assert np.array_equal(words[:, -2], plain[:, -1]) and np.array_equal(attempts, plain_attempts)
        flags, plain_flags = words[:, gadget.nsteps:gadget.ldw], plain[:, gadget.nsteps:gadget.ldw]
        assert np.array_equal(flags, plain_flags) and flags.any(axis=1).any() == (limit == 3)
        assert (words[:, :gadget.nsteps] != plain[:, :gadget.nsteps]).any()      # ... while the step words do differ


# -- exact distributions -----------------------------------------------------------------------------------------------------------

SAMPLES = 200000
ONE_ROUND_P = ONE_ROUND_Q = 5e-4   # of the 14-bit joint: the cells that expect fewer than 10 of 2 x 10^5 samples hold 0.67 % of the mass there (exact, no sampling)
WAIT_Z_P = WAIT_Z_Q = 3e-3         # the preparations pass with 0.39 and 0.44: 2.4 attempts per preparation


def test_wait_faults_follow_their_exact_mean_and_variance():
    gadget, p, q = streamed("steane", "cycle", (1, False)), rates(WAIT_Z_P), rates(WAIT_Z_Q)
    block = gadget.types[0]
    passes = [retry_ref.region_pass_probability(block, r, p) for r, row in enumerate(block.regions.tolist()) if row[2]]
    assert all(1.0 - s > 0.25 for s in passes)                                   # more than a quarter of the preparations take a second attempt
    mean, var, once, _ = retry_wait_ref.wait_faults_mean_var(gadget, p, q)
    assert abs(mean - once) * SAMPLES > 5.0 * (SAMPLES * var) ** 0.5             # waits on every attempt are told from waits on the accepted one
    words, _ = gadget.retry_wait_words_host(SAMPLES, *p, *q, seed=24)
    assert not words[:, gadget.nsteps:gadget.ldw].any()                         # (truncation at 256 attempts: below 1e-50)
    exact_dist.assert_z("wait faults of one Steane round at p = q = %g, mean %.4f per sample (%.4f if only the accepted attempt waited)"
                        % (WAIT_Z_P, mean, once), int(words[:, -1].sum(dtype=np.uint64)), SAMPLES * mean, SAMPLES * var)


def test_one_round_follows_the_convolution_with_the_wait_noise():
    gadget, p, q = streamed("steane", "cycle", (1, False)), rates(ONE_ROUND_P), rates(ONE_ROUND_Q)
    words, _ = gadget.retry_wait_words_host(SAMPLES, *p, *q, seed=25)
    assert not words[:, 2].any()
    exact = retry_wait_ref.one_round_distribution(gadget, p, q, 3, 3)
    assert exact.shape == (1 << 14,)
    plain = retry_ref.one_round_distribution(gadget, p, 3, 3)
    assert np.abs(exact - plain).sum() > 0.01                                    # the wait noise moves a percent of the mass
    exact_dist.assert_chi2("(round word, T) of one Steane round with waiting faults", np.bincount(retry_ref.one_round_cells(words, 3, 3), minlength=1 << 14),
                           exact, SAMPLES)
