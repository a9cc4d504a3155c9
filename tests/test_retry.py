"""
The repeat-until-success sampler of the streamed gadgets (DESIGN.md section 5d "Repeat-until-success") without a GPU: the regions of
the block types, the refusals of the shared argument check, gf2_retry_words_host against the NumPy restatement tests/retry_ref.py
bit for bit, and the host statement's samples against exact distributions (oracle/exact_dist.py, its thresholds as they are).
"""
import numpy as np
import pytest

from oracle import exact_dist
from quantum_css_codes_amd import _native, stream_noise
from tests import retry_ref
from tests.test_stream import oracle_code, streamed

EC_RANGES = {"steane": [(0, 148, 1), (148, 21, 0), (169, 133, 1), (302, 28, 0)],
             "rm15": [(0, 369, 1), (369, 45, 0), (414, 330, 1), (744, 60, 0)]}


def rates(p_kind):
    return (p_kind, p_kind, p_kind)


# -- regions -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,what,key", [("steane", "cycle", (1, False)), ("steane", "cycle", (1, True)), ("rm15", "cycle", (1, False)),
                                           ("rm15", "cycle", (1, True)), ("steane", "program", "XYZ"), ("rm15", "program", "XYZ")])
def test_regions_partition_the_locations_and_own_their_flags(name, what, key):
    gadget = streamed(name, what, key)
    rows = 7 if name == "steane" else 15
    for block in gadget.types:
        regions = block.regions.tolist()
        assert np.all(np.diff(block.locations[:, 0]) >= 0)                     # locations are in gate order
        at = 0
        for first, count, retried in regions:                                  # a partition, in order
            assert first == at and count >= 1 and retried in (0, 1)
            at += count
        assert at == block.num_locations
        masks = [int(m) for m in block.region_masks()]
        seen = 0
        for (first, count, retried), mask in zip(regions, masks):
            assert (mask == 0) if not retried else bin(mask).count("1") == rows  # no flag bit outside a preparation; 7 / 15 rows each
            if retried:
                low = (mask & -mask).bit_length() - 1
                assert mask == ((1 << rows) - 1) << low                        # contiguous rows
            assert not seen & mask
            seen |= mask
        assert seen == (1 << block.num_flags) - 1
        assert not any(a[2] == 0 and b[2] == 0 for a, b in zip(regions, regions[1:]))   # the regions between preparations are maximal
    assert np.array_equal(gadget.type_regions, np.concatenate([t.regions for t in gadget.types]))
    assert gadget.type_nregions.tolist() == [len(t.regions) for t in gadget.types]
    assert gadget.preparations == sum(int(gadget.types[t].regions[:, 2].sum()) for t in gadget.block_type if t >= 0)


def test_the_quoted_ranges():
    for name, want in EC_RANGES.items():
        assert streamed(name, "cycle", (1, False)).types[0].regions.tolist() == [list(r) for r in want]
        shift = 7 if name == "steane" else 15                                   # idle_data: one region of idle locations in front
        idle = streamed(name, "cycle", (1, True)).types[0].regions.tolist()
        assert idle == [[0, shift, 0]] + [[first + shift, count, retried] for first, count, retried in want]
    program = streamed("steane", "program", "XZ")
    assert {t.name: t.regions.tolist() for t in program.types}["prepare data"] == [[0, 133, 1]]
    assert {t.name: t.regions.tolist() for t in program.types}["MEASURE trial"] == [[0, 133, 1], [133, 21, 0]]
    assert streamed("steane", "cycle", (5, False)).preparations == 10 and program.preparations == 1 + 2 * 2 + 3 * 3


# -- refusals ------------------------------------------------------------------------------------------------------------------

def host_words(gadget, regions=None, nregions=None, max_attempts=256, count=1, p=rates(1e-3), ldw=None, first=0, sequence=None):
    sequence = gadget._sequence() if sequence is None else sequence
    return _native.retry_words_host(*sequence, gadget.type_regions if regions is None else regions,
                                    gadget.type_nregions if nregions is None else nregions, 0, first, count, *p, max_attempts,
                                    gadget.ldw + 1 if ldw is None else ldw, gadget.preparations)


def test_refusals():
    gadget = streamed("steane", "cycle", (2, False))
    who = "gf2_retry_words_host: "
    for regions, nregions, text in (([(0, 148, 1), (148, 21, 0), (170, 132, 1), (302, 28, 0)], [4], "do not partition its 330 locations in order: region 2"),
                                    ([(0, 148, 1), (148, 21, 0), (169, 133, 1)], [3], "do not partition its 330 locations in order: they end at location 302"),
                                    ([(0, 148, 1), (148, 21, 0), (169, 133, 1), (302, 29, 0)], [4], "do not partition"),
                                    ([(0, 148, 1), (148, 21, 0), (169, 133, 2), (302, 28, 0)], [4], "do not partition"),
                                    ([(0, 148, 1), (148, 21, 0), (169, 133, 0), (302, 28, 0)], [4], "region 2 of block type 0 (locations 169 .. 301) is not retried but its locations set a flag bit"),
                                    ([(0, 100, 1), (100, 69, 1), (169, 133, 1), (302, 28, 0)], [4], "the flag masks of regions 0 and 1 of block type 0 intersect")):
        with pytest.raises(_native.GF2Error) as err:
            host_words(gadget, np.array(regions), np.array(nregions))
        assert who in str(err.value) and text in str(err.value), str(err.value)
    for bad in (0, -1, 65537):
        with pytest.raises(_native.GF2Error) as err:
            host_words(gadget, max_attempts=bad)
        assert who + "needs 1 <= max_attempts <= 65536, got %d" % bad in str(err.value)
    assert _native.RETRY_MAX_ATTEMPTS == 65536 and len(host_words(gadget, max_attempts=65536)[0]) == 1
    # distinct segment sizes: a type of flag-free locations cut into regions of 1, 2, ..., 17 locations has one size too many
    sizes = np.arange(1, _native.RETRY_MAX_SIZES + 2)
    regions = np.stack([np.cumsum(sizes) - sizes, sizes, np.zeros_like(sizes)], axis=1)
    blank = (np.zeros((int(sizes.sum()), 2, 3), dtype=np.uint64), [int(sizes.sum())], [0], [0, -1], [stream_noise.EC, stream_noise.FINAL])
    with pytest.raises(_native.GF2Error) as err:
        _native.retry_words_host(*blank, regions, [len(sizes)], 0, 0, 1, *rates(1e-3), 256, 4, 0)
    assert who + "the regions have more than GF2_RETRY_MAX_SIZES = 16 distinct segment sizes" in str(err.value)
    words, _ = _native.retry_words_host(*blank, np.concatenate([regions[:-2], [[int(regions[-2, 0]), 33, 0]]]), [len(sizes) - 1], 0, 0, 3, *rates(1e-3), 256, 4, 0)
    assert words.shape == (3, 4) and not words.any()                     # 16 sizes pass: no flags, no retried region, no attempt
    # the sequence rules of gf2_stream_words_host, the range, the rates and the pitch
    eff, locs, flags, types, kinds = gadget._sequence()
    for sequence, text in (((eff, locs, flags, [0, -1, 0], [1, 3, 1]), "must be the last step"), ((eff, locs, flags, [0, 0, 0], [1, 1, 1]), "0 MEASURE steps"),
                           ((eff, locs, [13], types, kinds), "at or above its 13 flag rows"), ((eff, locs, [65], types, kinds), "at most 64")):
        with pytest.raises(_native.GF2Error) as err:
            host_words(gadget, sequence=sequence)
        assert who in str(err.value) and text in str(err.value), str(err.value)
    with pytest.raises(_native.GF2Error, match="negative range"):
        host_words(gadget, first=-1)
    with pytest.raises(_native.GF2Error, match="non-negative and sum to at most 1"):
        host_words(gadget, p=(0.5, 0.5, 0.5))
    with pytest.raises(_native.GF2Error, match=r"ldw must be at least the sequence's nsteps \+ F \+ 1 = 5 words"):
        host_words(gadget, ldw=4)


# -- the host statement against the restatement ----------------------------------------------------------------------------------

def prepare_final(name="steane"):
    code = oracle_code(name)
    block = stream_noise.BlockType(code, "prepare data", stream_noise.NONE, stream_noise._emit_prepare)
    return stream_noise.StreamedGadget(code, "cycle", [block], [0, -1], [stream_noise.NONE, stream_noise.FINAL])


HOST_CASES = {"steane 2 rounds": (lambda: streamed("steane", "cycle", (2, False)), 3e-3, 3000, 5, 1 << 40, 256),
              "rm15 1 round": (lambda: streamed("rm15", "cycle", (1, False)), 1e-3, 1000, 6, 0, 256),
              "steane XY": (lambda: streamed("steane", "program", "XY"), 2e-3, 1500, 7, 3, 256),
              "prepare, FINAL": (prepare_final, 3e-3, 3000, 8, 11, 256),
              "steane 2 rounds, 3 attempts": (lambda: streamed("steane", "cycle", (2, False)), 3e-3, 3000, 9, 0, 3)}


@pytest.mark.parametrize("case", sorted(HOST_CASES))
def test_host_statement_equals_the_restatement(case):
    make, p_kind, count, seed, first, max_attempts = HOST_CASES[case]
    gadget = make()
    words, attempts = gadget.retry_words_host(count, *rates(p_kind), seed=seed, first_sample=first, max_attempts=max_attempts)
    want_words, want_attempts = retry_ref.retry_words(gadget, seed, first, count, rates(p_kind), max_attempts)
    assert words.shape == (count, gadget.ldw + 1) and attempts.shape == (count, gadget.preparations)
    assert np.array_equal(words, want_words) and np.array_equal(attempts, want_attempts)
    assert (attempts > 1).any(axis=1).sum() * 3 >= count                        # not vacuous: a third of the samples took a retry
    assert np.array_equal(words[:, -1], attempts.sum(axis=1, dtype=np.uint64))
    exhausted = words[:, gadget.nsteps:gadget.ldw].any(axis=1)
    assert exhausted.any() == (max_attempts == 3)
    reached = np.cumsum(attempts == 0, axis=1) == 0                             # a preparation never reached has 0 attempts, and so have all after it
    assert np.array_equal(attempts != 0, reached) and np.all(attempts[~exhausted] != 0)
    last = attempts[exhausted, np.maximum(reached[exhausted].sum(axis=1) - 1, 0)]   # an exhausted sample's last preparation used every attempt
    assert np.all(last == max_attempts)


def test_wider_pitch_and_no_attempts_array():
    gadget = streamed("steane", "cycle", (2, False))
    words, _ = gadget.retry_words_host(50, *rates(3e-3), seed=1)
    wide = np.full((50, gadget.ldw + 3), 0xABCD, dtype="<u8")
    seq = _native._stream_sequence(*gadget._sequence())[1]
    regions = _native._retry_regions(gadget.type_regions, gadget.type_nregions, 1)[1]
    _native.check(_native.lib().gf2_retry_words_host(*seq, *regions, 1, 0, 50, 3e-3, 3e-3, 3e-3, 256, wide.ctypes.data, gadget.ldw + 3, None))
    assert np.array_equal(wide[:, :gadget.ldw + 1], words) and np.all(wide[:, gadget.ldw + 1:] == 0xABCD)
    assert gadget.retry_words_host(0, *rates(3e-3))[0].shape == (0, gadget.ldw + 1)


def test_no_noise():
    for gadget in (streamed("steane", "cycle", (3, False)), streamed("steane", "program", "XY"), prepare_final()):
        words, attempts = gadget.retry_words_host(64, 0.0, 0.0, 0.0, seed=3)
        assert not words[:, :-1].any() and np.all(words[:, -1] == gadget.preparations) and np.all(attempts == 1)


def test_accepted_flags_are_zero_and_two_attempts_exhaust():
    gadget = streamed("steane", "cycle", (1, False))
    count = 5000
    words, attempts = gadget.retry_words_host(count, *rates(3e-3), seed=2, max_attempts=2)
    flagged = words[:, gadget.nsteps:gadget.ldw].any(axis=1)
    exhausted = int(flagged.sum())                                              # exact fraction 1 - (1 - 0.608^2)(1 - 0.558^2) = 0.57
    assert exhausted > count // 5 and count - exhausted > count // 5
    assert np.all(attempts[~flagged] != 0) and np.all((attempts[flagged] == 2).any(axis=1))
    assert not words[flagged][:, :gadget.nsteps].any()                          # one block: exhausted in it, no step word
    tally = gadget.tally_host(words[:, :gadget.ldw], fields=True)
    assert int(tally[0]) == count - exhausted
    words, _ = gadget.retry_words_host(count, *rates(3e-3), seed=2)
    assert not words[:, gadget.nsteps:gadget.ldw].any()                         # 256 attempts: every sample accepted, its flag words zero


# -- exact distributions -------------------------------------------------------------------------------------------------------

SAMPLES = 200000
ONE_ROUND_P = 5e-4              # of the 14-bit joint: the cells that expect fewer than 10 of 2 x 10^5 samples hold 3 % of the mass at 3e-3, 1.07 % at 1e-3


@pytest.mark.parametrize("p_kind", [1e-3, 3e-3])
def test_attempts_follow_the_geometric_law(p_kind):
    gadget = streamed("steane", "cycle", (1, False))
    words, attempts = gadget.retry_words_host(SAMPLES, *rates(p_kind), seed=21)
    assert not words[:, gadget.nsteps:gadget.ldw].any()                         # (truncation at 256 attempts: below 1e-50)
    preps = [r for r, row in enumerate(gadget.types[0].regions.tolist()) if row[2]]
    for k, r in enumerate(preps):
        q = retry_ref.region_pass_probability(gadget.types[0], r, rates(p_kind))
        exact_dist.assert_z("attempts of preparation %d at p = %g, 1/q = %.4f" % (k, p_kind, 1.0 / q), int(attempts[:, k].sum(dtype=np.int64)),
                            SAMPLES / q, SAMPLES * (1.0 - q) / (q * q))
    mean, var = retry_ref.attempts_mean_var(gadget, rates(p_kind))
    exact_dist.assert_z("attempts of a sample at p = %g" % p_kind, int(words[:, -1].sum(dtype=np.uint64)), SAMPLES * mean, SAMPLES * var)


def test_prepared_frame_follows_the_conditional_distribution():
    gadget, p = prepare_final(), rates(3e-3)
    words, _ = gadget.retry_words_host(SAMPLES, *p, seed=22)
    assert not words[:, 1].any()
    exact = retry_ref.prepare_final_distribution(gadget, p, 3, 3)
    assert exact.shape == (256,)
    exact_dist.assert_chi2("T of [prepare, FINAL] given flags = 0", np.bincount(retry_ref.prepare_final_cells(words, 3, 3), minlength=256), exact, SAMPLES)


def test_one_round_follows_the_convolution_of_the_regions():
    gadget, p = streamed("steane", "cycle", (1, False)), rates(ONE_ROUND_P)
    words, _ = gadget.retry_words_host(SAMPLES, *p, seed=23)
    assert not words[:, 2].any()
    exact = retry_ref.one_round_distribution(gadget, p, 3, 3)
    assert exact.shape == (1 << 14,)
    exact_dist.assert_chi2("(round word, T) of one Steane round", np.bincount(retry_ref.one_round_cells(words, 3, 3), minlength=1 << 14), exact, SAMPLES)
