"""
The repeat-until-success sampler of multi-block programs (DESIGN.md section 5d "Repeat-until-success of multi-block programs")
without a GPU.

  restatement     gf2_mretry_words_host equals tests/multi_retry_ref.py, words and attempts per preparation, bit for bit
  identity        for every sample that is not exhausted, the words are those of the post-selected route on the faults of the attempts
                  that entered the blocks: MultiProgram.words_of_faults and the full-frame model multi_stream_ref.Rewritten
  Q = 1           words and attempts equal StreamedGadget.retry_words_host's bit for bit
  no faults       p = 0
  tally           gf2_mstream_tally_host completes the statement; every exhausted sample is rejected there
  refusals        by message
  exact laws      the attempts follow the geometric law; with two attempts the samples that are not exhausted follow the product of
                  the preparations' 1 - (1 - q)^2
"""
import numpy as np
import pytest

from oracle import exact_dist
from quantum_css_codes_amd import _native, stream_noise
from tests import multi_retry_ref, retry_ref, stream_ref
from tests.test_ft import oracle_code
from tests.test_multi_stream import CNOT_MEASURE, THREE, X_CNOT_TWO, multi

RATES = (1e-3, 5e-4, 1e-3)


def host_counts(program, words, records='reference'):
    """The twenty-two counts of the host statement: tally_host on the first nsteps + F words, the exhausted samples (a non-zero flag
    word), the attempts."""
    words = np.asarray(words, dtype=np.uint64)
    tally = program.tally_host(words[:, :program.ldw], records=records, fields=True)
    exhausted = int(words[:, program.nsteps:program.ldw].any(axis=1).sum())
    return [int(v) for v in tally] + [exhausted, int(words[:, program.ldw].sum())]


@pytest.mark.parametrize("name, instructions, first, count, max_attempts",
                         [("steane", X_CNOT_TWO, 0, 2500, 256), ("steane", THREE, 1 << 40, 2000, 3), ("steane", X_CNOT_TWO, 77, 1500, 1),
                          ("rm15", CNOT_MEASURE, 5, 1000, 256), ("rm15", CNOT_MEASURE, 5, 1000, 3), ("steane", THREE, 9, 2000, 256)])
def test_host_statement_equals_the_restatement_and_the_post_selected_route(name, instructions, first, count, max_attempts):
    got, ref = multi(name, instructions)
    words, attempts = got.retry_words_host(count, *RATES, seed=11, first_sample=first, max_attempts=max_attempts)
    want_words, want_attempts, faults = multi_retry_ref.retry_words(got, 11, first, count, RATES, max_attempts)
    assert words.shape == want_words.shape == (count, got.ldw + 1) and attempts.shape == (count, got.preparations)
    assert np.array_equal(words, want_words) and np.array_equal(attempts, want_attempts)
    assert np.array_equal(words[:, -1], attempts.sum(axis=1, dtype=np.uint64))
    alive = ~words[:, got.nsteps:got.ldw].any(axis=1)
    if max_attempts == 256:
        assert alive.all() and int(attempts.max()) > 2 and int(attempts.min()) == 1
    elif max_attempts == 3:
        assert 0 < int(alive.sum()) < count and int(attempts.max()) == 3
        assert (attempts[~alive] == 0).any() and not (attempts[alive] == 0).any()      # a preparation never reached
        assert not words[~alive][:, got.nsteps - 1].any()                               # ... and the later step words stay 0
    # the identity with the post-selected route, through the block tables and through the full-frame model
    assert int(alive.sum()) > 0 or max_attempts == 1
    assert np.array_equal(got.words_of_faults(*faults)[alive], words[alive, :got.ldw])
    full = ref.outcome_words(*stream_ref.dense_faults(got.num_locations, *faults))
    assert np.array_equal(full[alive], words[alive, :got.ldw])
    assert np.count_nonzero(words[alive, :got.nsteps]) > 0 or max_attempts == 1


@pytest.mark.parametrize("name, ops", [("steane", ""), ("steane", "XYZ"), ("rm15", "X")])
@pytest.mark.parametrize("max_attempts", [256, 2])
def test_one_qubit_programs_equal_the_retried_route(name, ops, max_attempts):
    code = oracle_code(name)
    one = stream_noise.StreamedGadget.program(code, ops)
    got = stream_noise.MultiProgram(code, [(op, 3) for op in ops] + [('MEASURE', 3)])
    assert got.preparations == one.preparations and got.ldw == one.ldw
    words, attempts = got.retry_words_host(1500, *RATES, seed=5, first_sample=1 << 33, max_attempts=max_attempts)
    want_words, want_attempts = one.retry_words_host(1500, *RATES, seed=5, first_sample=1 << 33, max_attempts=max_attempts)
    assert np.array_equal(words, want_words) and np.array_equal(attempts, want_attempts)
    assert np.count_nonzero(words[:, :got.nsteps]) > 0 and int(attempts.max()) > 1


def test_no_faults():
    got, _ = multi("steane", THREE)
    words, attempts = got.retry_words_host(300, 0.0, 0.0, 0.0, seed=1, max_attempts=7)
    assert not words[:, :got.ldw].any() and (words[:, got.ldw] == got.preparations).all() and (attempts == 1).all()
    for records in ('reference', 'propagated'):
        assert host_counts(got, words, records) == [300] + [0] * 20 + [300 * got.preparations]
    assert got.preparations == int(sum(got.types[t].regions[:, 2].sum() for t in got.block_type)) > 20
    cnot = next(t for t in got.types if t.kind == stream_noise.CNOT)
    assert cnot.regions.tolist() == [[0, 14, 0]]


@pytest.mark.parametrize("name, instructions", [("steane", X_CNOT_TWO), ("rm15", CNOT_MEASURE)])
def test_tally_completes_the_statement(name, instructions):
    got, ref = multi(name, instructions)
    words, _ = got.retry_words_host(3000, *RATES, seed=2, max_attempts=3)
    exhausted = words[:, got.nsteps:got.ldw].any(axis=1)
    assert 100 < int(exhausted.sum()) < 2900
    for records in ('reference', 'propagated'):
        counts, classes = got.tally_host(words[:, :got.ldw], records=records, fields=True, classes=True)
        assert np.array_equal((classes & 1).astype(bool), ~exhausted)
        assert counts.tolist() == ref.tally(words[:, :got.ldw], records)
        assert host_counts(got, words, records) == counts.tolist() + [int(exhausted.sum()), int(words[:, -1].sum())]
        assert int(counts[0]) + int(exhausted.sum()) == 3000 and int(counts[5]) > 0


def test_refusals():
    got, _ = multi("steane", CNOT_MEASURE)
    eff, locs, flags, types, kinds, frame_a, frame_b, frames, regions, counts = got._retry_sequence()
    cnot_type = next(t for t, kind in enumerate(got.types) if kind.kind == stream_noise.CNOT)
    cnot_block = int(np.flatnonzero(kinds == stream_noise.CNOT)[0])
    cnot_region = int(counts[:cnot_type].sum())
    retried = int(np.flatnonzero(regions[:, 2] == 1)[0])
    retried_type = int(np.searchsorted(np.cumsum(counts), retried, side="right"))

    def changed(array, at, value):
        out = array.copy()
        out[at] = value
        return out

    split = np.insert(changed(regions, (cnot_region, 1), 4), cnot_region + 1, [4, 10, 0], axis=0)
    cases = ((dict(regions=changed(regions, (cnot_region, 2), 1)),
              "gf2_mretry_words_host: the type of CNOT block %d has 1 regions, the first retried 1: a CNOT block has no flag rows" % cnot_block),
             (dict(regions=split, counts=changed(counts, cnot_type, 2)), "the type of CNOT block %d has 2 regions, the first retried 0" % cnot_block),
             (dict(regions=changed(regions, (retried, 1), regions[retried, 1] + 1)),
              "gf2_mretry_words_host: the regions of block type %d do not partition its %d locations in order" % (retried_type, locs[retried_type])),
             (dict(regions=np.delete(regions, cnot_region, axis=0), counts=changed(counts, cnot_type, 0)),
              "the regions of block type %d do not partition its 14 locations in order: it has 0 regions" % cnot_type),
             (dict(regions=changed(regions, (retried, 2), 0)), "of block type %d .* is not retried but its locations set a flag bit" % retried_type),
             (dict(regions=changed(regions, (retried, 2), 2)), "retried 2"),
             (dict(max_attempts=0), "gf2_mretry_words_host: needs 1 <= max_attempts <= 65536, got 0"),
             (dict(max_attempts=65537), "needs 1 <= max_attempts <= 65536, got 65537"),
             (dict(ldw=got.ldw), r"gf2_mretry_words_host: ldw must be at least the sequence's nsteps \+ F \+ 1 = %d words" % (got.ldw + 1)),
             (dict(frames=5), "gf2_mretry_words_host: needs 1 <= nframes <= 4 data frames"),
             (dict(kinds=changed(kinds, 3, 3)), "gf2_mretry_words_host: block 3 is a FINAL step, this route has none"),
             (dict(b=changed(frame_b, cnot_block, 0)), "CNOT block %d has frame 0 as control and as target" % cnot_block),
             (dict(first=-1), "gf2_mretry_words_host: negative range"), (dict(count=-1), "negative range"),
             (dict(p=(0.5, 0.4, 0.2)), "probabilities must be non-negative and sum to at most 1"),
             (dict(p=(-0.1, 0.0, 0.0)), "probabilities must be non-negative"))
    for change, text in cases:
        args = dict(eff=eff, locs=locs, flags=flags, types=types, kinds=kinds, a=frame_a, b=frame_b, frames=frames, regions=regions, counts=counts,
                    first=0, count=2, p=RATES, max_attempts=256, ldw=got.ldw + 1)
        args.update(change)
        with pytest.raises(_native.GF2Error, match=text):
            _native.mretry_words_host(args['eff'], args['locs'], args['flags'], args['types'], args['kinds'], args['a'], args['b'], args['frames'],
                                      args['regions'], args['counts'], 3, args['first'], args['count'], *args['p'], args['max_attempts'], args['ldw'],
                                      got.preparations)
    assert got.retry_words_host(0, *RATES)[0].shape == (0, got.ldw + 1)
    assert got.retry_words_host(2, *RATES, max_attempts=65536)[0].shape == (2, got.ldw + 1)
    with pytest.raises(ValueError, match="'reference' or 'propagated'"):
        got.retry_counts(1, *RATES, records=2)
    with pytest.raises(_native.GF2Error, match=r"records must be GF2_MSTREAM_REFERENCE \(0\) or GF2_MSTREAM_PROPAGATED \(1\), got 2"):
        _native.mstream_tally_host(np.zeros((1, got.ldw), dtype=np.uint64), kinds, frame_a, frame_b, frames, got.flag_words, 2, *got._tables())
    # the shared rules keep their text under the one-qubit route's name
    one = stream_noise.StreamedGadget.program(oracle_code("steane"), "")
    seq = one._retry_sequence()
    with pytest.raises(_native.GF2Error, match="gf2_retry_words_host: the regions of block type 0 do not partition its %d locations in order: they end at"
                                               % one.type_locations[0]):
        _native.retry_words_host(*seq[:5], changed(seq[5], (int(seq[6][0]) - 1, 1), seq[5][int(seq[6][0]) - 1, 1] - 1), seq[6], 0, 0, 1, *RATES, 256,
                                 one.ldw + 1, one.preparations)


def test_exact_laws():
    got, _ = multi("steane", X_CNOT_TWO)
    count = 200000
    words, attempts = got.retry_words_host(count, *RATES, seed=21)
    mean, var = retry_ref.attempts_mean_var(got, RATES)
    assert not words[:, got.nsteps:got.ldw].any() and 1.2 * got.preparations < mean < 1.35 * got.preparations
    exact_dist.assert_z("multi retry: attempts of X_CNOT_TWO", int(words[:, -1].sum()), count * mean, count * var)
    keep = 1.0
    for t in got.block_type:
        for r, (_, _, retried) in enumerate(got.types[t].regions.tolist()):
            if retried:
                keep *= 1.0 - (1.0 - retry_ref.region_pass_probability(got.types[t], r, RATES)) ** 2
    assert abs(keep - 0.177) < 0.0015
    words, attempts = got.retry_words_host(count, *RATES, seed=22, max_attempts=2)
    alive = int((~words[:, got.nsteps:got.ldw].any(axis=1)).sum())
    exact_dist.assert_z("multi retry: not exhausted with two attempts", alive, count * keep, count * keep * (1.0 - keep))
