"""
The repeat-until-success sampler of multi-block programs under gate-level faults (DESIGN.md section 5d "Repeat-until-success of
multi-block programs under gate-level faults") without a GPU.

  sites           CnotBlockType.gate_regions; every type's sites partition its regions
  restatement     gf2_mretry_gate_words_host equals tests/multi_retry_gate_ref.py, words and attempts per preparation, bit for bit
  full frames     for every sample that is not exhausted, the words are those of the location faults of the attempts that entered the
                  blocks (a CNOT event expanded into its one or two location faults): MultiProgram.words_of_faults and the
                  full-frame model multi_stream_ref.Rewritten, which has no tables and no frame map
  CNOT events     every site x kappa of a CNOT block shows on the frames kappa names
  Q = 1           words and attempts equal StreamedGadget.retry_gate_words_host's bit for bit
  trivial cases   p = 0, either class alone, the tally, other samples than the location route, refusals by message
  exact laws      the key bits of the two rounds after a CNOT against the exact law of the correlated event; the attempts against the
                  geometric law; with two attempts the samples that are not exhausted
  bare program    ft_noise.raw_circuit_gate_error_rate against an enumeration of the bare circuit
"""
import itertools

import numpy as np
import pytest

from oracle import exact_dist
from quantum_css_codes_amd import _native, ft_noise, stream_noise
from tests import multi_retry_gate_ref, retry_gate_ref, stream_ref
from tests.retry_ref import key_mask
from tests.test_ft import oracle_code
from tests.test_multi_stream import CNOT_MEASURE, THREE, X_CNOT_TWO, multi

# Rates picked on the host for what the cases assert.  A Steane preparation has about 100 sites: at (2e-3, 3e-3) it passes with
# probability near 0.8, so 256 attempts accept every sample and some preparation takes more than two; the 35 to 60 preparations of a
# program then leave both accepted and exhausted samples at 3 attempts.  The 21 preparations of the Reed-Muller program need (1.2e-3,
# 1.8e-3) for the same.
RATES = {"steane": (2e-3, 3e-3), "rm15": (1.2e-3, 1.8e-3)}


def host_counts(program, words, records='reference'):
    """The twenty-two counts of the host statement: tally_host on the first nsteps + F words, the exhausted samples (a non-zero flag
    word), the attempts."""
    words = np.asarray(words, dtype=np.uint64)
    tally = program.tally_host(words[:, :program.ldw], records=records, fields=True)
    exhausted = int(words[:, program.nsteps:program.ldw].any(axis=1).sum())
    return [int(v) for v in tally] + [exhausted, int(words[:, program.ldw].sum())]


@pytest.mark.parametrize("name", ["steane", "rm15"])
def test_sites(name):
    code = oracle_code(name)
    n = int(code.n)
    site_loc, site_regions = stream_noise.CnotBlockType(code).gate_regions()
    assert site_loc.tolist() == list(range(0, 2 * n, 2)) and site_regions.tolist() == [[0, n]]
    assert site_loc.dtype == np.int32 and site_regions.dtype == np.int64
    for instructions in (X_CNOT_TWO, THREE, CNOT_MEASURE):
        got, _ = multi(name, instructions)
        at = 0
        for kind in got.types:
            loc, counts = kind.gate_regions()
            assert len(counts) == len(kind.regions) and np.array_equal(counts[:, 0] + 2 * counts[:, 1], kind.regions[:, 1])
            covered = np.zeros(kind.num_locations, dtype=np.int64)
            first = 0
            for (start, size, _), (n1, n2) in zip(kind.regions.tolist(), counts.tolist()):
                one, two = loc[first:first + n1], loc[first + n1:first + n1 + n2]
                assert (np.diff(one) > 0).all() and (np.diff(two) > 0).all()
                inside = np.concatenate([one, two, two + 1])
                assert len(inside) == size and (inside >= start).all() and (inside < start + size).all()      # no site in two regions
                np.add.at(covered, inside, 1)
                first += n1 + n2
            assert first == len(loc) and (covered == 1).all()
            assert np.array_equal(got.type_site_loc[at:at + len(loc)], loc)
            at += len(loc)
        assert at == len(got.type_site_loc) and len(got.type_site_regions) == len(got.type_regions)


@pytest.mark.parametrize("name, instructions, first, count, max_attempts",
                         [("steane", X_CNOT_TWO, 0, 2500, 256), ("steane", THREE, 1 << 40, 2000, 3), ("steane", X_CNOT_TWO, 77, 1500, 1),
                          ("rm15", CNOT_MEASURE, 5, 1000, 256), ("rm15", CNOT_MEASURE, 5, 1000, 3), ("steane", THREE, 9, 2000, 256)])
def test_host_statement_equals_the_restatement_and_the_full_frame_model(name, instructions, first, count, max_attempts):
    got, ref = multi(name, instructions)
    p1, p2 = RATES[name]
    words, attempts = got.retry_gate_words_host(count, p1, p2, seed=11, first_sample=first, max_attempts=max_attempts)
    want_words, want_attempts, faults = multi_retry_gate_ref.retry_gate_words(got, 11, first, count, p1, p2, max_attempts)
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
    # the location faults of the entered attempts, through the block tables and through the full-frame model
    assert int(alive.sum()) > 0 or max_attempts == 1
    assert np.array_equal(got.words_of_faults(*faults)[alive], words[alive, :got.ldw])
    full = ref.outcome_words(*stream_ref.dense_faults(got.num_locations, *faults))
    assert np.array_equal(full[alive], words[alive, :got.ldw])
    assert np.count_nonzero(words[alive, :got.nsteps]) > 0 or max_attempts == 1
    if max_attempts == 256:                                                             # CNOT events with both operands hit entered
        cnot_blocks = np.flatnonzero(got.block_kind == stream_noise.CNOT)
        where = faults[1].astype(np.int64)
        in_cnot = np.zeros(len(where), dtype=bool)
        for b in cnot_blocks:
            in_cnot |= (where >= got.block_start[b]) & (where < got.block_start[b + 1])
        assert int(in_cnot.sum()) > 0


def test_every_single_cnot_event():
    got, ref = multi("steane", CNOT_MEASURE)
    code = got.code
    keys = np.uint64(key_mask(int(code.r_1), int(code.r_2)))
    block = int(np.flatnonzero(got.block_kind == stream_noise.CNOT)[0])
    fa, fb = int(got.block_a[block]), int(got.block_b[block])
    start = int(got.block_start[block])
    steps = {int(got.block_a[b]): int(got.block_step[b]) for b in range(len(got.block_kind) - 1, block, -1) if got.block_kind[b] == stream_noise.EC}
    assert set(steps) == {fa, fb} and sorted(steps.values()) == [0, 1]                 # the next EC word of either block
    low, high = np.uint64(0xFFFFFFFF), np.uint64(0xFFFFFFFF00000000)
    events = [(site, kappa) for site in range(int(code.n)) for kappa in range(1, 16)]
    first, where, what = [0], [], []
    for site, kappa in events:
        for operand in range(2):
            kind = (kappa >> (2 * operand)) & 3
            if kind:
                where.append(start + 2 * site + operand)
                what.append(kind)
        first.append(len(where))
    faults = (np.array(first, dtype=np.int64), np.array(where, dtype=np.int32), np.array(what, dtype=np.uint8))
    words = got.words_of_faults(*faults)
    assert np.array_equal(words, ref.outcome_words(*stream_ref.dense_faults(got.num_locations, *faults)))
    assert not words[:, got.nsteps:].any()                                             # a CNOT block has no flag row
    for (site, kappa), row in zip(events, words):
        on = {fa: row[steps[fa]] & keys, fb: row[steps[fb]] & keys}
        # a single-qubit error of a distance-3 code has a non-zero syndrome: the word shows exactly the components kappa names
        assert bool(on[fa] & low) == bool(kappa & 1) and bool(on[fa] & high) == bool(kappa & 2), (site, kappa)
        assert bool(on[fb] & low) == bool(kappa & 4) and bool(on[fb] & high) == bool(kappa & 8), (site, kappa)
    # the faults of this model follow their gate: an X on the control alone (kappa = 1) stays on block a and a Z on it (kappa = 2)
    # likewise, while the same Paulis on the control's qubit before the CNOT block are moved by the frame map -- X to both blocks, Z
    # stays on one
    prepare = got.types[got.block_type[fa]]
    assert got.block_a[fa] == fa and got.block_kind[fa] == stream_noise.NONE
    clean = np.flatnonzero((prepare.effects[:, 0, 2] == 0) & (prepare.effects[:, 1, 2] == 0) & ((prepare.effects[:, 0, 1] & keys) != 0) &
                           ((prepare.effects[:, 1, 1] & keys) != 0))
    at = int(got.block_start[fa]) + int(clean[-1])
    before = got.words_of_faults(np.array([0, 1, 2], dtype=np.int64), np.array([at, at], dtype=np.int32), np.array([1, 2], dtype=np.uint8))
    assert before[0, steps[fa]] & keys and before[0, steps[fb]] & keys and before[0, steps[fa]] & keys == before[0, steps[fb]] & keys
    assert before[1, steps[fa]] & keys and not before[1, steps[fb]] & keys


@pytest.mark.parametrize("name, ops", [("steane", ""), ("steane", "XYZ"), ("rm15", "X")])
@pytest.mark.parametrize("max_attempts", [256, 2])
def test_one_qubit_programs_equal_the_gate_level_retried_route(name, ops, max_attempts):
    code = oracle_code(name)
    p1, p2 = RATES[name]
    one = stream_noise.StreamedGadget.program(code, ops)
    got = stream_noise.MultiProgram(code, [(op, 3) for op in ops] + [('MEASURE', 3)])
    assert got.preparations == one.preparations and got.ldw == one.ldw
    words, attempts = got.retry_gate_words_host(1500, p1, p2, seed=5, first_sample=1 << 33, max_attempts=max_attempts)
    want_words, want_attempts = one.retry_gate_words_host(1500, p1, p2, seed=5, first_sample=1 << 33, max_attempts=max_attempts)
    assert np.array_equal(words, want_words) and np.array_equal(attempts, want_attempts)
    assert np.count_nonzero(words[:, :got.nsteps]) > 0 and int(attempts.max()) > 1


def test_trivial_cases():
    got, _ = multi("steane", THREE)
    words, attempts = got.retry_gate_words_host(300, 0.0, 0.0, seed=1, max_attempts=7)
    assert not words[:, :got.ldw].any() and (words[:, got.ldw] == got.preparations).all() and (attempts == 1).all()
    for records in ('reference', 'propagated'):
        assert host_counts(got, words, records) == [300] + [0] * 20 + [300 * got.preparations]
    # either class alone: the restatement, and the faults lie on sites of that class only
    for p1, p2 in ((4e-3, 0.0), (0.0, 5e-3)):
        words, attempts = got.retry_gate_words_host(1500, p1, p2, seed=3, max_attempts=256)
        want_words, want_attempts, faults = multi_retry_gate_ref.retry_gate_words(got, 3, 0, 1500, p1, p2, 256)
        assert np.array_equal(words, want_words) and np.array_equal(attempts, want_attempts)
        assert np.count_nonzero(words[:, :got.nsteps]) > 0 and int(attempts.max()) > 1 and len(faults[1]) > 0
        gate_of = got.locations()[faults[1], 0]
        is_cnot = got.gates()[gate_of, 0] == stream_noise.GATE_CNOT
        assert is_cnot.all() if p1 == 0.0 else not is_cnot.any()


@pytest.mark.parametrize("name, instructions", [("steane", X_CNOT_TWO), ("rm15", CNOT_MEASURE)])
def test_tally_completes_the_statement(name, instructions):
    got, ref = multi(name, instructions)
    words, _ = got.retry_gate_words_host(3000, *RATES[name], seed=2, max_attempts=3)
    exhausted = words[:, got.nsteps:got.ldw].any(axis=1)
    assert 100 < int(exhausted.sum()) < 2900
    for records in ('reference', 'propagated'):
        counts, classes = got.tally_host(words[:, :got.ldw], records=records, fields=True, classes=True)
        assert np.array_equal((classes & 1).astype(bool), ~exhausted)                   # every exhausted sample is rejected
        assert counts.tolist() == ref.tally(words[:, :got.ldw], records)
        assert host_counts(got, words, records) == counts.tolist() + [int(exhausted.sum()), int(words[:, -1].sum())]
        assert int(counts[0]) + int(exhausted.sum()) == 3000 and int(counts[5]) > 0


def test_other_samples_than_the_location_route():
    got, _ = multi("steane", X_CNOT_TWO)
    p = 2e-3
    gate_words, gate_attempts = got.retry_gate_words_host(1000, p, p, seed=4)
    words, attempts = got.retry_words_host(1000, p / 3, p / 3, p / 3, seed=4)
    assert not np.array_equal(gate_attempts, attempts)
    assert int((gate_words[:, :got.nsteps] != words[:, :got.nsteps]).any(axis=1).sum()) > 100


def test_refusals():
    got, _ = multi("steane", CNOT_MEASURE)
    who = "gf2_mretry_gate_words_host: "
    eff, locs, flags, types, kinds, frame_a, frame_b, frames, regions, counts, site_loc, site_regions = got._retry_gate_sequence()
    cnot_type = next(t for t, kind in enumerate(got.types) if kind.kind == stream_noise.CNOT)
    cnot_block = int(np.flatnonzero(kinds == stream_noise.CNOT)[0])
    cnot_region = int(counts[:cnot_type].sum())
    cnot_site = int(site_regions[:cnot_region].sum())
    retried = int(np.flatnonzero(regions[:, 2] == 1)[0])
    retried_type = int(np.searchsorted(np.cumsum(counts), retried, side="right"))
    retried_local = retried - int(counts[:retried_type].sum())
    retried_site = int(site_regions[:retried].sum())
    first, size = int(regions[retried, 0]), int(regions[retried, 1])
    n1, n2 = (int(v) for v in site_regions[retried])
    assert n1 > 4 and n2 > 1

    def changed(array, at, value):
        out = array.copy()
        out[at] = value
        return out

    swapped = site_loc.copy()
    swapped[[retried_site + 3, retried_site + 4]] = swapped[[retried_site + 4, retried_site + 3]]
    # one one-operand site of the CNOT block: (1, 6) does not cover 14 locations, (2, 6) does, and is this route's own refusal
    two_single = np.concatenate([site_loc[:cnot_site], [0, 1], site_loc[cnot_site + 1:]]).astype(np.int32)
    cases = ((dict(site_regions=changed(site_regions, (retried, 0), n1 + 1), site_loc=np.insert(site_loc, retried_site, 0)),
              who + "region %d of block type %d has n_1 + 2 n_2 = %d + 2 * %d sites' locations, not its %d locations"
              % (retried_local, retried_type, n1 + 1, n2, size)),
             (dict(site_loc=changed(site_loc, retried_site, first + size)),
              who + "the sites of region %d of block type %d do not partition its locations %d .. %d: one-operand site 0 at location %d"
              % (retried_local, retried_type, first, first + size - 1, first + size)),
             (dict(site_loc=changed(site_loc, retried_site + 1, site_loc[retried_site])),
              who + "the sites of region %d of block type %d do not partition its locations %d .. %d: one-operand site 1 at location"
              % (retried_local, retried_type, first, first + size - 1)),
             (dict(site_loc=swapped), who + "the one-operand sites of region %d of block type %d are not ascending: site 4 at location"
              % (retried_local, retried_type)),
             (dict(site_loc=changed(site_loc, cnot_site + 1, 0)),
              who + "the sites of region 0 of block type %d do not partition its locations 0 .. 13: CNOT site 1 at location 0" % cnot_type),
             (dict(site_loc=two_single, site_regions=changed(changed(site_regions, (cnot_region, 0), 2), (cnot_region, 1), 6)),
              who + "the type of CNOT block %d has 2 one-operand sites: every site of a CNOT block is a physical CNOT" % cnot_block),
             (dict(regions=changed(regions, (cnot_region, 2), 1)),
              who + "the type of CNOT block %d has 1 regions, the first retried 1: a CNOT block has no flag rows" % cnot_block),
             (dict(regions=changed(regions, (retried, 2), 0)), "of block type %d (locations %d .. %d) is not retried but its locations set a flag bit"
              % (retried_type, first, first + size - 1)),
             (dict(max_attempts=0), who + "needs 1 <= max_attempts <= 65536, got 0"),
             (dict(max_attempts=65537), who + "needs 1 <= max_attempts <= 65536, got 65537"),
             (dict(ldw=got.ldw), who + "ldw must be at least the sequence's nsteps + F + 1 = %d words" % (got.ldw + 1)),
             (dict(frames=5), who + "needs 1 <= nframes <= 4 data frames"),
             (dict(p=(1.5, 0.0)), who + "needs 0 <= p_1, p_2 <= 1, got p_1 = "), (dict(p=(0.0, -0.1)), who + "needs 0 <= p_1, p_2 <= 1, got p_1 = "),
             (dict(p=(float("nan"), 0.0)), who + "needs 0 <= p_1, p_2 <= 1, got p_1 = "),
             (dict(first=-1), who + "negative range (needs count >= 0 and first_sample >= 0)"),
             (dict(count=-1), who + "negative range (needs count >= 0 and first_sample >= 0)"))
    for change, text in cases:
        args = dict(eff=eff, locs=locs, flags=flags, types=types, kinds=kinds, a=frame_a, b=frame_b, frames=frames, regions=regions, counts=counts,
                    site_loc=site_loc, site_regions=site_regions, first=0, count=2, p=RATES["steane"], max_attempts=256, ldw=got.ldw + 1)
        args.update(change)
        with pytest.raises(_native.GF2Error) as err:
            _native.mretry_gate_words_host(args['eff'], args['locs'], args['flags'], args['types'], args['kinds'], args['a'], args['b'],
                                           args['frames'], args['regions'], args['counts'], args['site_loc'], args['site_regions'], 3, args['first'],
                                           args['count'], *args['p'], args['max_attempts'], args['ldw'], got.preparations)
        assert text in str(err.value), (text, str(err.value))
    assert got.retry_gate_words_host(0, *RATES["steane"])[0].shape == (0, got.ldw + 1)
    assert got.retry_gate_words_host(2, *RATES["steane"], max_attempts=65536)[0].shape == (2, got.ldw + 1)
    with pytest.raises(ValueError, match="'reference' or 'propagated'"):
        got.retry_gate_counts(1, *RATES["steane"], records=2)
    with pytest.raises(ValueError, match=r"one \(n_1, n_2\) per region"):
        _native.mretry_gate_words_host(eff, locs, flags, types, kinds, frame_a, frame_b, frames, regions, counts, site_loc[:-1], site_regions, 3, 0, 2,
                                       *RATES["steane"], 256, got.ldw + 1, got.preparations)
    # the shared site rules keep their text under the one-qubit route's name
    one = stream_noise.StreamedGadget.program(oracle_code("steane"), "")
    seq = one._retry_gate_sequence()
    with pytest.raises(_native.GF2Error) as err:
        _native.retry_gate_words_host(*seq[:7], changed(seq[7], 0, int(seq[5][0, 1])), seq[8], 0, 0, 1, 1e-3, 1e-3, 256, one.ldw + 1, one.preparations)
    assert "gf2_retry_gate_words_host: the sites of region 0 of block type 0 do not partition its locations 0 .. %d: one-operand site 0 at location %d" \
        % (int(seq[5][0, 1]) - 1, int(seq[5][0, 1])) in str(err.value)


def test_exact_law_of_the_cnot_correlation():
    """Steane `CNOT 0 1; MEASURE 1` at p_1 = p_2 = 1e-3: the 12 key bits of the rounds on D_0 and D_1 right after the CNOT.  A CNOT block
    that failed as two independent operands with the same marginals would miss this law by a non-centrality of several hundred."""
    got, _ = multi("steane", CNOT_MEASURE)
    p, count = 1e-3, 200000
    law = multi_retry_gate_ref.cnot_pair_law(got, p, p)
    assert law.shape == (4096,) and abs(float(law.sum()) - 1.0) < 1e-12
    kept = law * count >= exact_dist.MIN_EXPECTED
    rest = float(law[~kept].sum())
    print("cells expecting >= 10 of %d samples: %d; rest-bin share %.4f %%" % (count, int(kept.sum()), 100.0 * rest))
    assert int(kept.sum()) == 106 and abs(rest - 0.0029) < 0.0002 and rest < exact_dist.MAX_REST_MASS      # before drawing
    # the power of the test: the same marginals per operand (4 p / 15 per kind), the operands independent
    independent = _independent_operand_law(got, p)
    assert float((count * (independent[kept] - law[kept]) ** 2 / law[kept]).sum()) > 500.0
    words, _ = got.retry_gate_words_host(count, p, p, seed=31, max_attempts=256)
    assert not words[:, got.nsteps:got.ldw].any()
    cells = multi_retry_gate_ref.cnot_pair_cells(words, int(got.code.r_1), int(got.code.r_2))
    exact_dist.assert_chi2("multi retry gate: key bits of the two rounds after the CNOT", np.bincount(cells, minlength=4096), law, count)


def _independent_operand_law(program, p):
    """cnot_pair_law with the CNOT block's operands failing independently, each kind of an operand at its marginal 4 p / 15."""
    class Independent(object):
        def __init__(self, block):
            self.effects, self.regions, self.locations = block.effects, block.regions, block.locations

        def gate_regions(self):
            return np.arange(len(self.effects), dtype=np.int32), np.array([[len(self.effects), 0]], dtype=np.int64)

    joint = retry_gate_ref.region_joint
    block = int(np.flatnonzero(program.block_kind == stream_noise.CNOT)[0])
    cnot = program.types[program.block_type[block]]

    def swapped(kind, region, p1, p2, local_mask, tail_mask):
        if kind is cnot:
            return joint(Independent(cnot), region, 3.0 * 4.0 * p2 / 15.0, 0.0, local_mask, tail_mask)
        return joint(kind, region, p1, p2, local_mask, tail_mask)

    retry_gate_ref.region_joint = swapped
    try:
        return multi_retry_gate_ref.cnot_pair_law(program, p, p)
    finally:
        retry_gate_ref.region_joint = joint


def test_attempts_and_exhaustion_laws():
    got, _ = multi("steane", X_CNOT_TWO)
    p1, p2 = RATES["steane"]
    count = 200000
    words, attempts = got.retry_gate_words_host(count, p1, p2, seed=21)
    mean, var = multi_retry_gate_ref.attempts_mean_var(got, p1, p2)
    assert not words[:, got.nsteps:got.ldw].any() and 1.1 * got.preparations < mean < 1.5 * got.preparations
    exact_dist.assert_z("multi retry gate: attempts of X_CNOT_TWO", int(words[:, -1].sum()), count * mean, count * var)
    keep = float(np.prod([1.0 - (1.0 - q) ** 2 for q in multi_retry_gate_ref.retried_pass_probabilities(got, p1, p2)]))
    assert 0.05 < keep < 0.95
    words, attempts = got.retry_gate_words_host(count, p1, p2, seed=22, max_attempts=2)
    alive = int((~words[:, got.nsteps:got.ldw].any(axis=1)).sum())
    exact_dist.assert_z("multi retry gate: not exhausted with two attempts", alive, count * keep, count * keep * (1.0 - keep))


def bare_enumeration(instructions, p1, p2):
    """Per MEASURE, the probability that the bare program's bit is wrong, by carrying the exact distribution over the X components of
    the physical qubits through the circuit and enumerating every Pauli of every gate: 3 of a one-operand gate (p1 / 3 each, a Pauli
    other than I and a measurement), 15 of a CNOT (p2 / 15 each), the fault following its gate and preceding a measurement."""
    instructions, qubits = ft_noise.check_instructions(instructions)
    index = {q: k for k, q in enumerate(qubits)}
    states = {(0,) * len(qubits): 1.0}

    def spread(states, flips):
        """flips: (probability, {qubit index: X component}) of every case"""
        out = {}
        for state, weight in states.items():
            for prob, flip in flips:
                new = list(state)
                for k, x in flip.items():
                    new[k] ^= x
                out[tuple(new)] = out.get(tuple(new), 0.0) + weight * prob
        return out

    def one(k):
        return [(1.0 - p1, {})] + [(p1 / 3.0, {k: kind & 1}) for kind in (1, 2, 3)]

    out = []
    for inst in instructions:
        if inst[0] == 'CNOT':
            a, b = index[inst[1]], index[inst[2]]
            moved = {}
            for state, weight in states.items():
                new = list(state)
                new[b] ^= new[a]
                moved[tuple(new)] = moved.get(tuple(new), 0.0) + weight
            states = spread(moved, [(1.0 - p2, {})] + [(p2 / 15.0, {a: kappa & 1, b: (kappa >> 2) & 1}) for kappa in range(1, 16)])
        elif inst[0] == 'MEASURE':
            k = index[inst[1]]
            states = spread(states, one(k))
            out.append(sum(weight for state, weight in states.items() if state[k]))
        elif inst[0] != 'I':
            states = spread(states, one(index[inst[1]]))
    return out


@pytest.mark.parametrize("instructions", [X_CNOT_TWO, THREE, CNOT_MEASURE, (('X', 0), ('CNOT', 0, 1), ('CNOT', 0, 1), ('Z', 1), ('MEASURE', 1))])
def test_bare_program_closed_form(instructions):
    for p1, p2 in itertools.product((0.0, 1e-3, 0.05), (0.0, 2e-3, 0.07)):
        got = ft_noise.raw_circuit_gate_error_rate(instructions, p1, p2)
        want = bare_enumeration(instructions, p1, p2)
        assert len(got) == len(want) == sum(1 for inst in instructions if inst[0] == 'MEASURE')
        assert np.allclose(got, want, rtol=1e-12, atol=1e-15), (got, want)
        assert all(0.0 < rate < 0.5 for rate in got) or (p1, p2) == (0.0, 0.0)
    # at p_1 = p_x + p_y + p_z of uniform kinds and no CNOT the location model's closed form
    assert np.allclose(ft_noise.raw_circuit_gate_error_rate((('X', 0), ('MEASURE', 0)), 3e-3, 0.0),
                       ft_noise.raw_circuit_error_rate((('X', 0), ('MEASURE', 0)), 1e-3, 1e-3, 1e-3))
