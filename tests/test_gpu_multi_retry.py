"""
The repeat-until-success sampler of multi-block programs on the GPU (stream_noise.MultiProgram.retry_*, csrc/gf2_mretry.hip;
DESIGN.md section 5d "Repeat-until-success of multi-block programs").  Every comparison is exact unless it says otherwise.

The device words must equal gf2_mretry_words_host, and the device counts under both settings of `records` gf2_mstream_tally_host
over those words plus the exhausted samples and the attempts.  The host statement itself is checked against the NumPy restatement
and against the post-selected route without a GPU (tests/test_multi_retry.py).  A case's reference is computed once and shared.

The programs are tests/test_gpu_multi_stream.py's five: one instantiation per frame count (three frames run as four), all six
ordered frame pairs, Reed-Muller (r_1 != r_2), tables staged in LDS and tables of 190 752 bytes read through L2.  Each runs at three
settings, 4096 samples each:
  (a) rates (1e-3, 5e-4, 1e-3), 256 attempts     every sample accepted, 1.26 to 1.82 attempts per preparation
  (b) the same rates, 3 attempts                 exact acceptance 0.70, 0.415, 0.137, 0.40, 0.042: accepted and exhausted samples
  (c) the case's own rate, 1 attempt             post-selection by this kernel: exact acceptance 0.062, 0.032, 0.081, 0.028, 0.137
"""
import functools

import numpy as np
import pytest

from oracle import exact_dist
from quantum_css_codes_amd import _native, stream_noise
from tests import retry_ref
from tests import stream_synthetic as syn
from tests.test_gpu_multi_stream import CASES, program
from tests.test_gpu_stream import make_code
from tests.test_multi_retry import host_counts

pytestmark = pytest.mark.gpu

SAMPLES = 1 << 12
RATES = (1e-3, 5e-4, 1e-3)
SETTINGS = ("a", "b", "c")


def setting_of(case, setting):
    """(rates, max_attempts)"""
    p = CASES[case][2]
    return {"a": (RATES, 256), "b": (RATES, 3), "c": ((p, p / 2, p), 1)}[setting]


def staged_limit(prog):
    """What mretry_launch leaves for the block tables: 160 KiB less the packed inverse-CDF tables, the attempts bin, the taken maps and
    the bins."""
    sizes = set()
    for _, count, _ in prog.type_regions.tolist():
        sizes.add(count - (count - 1) // 512 * 512)
        if count > 512:
            sizes.add(512)
    return 160 * 1024 - (sum(nb + 1 for nb in sizes) * 8 + 8 + 256 * 17 * 4 + 32 * 4)


@functools.lru_cache(maxsize=None)
def reference(case, setting):
    """(the host statement's words, its twenty-two counts under either setting of `records`); never modified."""
    name, instructions, _, seed, first = CASES[case]
    prog = program(name, instructions)
    p, limit = setting_of(case, setting)
    words, _ = prog.retry_words_host(SAMPLES, *p, seed=seed, first_sample=first, max_attempts=limit)
    words.setflags(write=False)
    return words, {records: host_counts(prog, words, records) for records in stream_noise.RECORDS}


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_words_and_counts_equal_the_host_statement(case, setting):
    name, instructions, _, seed, first = CASES[case]
    prog = program(name, instructions)
    p, limit = setting_of(case, setting)
    want_words, want = reference(case, setting)
    assert (prog.type_eff.nbytes > staged_limit(prog)) == (case == "rm15-unstaged")
    assert prog.type_eff.nbytes == 190752 or case != "rm15-unstaged"
    got = prog.retry_outcomes(SAMPLES, *p, seed=seed, first_sample=first, max_attempts=limit)
    assert got.shape == want_words.shape == (SAMPLES, prog.ldw + 1) and np.array_equal(got, want_words)
    reference_counts = want['reference']
    print("\n%s (%s): L = %d, %d blocks, %d preparations, reference %s" % (case, setting, prog.num_locations, len(prog.block_type), prog.preparations,
                                                                         reference_counts))
    accepted, exhausted, attempts = reference_counts[0], reference_counts[20], reference_counts[21]
    assert accepted + exhausted == SAMPLES
    if setting == "a":
        assert accepted == SAMPLES and attempts > 1.2 * prog.preparations * SAMPLES and reference_counts[5] >= 1
    elif setting == "b":
        assert accepted >= 100 and exhausted >= 100
    else:
        assert accepted >= 50
    for records in stream_noise.RECORDS:
        counts = prog.retry_counts(SAMPLES, *p, seed=seed, first_sample=first, records=records, max_attempts=limit)
        assert counts.tolist() == want[records] == host_counts(prog, got, records)
    as_dict = prog.retry_error_rates(SAMPLES, *p, seed=seed, first_sample=first, records='propagated', max_attempts=limit)
    tally = prog.tally_host(got[:, :prog.ldw], records='propagated')
    assert {k: v for k, v in as_dict.items() if k not in ('exhausted', 'attempts', 'preparations')} == tally
    assert (as_dict['exhausted'], as_dict['attempts'], as_dict['preparations']) == (exhausted, attempts, prog.preparations)
    if case == "steane-2" and setting == "a":
        code = make_code("steane")
        assert code.logical_circuit_retried_error_rates(instructions, SAMPLES, *p, seed=seed, first_sample=first, records='propagated') == as_dict


def test_records_change_the_counts_of_a_case():
    _, want = reference("steane-3-pairs", "a")
    assert want['reference'] != want['propagated'] and want['reference'][0] == want['propagated'][0] == SAMPLES


@pytest.mark.parametrize("name, ops", [("steane", ""), ("steane", "XYZIZYX"), ("rm15", "X")])
@pytest.mark.parametrize("limit", [256, 2])
def test_one_qubit_programs_equal_the_retried_kernel(name, ops, limit):
    code = make_code(name)
    one = stream_noise.stream_for(code, "program", tuple(ops))
    prog = program(name, tuple((op, 0) for op in ops) + (('MEASURE', 0),))
    want = one.retry_counts(SAMPLES, *RATES, seed=3, first_sample=9, max_attempts=limit)          # gf2_mc_retry_decode's fourteen
    assert want[0] >= 100 and (limit == 256 or want[12] >= 100)
    for records in stream_noise.RECORDS:
        got = prog.retry_counts(SAMPLES, *RATES, seed=3, first_sample=9, records=records, max_attempts=limit)
        assert [int(got[k]) for k in (0, 2, 3, 4, 5, 6, 7, 20, 21)] == [int(want[k]) for k in (0, 6, 7, 8, 9, 10, 11, 12, 13)]
        assert got[1] == got[4] and not got[8:20].any()
    assert np.array_equal(prog.retry_outcomes(2000, *RATES, seed=3, first_sample=9, max_attempts=limit),
                          one.retry_outcomes(2000, *RATES, seed=3, first_sample=9, max_attempts=limit))


def test_no_faults_no_failures():
    for case in ("steane-2", "steane-3-pairs", "rm15-unstaged"):
        name, instructions, _, _, _ = CASES[case]
        prog = program(name, instructions)
        for records in stream_noise.RECORDS:
            counts = prog.retry_counts(5000, 0.0, 0.0, 0.0, seed=1, records=records, max_attempts=5)
            assert counts.tolist() == [5000] + [0] * 20 + [5000 * prog.preparations]
        words = prog.retry_outcomes(300, 0.0, 0.0, 0.0)
        assert not words[:, :prog.ldw].any() and (words[:, prog.ldw] == prog.preparations).all()


@pytest.mark.parametrize("setting", ["a", "b"])
def test_shards_add_up(setting):
    name, instructions, _, seed, _ = CASES["steane-2"]
    prog = program(name, instructions)
    p, limit = setting_of("steane-2", setting)
    first = 1 << 33
    words, _ = prog.retry_words_host(SAMPLES + 2000, *p, seed=seed, first_sample=first, max_attempts=limit)
    for records in stream_noise.RECORDS:
        total = np.zeros(22, dtype=np.uint64)
        at = first
        for count in (1, 255, 1000, 0, 4097):                       # a count of 1, counts that are no multiple of 256
            total += prog.retry_counts(count, *p, seed=seed, first_sample=at, records=records, max_attempts=limit)
            at += count
        assert total.tolist() == host_counts(prog, words[:at - first], records)
    assert np.array_equal(prog.retry_outcomes(1, *p, seed=seed, first_sample=first + 777, max_attempts=limit), words[777:778])
    assert np.array_equal(prog.retry_outcomes(301, *p, seed=seed, first_sample=first + 5000, max_attempts=limit), words[5000:5301])


def test_a_long_program():
    # tests/test_gpu_multi_stream.py's 300 gates on two qubits, 205 490 locations: at these rates one attempt per preparation accepts
    # nothing, the retried walk everything
    gates = [(('X', 'CNOT', 'Z', 'CNOT', 'Y')[g % 5],) + ((g % 2, 1 - g % 2) if g % 5 in (1, 3) else (g % 2,)) for g in range(300)]
    prog = program("steane", tuple(gates) + (('MEASURE', 1), ('MEASURE', 0)))
    assert prog.num_locations > 190000 and prog.nsteps > 600
    count = 1 << 10
    want, _ = prog.retry_words_host(count, *RATES, seed=21, first_sample=5)
    got = prog.retry_outcomes(count, *RATES, seed=21, first_sample=5)
    assert np.array_equal(got, want)
    for records in stream_noise.RECORDS:
        counts = prog.retry_counts(count, *RATES, seed=21, first_sample=5, records=records)
        assert counts.tolist() == host_counts(prog, want, records)
    assert counts[0] == count and counts[20] == 0 and counts[21] > 1.2 * prog.preparations * count
    assert prog.counts(count, *RATES, seed=21, first_sample=5)[0] == 0


@functools.lru_cache(maxsize=None)
def long_regions_two_frames(r):
    """tests/stream_synthetic.long_regions' two block types (regions of 513, 7, 1024, 1100, 1 and of 511, 2, 600 locations; 64 and 63 flag
    rows) on frames 0 and 1 with CNOT blocks between them: first flag rows 0, 64, 127 and 191, the last two across two flag words."""
    b = syn._Builder("long_regions two frames", r, 2 * 2645 + 2 * 1113 + 3 * 30, p_total=syn.P_RETRY)
    type_a = [(513, 1, (1, 256), 0), (7, 0, (3, 2), 0), (1024, 1, (600, 212), 0), (1100, 1, (40, 530), 0), (1, 0, (1, 0), 0)]
    type_b = [(511, 1, (511, 0), 0), (2, 1, (0, 1), 0), (600, 1, (88, 256), 0)]
    cnot = dict(num_flags=0, regions=[(30, 0, None, 0)])
    b.add(2645, syn.EC, a=0, num_flags=64, regions=type_a).add(30, syn.CNOT, a=0, b=1, **cnot)
    b.add(1113, syn.MEASURE, a=0, num_flags=63, regions=type_b).add(30, syn.CNOT, a=1, b=0, **cnot)
    b.add(2645, syn.EC, a=1, num_flags=64, regions=type_a).add(30, syn.CNOT, a=0, b=1, **cnot)
    b.add(1113, syn.MEASURE, a=1, num_flags=63, regions=type_b)
    return b.done(nframes=2)


@pytest.mark.parametrize("limit", [256, 2])
@pytest.mark.parametrize("r", syn.R_SETS[:2])
def test_a_synthetic_sequence(r, limit):
    seq = long_regions_two_frames(r)
    assert [seq.flag_row_of(b) for b in (0, 2, 4, 6)] == [0, 64, 127, 191] and seq.flag_words == 4
    args = seq.mstream_args() + (seq.type_regions, seq.type_nregions)
    tables = syn.decoder(*r)
    ctx = _native.default_context()
    handle = ctx.mretry_create(*args)
    count, seed, first = 3000, 31, (1 << 33) + 5
    words, tries = _native.mretry_words_host(*args, seed, first, count, *seq.p, limit, seq.ldw + 1, seq.preparations)
    exhausted = words[:, seq.nsteps:seq.ldw].any(axis=1)
    if limit == 256:
        assert not exhausted.any() and int(tries.max()) > 4
    else:                                                           # the exhausted path: flags in every flag word, the straddles included
        assert 300 < int(exhausted.sum()) < count - 300 and all(words[:, seq.nsteps + q].any() for q in range(4))
    got = ctx.outcomes(ctx.mretry_outcomes_dev, handle, seed, first, count, *seq.p, seq.ldw + 1, limit)
    assert np.array_equal(got, words)
    for records in (0, 1):
        tally = _native.mstream_tally_host(np.ascontiguousarray(words[:, :seq.ldw]), seq.block_kind, seq.block_a, seq.block_b, seq.nframes,
                                           seq.flag_words, records, *tables)
        want = [int(v) for v in tally] + [int(exhausted.sum()), int(words[:, -1].sum())]
        assert ctx.mc_mretry_decode(handle, records, *tables, seed, first, count, *seq.p, limit).tolist() == want
        assert want[0] >= 300 and want[2] > 0 and want[5] > 0
    handle.free()


def test_refusals_of_the_device_entry_points():
    name, instructions, p, _, _ = CASES["steane-2"]
    prog = program(name, instructions)
    ctx = _native.default_context()
    device, tables = prog.retry_device(), prog._tables()
    with pytest.raises(_native.GF2Error, match=r"gf2_mc_mretry_decode: records must be GF2_MSTREAM_REFERENCE \(0\) or GF2_MSTREAM_PROPAGATED \(1\), got 2"):
        ctx.mc_mretry_decode(device, 2, *tables, 0, 0, 10, p, p, p, 256)
    with pytest.raises(_native.GF2Error, match=r"gf2_mretry_outcomes_dev: ldo must be at least the sequence's nsteps \+ F \+ 1 = 28 words"):
        ctx.outcomes(ctx.mretry_outcomes_dev, device, 0, 0, 10, p, p, p, prog.ldw, 256)
    with pytest.raises(_native.GF2Error, match="r_1, r_2 <= 31"):
        ctx.mc_mretry_decode(device, 0, 32, *tables[1:], 0, 0, 10, p, p, p, 256)
    with pytest.raises(_native.GF2Error, match="beyond the layout"):
        ctx.mc_mretry_decode(device, 0, 2, *tables[1:], 0, 0, 10, p, p, p, 256)
    for limit in (0, 65537):
        with pytest.raises(_native.GF2Error, match="gf2_mc_mretry_decode: needs 1 <= max_attempts <= 65536, got %d" % limit):
            ctx.mc_mretry_decode(device, 0, *tables, 0, 0, 10, p, p, p, limit)
        with pytest.raises(_native.GF2Error, match="gf2_mretry_outcomes_dev: needs 1 <= max_attempts"):
            ctx.outcomes(ctx.mretry_outcomes_dev, device, 0, 0, 10, p, p, p, prog.ldw + 1, limit)
    with pytest.raises(_native.GF2Error, match="gf2_mc_mretry_decode: negative range"):
        ctx.mc_mretry_decode(device, 0, *tables, 0, -1, 10, p, p, p, 256)
    regions = prog.type_regions.copy()
    cnot_type = next(t for t, kind in enumerate(prog.types) if kind.kind == stream_noise.CNOT)
    regions[int(prog.type_nregions[:cnot_type].sum()), 2] = 1
    with pytest.raises(_native.GF2Error, match="gf2_mretry_create: the type of CNOT block 4 has 1 regions, the first retried 1"):
        ctx.mretry_create(*prog._sequence(), regions, prog.type_nregions)
    # nine blocks in one 512-location segment: gf2_mstream_create refuses them, this route has no overlap rule
    eff, locs, flags, types, kinds, frame_a, frame_b, frames = prog._sequence()
    pauli = stream_noise.BlockType(prog.code, "logical X", stream_noise.NONE, stream_noise._emit_pauli([0, 1, 2]))
    many = (np.concatenate([eff, pauli.effects]), list(locs) + [3], list(flags) + [0], [len(locs)] * 9 + list(types), [0] * 9 + list(kinds),
            [0] * 9 + list(frame_a), [-1] * 9 + list(frame_b), frames, np.concatenate([prog.type_regions, [[0, 3, 0]]]), list(prog.type_nregions) + [1])
    handle = ctx.mretry_create(*many)
    want, _ = _native.mretry_words_host(*many, 1, 0, 500, *RATES, 256, prog.ldw + 1, prog.preparations)
    assert np.array_equal(ctx.outcomes(ctx.mretry_outcomes_dev, handle, 1, 0, 500, *RATES, prog.ldw + 1, 256), want)
    handle.free()


# ---- statistics ----------------------------------------------------------------------------------------------------------------

BIG = 1 << 24


def test_attempts_follow_the_geometric_law():
    name, instructions, _, _, _ = CASES["steane-2"]
    prog = program(name, instructions)
    p = (1e-3, 1e-3, 1e-3)
    counts = prog.retry_counts(BIG, *p, seed=51)
    mean, var = retry_ref.attempts_mean_var(prog, p)
    assert counts[0] == BIG and counts[20] == 0
    exact_dist.assert_z("multi retry: attempts of steane-2 at 1e-3", int(counts[21]), BIG * mean, BIG * var)


def test_rates_equal_the_post_selected_route():
    name, instructions, _, _, _ = CASES["steane-2"]
    prog = program(name, instructions)
    p = (1e-4, 1e-4, 1e-4)
    retried = prog.retry_error_rates(BIG, *p, seed=41)
    selected = prog.error_rates(1 << 26, *p, seed=42)
    assert retried['exhausted'] == 0 and retried['accepted'] == BIG
    assert 0.29 * (1 << 26) < selected['accepted'] < 0.32 * (1 << 26)               # exact acceptance 0.306
    n_1, n_2 = float(retried['accepted']), float(selected['accepted'])
    pairs = [("wrong_any", retried['wrong_any'], selected['wrong_any'])]
    for m in range(2):
        for field in ('wrong', 'first_trial_wrong', 'split_vote'):
            pairs.append(("%s of measurement %d" % (field, m), retried['measurements'][m][field], selected['measurements'][m][field]))
    for label, a, b in pairs:
        pooled = (a + b) / (n_1 + n_2)
        var = pooled * (1.0 - pooled) * (1.0 / n_1 + 1.0 / n_2)                      # of the difference of the two rates under the pooled rate
        exact_dist.assert_z("%s per accepted sample, retried - post-selected" % label, a / n_1 - b / n_2, 0.0, var)
