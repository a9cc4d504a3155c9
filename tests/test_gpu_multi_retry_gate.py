"""
The repeat-until-success sampler of multi-block programs under gate-level faults on the GPU (stream_noise.MultiProgram.retry_gate_*,
csrc/gf2_mretry_gate.hip; DESIGN.md section 5d "Repeat-until-success of multi-block programs under gate-level faults").  Every
comparison is exact unless it says otherwise.

The device words must equal gf2_mretry_gate_words_host, and the device counts under both settings of `records`
gf2_mstream_tally_host over those words plus the exhausted samples and the attempts.  The host statement itself is checked against
the NumPy restatement, the full-frame model and the exact law of the CNOT's correlation without a GPU
(tests/test_multi_retry_gate.py).  A case's reference is computed once and shared.

The programs are tests/test_gpu_multi_stream.py's five: one instantiation per frame count (three frames run as four), all six
ordered frame pairs, Reed-Muller (r_1 != r_2), tables staged in LDS and tables read through L2.  Each runs at three settings, 4096
samples each, the rates picked on the host so that the host reference shows what the setting is for:
  (a) Steane (3e-3, 4e-3), Reed-Muller (1.5e-3, 2.5e-3), 256 attempts    every sample accepted, 1.27 / 1.41 attempts per preparation
  (b) the same rates, 3 attempts                                         accepted and exhausted samples, at least 100 each
  (c) (2 p, 3 p) of the case's own rate p, 1 attempt                     gate-level post-selection by this kernel, at least 50 kept
"""
import functools

import numpy as np
import pytest

from oracle import exact_dist
from quantum_css_codes_amd import _native, stream_noise
from tests import multi_retry_gate_ref
from tests import stream_synthetic as syn
from tests.test_gpu_multi_stream import CASES, program
from tests.test_gpu_stream import make_code
from tests.test_multi_retry_gate import host_counts

pytestmark = pytest.mark.gpu

SAMPLES = 1 << 12
RATES = {"steane": (3e-3, 4e-3), "rm15": (1.5e-3, 2.5e-3)}
SETTINGS = ("a", "b", "c")


def setting_of(case, setting):
    """(p_1, p_2, max_attempts)"""
    name, _, p, _, _ = CASES[case]
    return {"a": RATES[name] + (256,), "b": RATES[name] + (3,), "c": (2 * p, 3 * p, 1)}[setting]


def staged_limit(prog):
    """What mretry_gate_launch leaves for the block tables and the site table: 160 KiB less the packed inverse-CDF tables of both
    classes, the attempts bin, the taken maps and the bins."""
    words = 0
    for cl in range(2):
        sizes = set()
        for m in prog.type_site_regions[:, cl].tolist():
            if m > 0:
                sizes.add(m - (m - 1) // 512 * 512)
            if m > 512:
                sizes.add(512)
        words += sum(nb + 1 for nb in sizes)
    return 160 * 1024 - (words * 8 + 8 + 256 * 17 * 4 + 32 * 4)


@functools.lru_cache(maxsize=None)
def reference(case, setting):
    """(the host statement's words, its twenty-two counts under either setting of `records`); never modified."""
    name, instructions, _, seed, first = CASES[case]
    prog = program(name, instructions)
    p1, p2, limit = setting_of(case, setting)
    words, _ = prog.retry_gate_words_host(SAMPLES, p1, p2, seed=seed, first_sample=first, max_attempts=limit)
    words.setflags(write=False)
    return words, {records: host_counts(prog, words, records) for records in stream_noise.RECORDS}


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_words_and_counts_equal_the_host_statement(case, setting):
    name, instructions, _, seed, first = CASES[case]
    prog = program(name, instructions)
    p1, p2, limit = setting_of(case, setting)
    want_words, want = reference(case, setting)
    tables = prog.type_eff.nbytes + prog.type_site_loc.nbytes
    assert (tables > staged_limit(prog)) == (case == "rm15-unstaged")                 # the path: staged in LDS, or read through L2
    got = prog.retry_gate_outcomes(SAMPLES, p1, p2, seed=seed, first_sample=first, max_attempts=limit)
    assert got.shape == want_words.shape == (SAMPLES, prog.ldw + 1) and np.array_equal(got, want_words)
    reference_counts = want['reference']
    print("\n%s (%s): L = %d, %d sites, %d blocks, %d preparations, reference %s"
          % (case, setting, prog.num_locations, len(prog.type_site_loc), len(prog.block_type), prog.preparations, reference_counts))
    accepted, exhausted, attempts = reference_counts[0], reference_counts[20], reference_counts[21]
    assert accepted + exhausted == SAMPLES
    if setting == "a":
        assert accepted == SAMPLES and attempts > 1.2 * prog.preparations * SAMPLES and reference_counts[5] >= 1
    elif setting == "b":
        assert accepted >= 100 and exhausted >= 100
    else:
        assert accepted >= 50
    for records in stream_noise.RECORDS:
        counts = prog.retry_gate_counts(SAMPLES, p1, p2, seed=seed, first_sample=first, records=records, max_attempts=limit)
        assert counts.tolist() == want[records] == host_counts(prog, got, records)
    as_dict = prog.retry_gate_error_rates(SAMPLES, p1, p2, seed=seed, first_sample=first, records='propagated', max_attempts=limit)
    tally = prog.tally_host(got[:, :prog.ldw], records='propagated')
    assert {k: v for k, v in as_dict.items() if k not in ('exhausted', 'attempts', 'preparations')} == tally
    assert (as_dict['exhausted'], as_dict['attempts'], as_dict['preparations']) == (exhausted, attempts, prog.preparations)
    if case == "steane-2" and setting == "a":
        code = make_code("steane")
        assert code.logical_circuit_retried_gate_error_rates(instructions, SAMPLES, p1, p2, seed=seed, first_sample=first,
                                                             records='propagated') == as_dict


def test_records_change_the_counts_of_a_case():
    _, want = reference("steane-3-pairs", "a")
    assert want['reference'] != want['propagated'] and want['reference'][0] == want['propagated'][0] == SAMPLES


@pytest.mark.parametrize("name, ops", [("steane", ""), ("steane", "XYZIZYX"), ("rm15", "X")])
@pytest.mark.parametrize("limit", [256, 2])
def test_one_qubit_programs_equal_the_gate_level_retried_kernel(name, ops, limit):
    code = make_code(name)
    p1, p2 = RATES[name]
    one = stream_noise.stream_for(code, "program", tuple(ops))
    prog = program(name, tuple((op, 0) for op in ops) + (('MEASURE', 0),))
    want = one.retry_gate_counts(SAMPLES, p1, p2, seed=3, first_sample=9, max_attempts=limit)     # gf2_mc_retry_gate_decode's fourteen
    assert want[0] >= 100 and (limit == 256 or want[12] >= 100)
    for records in stream_noise.RECORDS:
        got = prog.retry_gate_counts(SAMPLES, p1, p2, seed=3, first_sample=9, records=records, max_attempts=limit)
        assert [int(got[k]) for k in (0, 2, 3, 4, 5, 6, 7, 20, 21)] == [int(want[k]) for k in (0, 6, 7, 8, 9, 10, 11, 12, 13)]
        assert got[1] == got[4] and not got[8:20].any()
    assert np.array_equal(prog.retry_gate_outcomes(2000, p1, p2, seed=3, first_sample=9, max_attempts=limit),
                          one.retry_gate_outcomes(2000, p1, p2, seed=3, first_sample=9, max_attempts=limit))


def test_no_faults_and_either_class_alone():
    for case in ("steane-2", "steane-3-pairs", "rm15-unstaged"):
        name, instructions, _, _, _ = CASES[case]
        prog = program(name, instructions)
        for records in stream_noise.RECORDS:
            counts = prog.retry_gate_counts(5000, 0.0, 0.0, seed=1, records=records, max_attempts=5)
            assert counts.tolist() == [5000] + [0] * 20 + [5000 * prog.preparations]
        words = prog.retry_gate_outcomes(300, 0.0, 0.0)
        assert not words[:, :prog.ldw].any() and (words[:, prog.ldw] == prog.preparations).all()
    name, instructions, _, seed, _ = CASES["steane-4"]
    prog = program(name, instructions)
    for p1, p2 in ((5e-3, 0.0), (0.0, 6e-3)):
        want, _ = prog.retry_gate_words_host(2000, p1, p2, seed=seed)
        assert want[:, :prog.nsteps].any() and int(want[:, -1].max()) > prog.preparations
        assert np.array_equal(prog.retry_gate_outcomes(2000, p1, p2, seed=seed), want)
        for records in stream_noise.RECORDS:
            assert prog.retry_gate_counts(2000, p1, p2, seed=seed, records=records).tolist() == host_counts(prog, want, records)


@pytest.mark.parametrize("setting", ["a", "b"])
def test_shards_add_up(setting):
    name, instructions, _, seed, _ = CASES["steane-2"]
    prog = program(name, instructions)
    p1, p2, limit = setting_of("steane-2", setting)
    first = 1 << 33
    words, _ = prog.retry_gate_words_host(SAMPLES + 2000, p1, p2, seed=seed, first_sample=first, max_attempts=limit)
    for records in stream_noise.RECORDS:
        total = np.zeros(22, dtype=np.uint64)
        at = first
        for count in (1, 255, 1000, 0, 4097):                       # a count of 1, counts that are no multiple of 256
            total += prog.retry_gate_counts(count, p1, p2, seed=seed, first_sample=at, records=records, max_attempts=limit)
            at += count
        assert total.tolist() == host_counts(prog, words[:at - first], records)
    assert np.array_equal(prog.retry_gate_outcomes(1, p1, p2, seed=seed, first_sample=first + 777, max_attempts=limit), words[777:778])
    assert np.array_equal(prog.retry_gate_outcomes(301, p1, p2, seed=seed, first_sample=first + 5000, max_attempts=limit), words[5000:5301])


def test_a_long_program():
    # tests/test_gpu_multi_stream.py's 300 gates on two qubits, 205 490 locations
    gates = [(('X', 'CNOT', 'Z', 'CNOT', 'Y')[g % 5],) + ((g % 2, 1 - g % 2) if g % 5 in (1, 3) else (g % 2,)) for g in range(300)]
    prog = program("steane", tuple(gates) + (('MEASURE', 1), ('MEASURE', 0)))
    assert prog.num_locations > 190000 and prog.nsteps > 600
    count = 1 << 10
    p1, p2 = RATES["steane"]
    want, _ = prog.retry_gate_words_host(count, p1, p2, seed=21, first_sample=5)
    got = prog.retry_gate_outcomes(count, p1, p2, seed=21, first_sample=5)
    assert np.array_equal(got, want)
    for records in stream_noise.RECORDS:
        counts = prog.retry_gate_counts(count, p1, p2, seed=21, first_sample=5, records=records)
        assert counts.tolist() == host_counts(prog, want, records)
    assert counts[0] == count and counts[20] == 0 and counts[21] > 1.2 * prog.preparations * count


@functools.lru_cache(maxsize=None)
def long_regions_two_frames(r):
    """tests/stream_synthetic.long_regions' two block types (regions of 513, 7, 1024, 1100, 1 and of 511, 2, 600 locations; 64 and 63 flag
    rows; 600 one-operand sites in one region, 530 CNOT sites in another) on frames 0 and 1 with CNOT blocks of 15 CNOT sites between
    them: first flag rows 0, 64, 127 and 191, the last two across two flag words."""
    b = syn._Builder("long_regions two frames, gates", r, 2 * 2645 + 2 * 1113 + 3 * 30, p_total=syn.P_RETRY)
    type_a = [(513, 1, (1, 256), 0), (7, 0, (3, 2), 0), (1024, 1, (600, 212), 0), (1100, 1, (40, 530), 0), (1, 0, (1, 0), 0)]
    type_b = [(511, 1, (511, 0), 0), (2, 1, (0, 1), 0), (600, 1, (88, 256), 0)]
    cnot = dict(num_flags=0, regions=[(30, 0, (0, 15), 0)])
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
    assert int(seq.site_regions[:, 0].max()) > 512 and int(seq.site_regions[:, 1].max()) > 512
    args = seq.mstream_args() + (seq.type_regions, seq.type_nregions) + seq.sites()
    tables = syn.decoder(*r)
    p1, p2 = 0.7 * syn.P_RETRY, 0.7 * syn.P_RETRY                   # picked on the host: at 2 attempts 1037 / 1125 of 3000 samples are accepted
    ctx = _native.default_context()
    handle = ctx.mretry_gate_create(*args)
    count, seed, first = 3000, 31, (1 << 33) + 5
    words, tries = _native.mretry_gate_words_host(*args, seed, first, count, p1, p2, limit, seq.ldw + 1, seq.preparations)
    exhausted = words[:, seq.nsteps:seq.ldw].any(axis=1)
    if limit == 256:
        assert not exhausted.any() and int(tries.max()) > 4
    else:                                                           # the exhausted path: flags in every flag word, the straddles included
        assert 300 < int(exhausted.sum()) < count - 300 and all(words[:, seq.nsteps + q].any() for q in range(4))
    buf = ctx.alloc(count * (seq.ldw + 1) * 8)
    ctx.mretry_gate_outcomes_dev(handle, seed, first, count, p1, p2, limit, buf, seq.ldw + 1)
    got = buf.download((count, seq.ldw + 1), np.uint64)
    buf.free()
    assert np.array_equal(got, words)
    for records in (0, 1):
        tally = _native.mstream_tally_host(np.ascontiguousarray(words[:, :seq.ldw]), seq.block_kind, seq.block_a, seq.block_b, seq.nframes,
                                           seq.flag_words, records, *tables)
        want = [int(v) for v in tally] + [int(exhausted.sum()), int(words[:, -1].sum())]
        assert ctx.mc_mretry_gate_decode(handle, records, *tables, seed, first, count, p1, p2, limit).tolist() == want
        assert want[0] >= 300 and want[2] > 0 and want[5] > 0
    handle.free()


def test_refusals_of_the_device_entry_points():
    name, instructions, p, _, _ = CASES["steane-2"]
    prog = program(name, instructions)
    ctx = _native.default_context()
    device, tables = prog.retry_gate_device(), prog._tables()
    buf = ctx.alloc(10 * (prog.ldw + 1) * 8)
    with pytest.raises(_native.GF2Error, match=r"gf2_mc_mretry_gate_decode: records must be GF2_MSTREAM_REFERENCE \(0\) or GF2_MSTREAM_PROPAGATED \(1\), got 2"):
        ctx.mc_mretry_gate_decode(device, 2, *tables, 0, 0, 10, p, p, 256)
    with pytest.raises(_native.GF2Error, match=r"gf2_mretry_gate_outcomes_dev: ldo must be at least the sequence's nsteps \+ F \+ 1 = 28 words"):
        ctx.mretry_gate_outcomes_dev(device, 0, 0, 10, p, p, 256, buf, prog.ldw)
    with pytest.raises(_native.GF2Error, match="r_1, r_2 <= 31"):
        ctx.mc_mretry_gate_decode(device, 0, 32, *tables[1:], 0, 0, 10, p, p, 256)
    for limit in (0, 65537):
        with pytest.raises(_native.GF2Error, match="gf2_mc_mretry_gate_decode: needs 1 <= max_attempts <= 65536, got %d" % limit):
            ctx.mc_mretry_gate_decode(device, 0, *tables, 0, 0, 10, p, p, limit)
        with pytest.raises(_native.GF2Error, match="gf2_mretry_gate_outcomes_dev: needs 1 <= max_attempts"):
            ctx.mretry_gate_outcomes_dev(device, 0, 0, 10, p, p, limit, buf, prog.ldw + 1)
    with pytest.raises(_native.GF2Error, match="gf2_mc_mretry_gate_decode: negative range"):
        ctx.mc_mretry_gate_decode(device, 0, *tables, 0, -1, 10, p, p, 256)
    with pytest.raises(_native.GF2Error, match="gf2_mretry_gate_outcomes_dev: needs 0 <= p_1, p_2 <= 1"):
        ctx.mretry_gate_outcomes_dev(device, 0, 0, 10, 1.5, p, 256, buf, prog.ldw + 1)
    buf.free()
    regions = prog.type_regions.copy()
    cnot_type = next(t for t, kind in enumerate(prog.types) if kind.kind == stream_noise.CNOT)
    regions[int(prog.type_nregions[:cnot_type].sum()), 2] = 1
    with pytest.raises(_native.GF2Error, match="gf2_mretry_gate_create: the type of CNOT block 4 has 1 regions, the first retried 1"):
        ctx.mretry_gate_create(*prog._sequence(), regions, prog.type_nregions, prog.type_site_loc, prog.type_site_regions)
    sites = prog.type_site_loc.copy()
    sites[0], sites[1] = sites[1], sites[0]
    with pytest.raises(_native.GF2Error, match="gf2_mretry_gate_create: the one-operand sites of region 0 of block type 0 are not ascending"):
        ctx.mretry_gate_create(*prog._retry_sequence(), sites, prog.type_site_regions)


# ---- statistics ----------------------------------------------------------------------------------------------------------------

BIG = 1 << 24
PAIR = (('CNOT', 0, 1), ('MEASURE', 1))


@pytest.mark.parametrize("p, rest", [(1e-3, 5e-5), (1e-2, 0.0)])
def test_key_bits_after_the_cnot_follow_the_exact_law(p, rest):
    """tests/test_multi_retry_gate.py's exact law of the CNOT's correlation on 2^26 device samples: at 1e-3 the rest bin holds 0.005 % of
    the mass, at 1e-2 all 4096 cells are kept and the smallest pass probability of a region is 0.49."""
    prog = program("steane", PAIR)
    count, chunk = 1 << 26, 1 << 22
    law = multi_retry_gate_ref.cnot_pair_law(prog, p, p)
    sparse = float(law[law * count < exact_dist.MIN_EXPECTED].sum())
    least = min(multi_retry_gate_ref.retried_pass_probabilities(prog, p, p))
    print("rest-bin share %.5f %%, smallest pass probability %.3f" % (100.0 * sparse, least))
    assert sparse <= rest * 1.2 and sparse <= exact_dist.MAX_REST_MASS                  # before drawing
    assert p != 1e-2 or (int((law * count >= exact_dist.MIN_EXPECTED).sum()) == 4096 and abs(least - 0.49) < 0.01)
    hist = np.zeros(4096, dtype=np.int64)
    for start in range(0, count, chunk):
        words = prog.retry_gate_outcomes(chunk, p, p, seed=61, first_sample=start)
        assert not words[:, prog.nsteps:prog.ldw].any()                                  # (exhaustion at 256 attempts: below 1e-70)
        hist += np.bincount(multi_retry_gate_ref.cnot_pair_cells(words[:, :2], 3, 3), minlength=4096)
    exact_dist.assert_chi2("multi retry gate: key bits of the two rounds after the CNOT at p = %g" % p, hist, law, count)


def test_attempts_follow_the_geometric_law():
    name, instructions, _, _, _ = CASES["steane-2"]
    prog = program(name, instructions)
    p = 1e-3
    counts = prog.retry_gate_counts(BIG, p, p, seed=51)
    mean, var = multi_retry_gate_ref.attempts_mean_var(prog, p, p)
    assert counts[0] == BIG and counts[20] == 0
    exact_dist.assert_z("multi retry gate: attempts of steane-2 at 1e-3", int(counts[21]), BIG * mean, BIG * var)


def test_rates_equal_gate_level_post_selection():
    """2^24 retried samples against 2^26 at max_attempts = 1.  The rate, picked on the host: at p_1 = p_2 = 5e-4 one attempt per
    preparation keeps 0.261 of the samples (the product of the exact pass probabilities), and a host run of 4e5 retried samples counts
    649 or more in every field compared, so either side expects more than 2e4."""
    name, instructions, _, _, _ = CASES["steane-2"]
    prog = program(name, instructions)
    p = 5e-4
    keep = float(np.prod(multi_retry_gate_ref.retried_pass_probabilities(prog, p, p)))
    assert keep >= 0.10
    retried = prog.retry_gate_error_rates(BIG, p, p, seed=41)
    selected = prog.retry_gate_error_rates(1 << 26, p, p, seed=42, max_attempts=1)
    assert retried['exhausted'] == 0 and retried['accepted'] == BIG
    assert selected['accepted'] >= 0.10 * (1 << 26) and abs(selected['accepted'] / float(1 << 26) - keep) < 1e-3
    n_1, n_2 = float(retried['accepted']), float(selected['accepted'])
    pairs = [("wrong_any", retried['wrong_any'], selected['wrong_any'])]
    for m in range(2):
        for field in ('wrong', 'first_trial_wrong', 'split_vote'):
            pairs.append(("%s of measurement %d" % (field, m), retried['measurements'][m][field], selected['measurements'][m][field]))
    for label, a, b in pairs:
        print("%s: %d of %d retried, %d of %d at one attempt" % (label, a, n_1, b, n_2))
        assert a >= 100 and b >= 100
        pooled = (a + b) / (n_1 + n_2)
        var = pooled * (1.0 - pooled) * (1.0 / n_1 + 1.0 / n_2)                      # of the difference of the two rates under the pooled rate
        exact_dist.assert_z("%s per accepted sample, retried - one attempt" % label, a / n_1 - b / n_2, 0.0, var)
