"""
The synthetic block sequences of tests/stream_synthetic.py without a GPU: what tests/test_gpu_stream_synthetic.py
compares the six streamed kernels against is tied here to restatements that share nothing with the library.

  1  the word-level tallies of tests/gadget_tally_ref.py (stream_tally, mstream_tally) equal the older restatements: ec_tally and
     ft_tally on real Steane sequences, multi_stream_ref.tally on tables that hold a part of the keys
  2  every host statement used as a GPU reference equals its restatement on the synthetic sequences: gf2_stream_words_host and
     gf2_mstream_words_host a NumPy XOR-and-frame-map walk written here (slot_walk), the four gf2_retry*_words_host tests/retry_ref.py
     and its siblings, the two tally host statements stream_tally and mstream_tally; 2000 samples each
  3  no reference is vacuous (the assertions are functions the GPU tests call again on their own references)
  4  ten wrong kernels, restated in NumPy, each change a reference at the committed seeds

Measured on an 8-core machine without a GPU: the module takes 16 s, most of it the per-sample tallies in Python.
"""
import functools
import itertools

import numpy as np
import pytest

from oracle import cpu_ref
from quantum_css_codes_amd import _native, stream_noise
from tests import gadget_tally_ref as ref, multi_stream_ref, retry_gate_ref, retry_gate_wait_ref, retry_ref, retry_wait_ref, stream_ref
from tests import stream_synthetic as syn
from tests.gate_mc_ref import SLOT_BASE as GATE_SLOT_BASE, cdf_table
from tests.strata_ref import GOLDEN, STREAM_MULT, mix64
from tests.test_multi_stream import random_words
from tests.test_stream import streamed

SAMPLES = 2000
SEED = syn.SEED0 + 7
FIRSTS = (0, (1 << 33) + 5)
SEG = syn.SEG
NONE, EC, MEASURE, FINAL, CNOT = syn.NONE, syn.EC, syn.MEASURE, syn.FINAL, syn.CNOT
LOW, HIGH = np.uint64(0x00000000FFFFFFFF), np.uint64(0xFFFFFFFF00000000)
FRAME = {NONE: 0, EC: retry_ref.FRAME[retry_ref.EC], MEASURE: 0xFFFFFFFF, FINAL: (1 << 64) - 1}

# ---- the cases: shared with tests/test_gpu_stream_synthetic.py -------------------------------------------------------------------------

STREAM_SEQS = {"overlap8-last1": lambda r: syn.overlap8_stream("last1", r), "overlap8-final8": lambda r: syn.overlap8_stream("final8", r),
               "flags64": lambda r: syn.flags64("stream", r)}
MSTREAM_SEQS = {"overlap8-1": lambda r: syn.overlap8_mstream(1, r), "overlap8-2": lambda r: syn.overlap8_mstream(2, r),
                "overlap8-3": lambda r: syn.overlap8_mstream(3, r), "overlap8-4": lambda r: syn.overlap8_mstream(4, r),
                "flags64": lambda r: syn.flags64("mstream", r)}
ROUTES = ("retry", "retry_wait", "retry_gate", "retry_gate_wait")
#  name: (sequence of the location routes, sequence of the gate routes, max_attempts)
RETRY_SEQS = {"long_regions": (syn.long_regions, syn.long_regions, 256), "long_regions-2": (syn.long_regions, syn.long_regions, 2),
              "sixteen_sizes": (lambda r: syn.sixteen_sizes("location", r), lambda r: syn.sixteen_sizes("gate", r), 256),
              "sixteen_sizes-staged": (lambda r: syn.sixteen_sizes("location-staged", r), lambda r: syn.sixteen_sizes("gate-staged", r), 256),
              "sixteen_sizes-full": (lambda r: syn.sixteen_sizes("location-full", r), lambda r: syn.sixteen_sizes("gate-full", r), 256),
              "flags64": (lambda r: syn.flags64("retry", r), lambda r: syn.flags64("retry", r), 256),
              "flags64-2": (lambda r: syn.flags64("retry", r), lambda r: syn.flags64("retry", r), 2),
              "attempts": (syn.attempts, syn.attempts, 65536)}


STREAM_CASES = [("stream", name) for name in STREAM_SEQS] + [("mstream", name) for name in MSTREAM_SEQS]
#  every retried sequence with every (r_1, r_2); `attempts` and the sixteen largest sizes with the first
RETRY_CASES = [(route, name, r) for route in ROUTES for name in RETRY_SEQS
               for r in (syn.R_SETS[:1] if name in ("attempts", "sixteen_sizes-full") else syn.R_SETS)]
RETRY_IDS = ["%s-%s-r%d-%d" % ((route, name) + r) for route, name, r in RETRY_CASES]
CASES = [(route, name, r) for route, name in STREAM_CASES for r in syn.R_SETS] + RETRY_CASES


def case_seed(route, name, r):
    """(seed, first sample) of a case from its place among all cases: the first sample is 0 and 2^33 + 5 in turn."""
    number = CASES.index((route, name, tuple(r)))
    return SEED + number, FIRSTS[number % 2]


def retry_sequence(route, name, r):
    location, gate, limit = RETRY_SEQS[name]
    return (gate if "gate" in route else location)(r), limit


# ---- the host statements as the references of the GPU tests --------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def stream_reference(route, name, r, count):
    """(seq, seed, first, faults, words) by gf2_stream_words_host / gf2_mstream_words_host on the oracle's sampler."""
    seq = (STREAM_SEQS if route == "stream" else MSTREAM_SEQS)[name](r)
    seed, first = case_seed(route, name, r)
    faults = syn.frozen(*stream_ref.sampled_faults(seq.locations, seed, first, count, seq.p))
    if route == "stream":
        words = _native.stream_words_host(*seq.stream_args(), *faults, seq.ldw)
    else:
        words = _native.mstream_words_host(*seq.mstream_args(), *faults, seq.ldw)
    return seq, seed, first, faults, syn.frozen(words)[0]


def tally_host(route, seq, words, tables, records=0):
    if route == "mstream":
        return _native.mstream_tally_host(words, seq.block_kind, seq.block_a, seq.block_b, seq.nframes, seq.flag_words, records, *tables).tolist()
    return _native.stream_tally_host(words, seq.block_kind, seq.flag_words, *tables).tolist()


def retry_rates(route, seq):
    return (seq.p_gate if "gate" in route else seq.p) + (seq.q if "wait" in route else ())


def retry_tables(route, seq):
    return seq.retry_args() + (seq.sites() if "gate" in route else ()) + (seq.waits() if "wait" in route else ())


@functools.lru_cache(maxsize=None)
def retry_reference(route, name, r, count):
    """(seq, seed, first, max_attempts, words, attempts) by the route's gf2_retry*_words_host."""
    seq, limit = retry_sequence(route, name, r)
    seed, first = case_seed(route, name, r)
    host = getattr(_native, route + "_words_host")
    words, tries = host(*retry_tables(route, seq), seed, first, count, *retry_rates(route, seq), limit, seq.ldw + (2 if "wait" in route else 1),
                        seq.preparations)
    return (seq, seed, first, limit) + syn.frozen(words, tries)


def retry_restated(route, seq, seed, first, count, limit):
    if route == "retry":
        return retry_ref.retry_words(seq, seed, first, count, seq.p, limit)
    if route == "retry_gate":
        return retry_gate_ref.retry_gate_words(seq, seed, first, count, *seq.p_gate, limit)
    if route == "retry_wait":
        return retry_wait_ref.retry_wait_words(*retry_wait_ref.tables_of(seq), seed, first, count, seq.p, seq.q, limit)
    return retry_gate_wait_ref.retry_gate_wait_words(*retry_gate_wait_ref.tables_of(seq), seed, first, count, *seq.p_gate, seq.q, limit)


def host_counts(route, seq, words, tables):
    """The fourteen or fifteen counts of a retried route: gf2_stream_tally_host on the first nsteps + F words, the exhausted samples, the
    attempts and, with waiting faults, those."""
    fields = tally_host("stream", seq, words[:, :seq.ldw], tables)
    extra = [len(words) - fields[0], int(words[:, seq.ldw].sum(dtype=np.uint64))]
    return fields + extra + ([int(words[:, seq.ldw + 1].sum(dtype=np.uint64))] if "wait" in route else [])


# ---- non-vacuity: asserted on a reference before any device is asked -----------------------------------------------------------------------

def assert_decoder_counts(name, counts, key0, fields=range(1, 8)):
    """Of a streamed tally with a FINAL step under a decoder set: the flips, the FINAL misses and the unmatched keys all occur.  The
    flips are counted once a sample and stay below the accepted samples under every table set.  So do the FINAL misses and the
    unmatched keys (counted once a step) where the tables hold key 0: a lookup of key 0 -> flip 1 flips the record but is a hit.
    Without key 0 every quiet step is a miss and so is the FINAL step of every sample whose frame is matched: the unmatched keys only
    have to occur, and the FINAL misses may reach the accepted samples but not pass them."""
    assert all(counts[f] > 0 for f in fields), (name, key0, counts)
    assert all(counts[f] < counts[0] for f in fields if f < 4 or key0 != "absent"), (name, key0, counts)
    assert all(counts[f] <= counts[0] for f in fields if f < 6), (name, key0, counts)


def assert_flags64_words(seq, words):
    """Some stored flag word has bit 63 of a 64-row type set, and the high part of the type that lies across two words is non-zero."""
    flag = words[:, seq.nsteps:seq.nsteps + seq.flag_words]
    assert seq.flag_words == 5 and (flag[:, 0] >> np.uint64(63)).any() and (flag[:, 2] >> np.uint64(63)).any(), seq.name
    assert flag[:, 4].any() and (flag[:, 3] >> np.uint64(5)).any(), seq.name   # rows 197 .. 260: bits 5 .. 63 of word 3, bits 0 .. 4 of word 4


def assert_share(name, part, count):
    assert 20 * part >= count, (name, part, count)                            # at least 5 % of the samples


def assert_retry_reference(route, name, reference, counts):
    """Accepted and exhausted samples are each 5 % at max_attempts = 2 and nothing is exhausted otherwise; the mean attempts per
    preparation lie between 1.2 and 4 (the host statement's attempts column); a sample of `attempts` needs more than 256."""
    seq, seed, first, limit, words, tries = reference
    count = len(words)
    assert counts[0] + counts[12] == count and counts[13] == int(tries.sum(dtype=np.uint64))
    if limit == 2:                                                              # lanes exhaust inside accepted wavefronts
        assert_share(name, counts[0], count)
        assert_share(name, counts[12], count)
        assert words[:, seq.nsteps:seq.ldw].any(axis=1).sum() == counts[12]
    else:
        assert counts[12] == 0 and not words[:, seq.nsteps:seq.ldw].any(), (name, counts)
    if name == "attempts":
        assert int(tries.max()) > 256 and counts[12] == 0, (route, int(tries.max()))
    else:
        made = tries[tries > 0]
        assert 1.2 <= made.mean() <= 4.0, (route, name, float(made.mean()))
    if "wait" in route:
        assert counts[14] > 0 or name == "attempts", (route, name, counts)


# ---- 1: the new restatements against the old ones ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("what,key", [("cycle", (1, False)), ("cycle", (5, False)), ("program", ()), ("program", tuple("XY"))])
def test_stream_tally_equals_the_older_restatements_on_steane(what, key):
    gadget = streamed("steane", what, key)
    eff = gadget.dense_effects()
    rng = np.random.default_rng(5)
    words = np.zeros((3000, gadget.ldw), dtype=np.uint64)                      # XORs of up to three single faults, as tests/test_stream.py makes them
    for k in range(3):
        pick, comp = rng.integers(0, gadget.num_locations, len(words)), rng.integers(0, 2, len(words))
        words ^= np.where((rng.random(len(words)) < (1.0, 0.6, 0.3)[k])[:, None], eff[pick, comp], np.uint64(0))
    tables = gadget._tables()
    got = ref.stream_tally(words, gadget.block_kind, gadget.flag_words, *tables)
    if what == "cycle":
        want = ref.ec_tally(gadget.to_cycle_layout(words), gadget.nsteps - 1, *tables)
        assert got[:8] == want and got[8:] == [0] * 4 and want[3] >= 10
    else:
        mask = sum(1 << int(s) for s in gadget.block_step[gadget.block_kind == stream_noise.MEASURE])
        want = ref.ft_tally(gadget.to_program_layout(words), gadget.nsteps, mask, *tables)
        assert [got[k] for k in (0, 8, 9, 10, 11, 6, 7)] == want and got[1:6] == [0] * 5 and want[2] >= 10
    assert 100 <= got[0] <= len(words) - 100


def test_mstream_tally_equals_the_older_restatement_with_unmatched_keys():
    # tests/test_multi_stream.py's construction (test_tally_host_with_unmatched_keys_on_both_sides): random full-rank checks on 9 bits,
    # tables that hold a part of the keys, four frames, CNOTs in both directions, one to five trials
    rng = np.random.default_rng(17)
    vectors = np.array(list(itertools.product((0, 1), repeat=9)))

    def side(r, entries):
        while True:
            check = rng.integers(0, 2, (r, 9))
            keys = np.array([cpu_ref.vec_to_int(v) for v in (vectors @ check.T) % 2])
            if len(set(keys.tolist())) == 1 << r:
                break
        return check, {int(k): vectors[np.flatnonzero(keys == k)[0]] for k in rng.choice(1 << r, entries, replace=False)}

    class Tables(object):
        n, r_1, r_2 = 9, 5, 6
        x_op, z_op = rng.integers(0, 2, (1, 9)), rng.integers(0, 2, (1, 9))
        x_operator_matrix = lambda self: self.x_op
        z_operator_matrix = lambda self: self.z_op

    code = Tables()
    (code.parity_check_c1, code._c1_syndromes), (code.parity_check_c2, code._c2_syndromes) = side(5, 12), side(6, 20)
    keys1 = np.array(list(code._c1_syndromes), dtype=np.uint64)
    flips1 = np.array([int(code.x_op[0] @ v) & 1 for v in code._c1_syndromes.values()], dtype=np.uint8)
    keys2 = np.array(list(code._c2_syndromes), dtype=np.uint64)
    flips2 = np.array([int(code.z_op[0] @ v) & 1 for v in code._c2_syndromes.values()], dtype=np.uint8)
    E, M, C = multi_stream_ref.EC, multi_stream_ref.MEASURE, multi_stream_ref.GATE_CNOT
    for frames, events in ((1, [(M, 0, 0)]),
                           (2, [(E, 0), (E, 1), (C, 0, 1), (E, 0), (E, 1), (C, 1, 0), (E, 1)] + [(M, 1, 0), (E, 0), (E, 1)] * 3),
                           (4, [(E, 3), (C, 3, 0), (E, 0), (C, 0, 2), (E, 2), (C, 2, 1), (E, 1), (C, 1, 3)] + [(M, 2, 0), (E, 2), (E, 1)] * 5 +
                               [(M, 0, 1), (E, 3)] * 5 + [(M, 3, 2)] * 5 + [(M, 1, 3), (C, 0, 1)] * 5)):
        kinds = [{E: EC, M: MEASURE, C: CNOT}[e[0]] for e in events]
        frame_a = [e[1] for e in events]
        frame_b = [e[2] if e[0] == C else -1 for e in events]
        nsteps = sum(e[0] != C for e in events)
        words = random_words(rng, 5, 6, events, nsteps + 2, 2000)
        both = []
        for records in ('reference', 'propagated'):
            want = multi_stream_ref.tally(code, events, frames, words, records)
            got = ref.mstream_tally(words, kinds, frame_a, frame_b, frames, 2, stream_noise.RECORDS[records], 5, keys1, flips1, 6, keys2, flips2)
            assert got == want and want[2] > 0 and (want[3] > 0 or frames == 1) and want[1] > 0
            both.append(got)
        assert (both[0] != both[1]) == (frames > 1)


# ---- 2: the host statements against their restatements -----------------------------------------------------------------------------------------

def slot_walk(seq, faults, count, fold_eighth=False, close_late=False, drop_straddle=False):
    """The words of samples given by their faults, by XOR and the frame map -- and, for section 4, what three wrong kernels would store.
    A fault is put where the streamed kernels put it: segment s = location // 512, lo = the first block that ends after the segment's
    start, slot = block - lo, the table row from the slot's block.  fold_eighth: slot 7 is taken for slot 6.  close_late: a block that ends
    exactly at a segment's start still holds slot 0 there, so eight blocks of that segment need nine slots and the chain of compares stops
    at the eighth.  drop_straddle: the part of a block's flags that belongs to the next flag word is not stored."""
    fault_first, location, kind = faults
    sample = np.repeat(np.arange(count), np.diff(fault_first))
    location = location.astype(np.int64)
    start = seq.start
    ends = start[1:]
    type_offset = np.concatenate([[0], np.cumsum(seq.type_locations)])
    has_rows = seq.block_type >= 0
    base = np.where(has_rows, type_offset[np.where(has_rows, seq.block_type, 0)], 0)[:len(ends)] - start[:-1]
    block = np.searchsorted(start, location, side='right') - 1
    seg_start = location // SEG * SEG
    lo = np.searchsorted(ends, seg_start, side='left' if close_late else 'right')
    slot = block - lo
    assert slot.min() >= 0 and slot.max() <= (8 if close_late else 7)
    if fold_eighth:
        slot = np.where(slot == 7, 6, slot)
    slot = np.minimum(slot, 7)
    block = lo + slot
    row = (base[block] + location) % len(seq.type_eff)                      # (a wrong slot's row may lie outside the table: any row shows it)
    nblocks = len(seq.block_kind)
    acc = np.zeros((count, nblocks, 3), dtype=np.uint64)
    for component in (0, 1):
        has = ((kind >> component) & 1) == 1
        np.bitwise_xor.at(acc, (sample[has], block[has]), seq.type_eff[row[has], component])
    words = np.zeros((count, seq.ldw), dtype=np.uint64)
    T = np.zeros((seq.nframes, count), dtype=np.uint64)
    step = flag_row = 0
    for b, (t, kind_, a, c) in enumerate(zip(seq.block_type.tolist(), seq.block_kind.tolist(), seq.block_a.tolist(), seq.block_b.tolist())):
        if kind_ == CNOT:
            T[c] ^= T[a] & LOW
            T[a] ^= T[c] & HIGH
            T[a] ^= acc[:, b, 0]
            T[c] ^= acc[:, b, 1]
            continue
        if kind_ != NONE:
            words[:, step] = (T[a] & np.uint64(FRAME[kind_])) ^ acc[:, b, 0]
            step += 1
        if kind_ != FINAL:
            word, shift = divmod(flag_row, 64)
            words[:, seq.nsteps + word] |= acc[:, b, 2] << np.uint64(shift)
            if shift and word + 1 < seq.flag_words and not drop_straddle:
                words[:, seq.nsteps + word + 1] |= acc[:, b, 2] >> np.uint64(64 - shift)
            flag_row += seq.type_flags[t]
            T[a] ^= acc[:, b, 1]
    return words


@pytest.mark.parametrize("r", syn.R_SETS, ids=lambda r: "r%d-%d" % r)
@pytest.mark.parametrize("route, name", STREAM_CASES)
def test_streamed_host_statements_equal_the_walk_and_the_tallies(route, name, r):
    seq, seed, first, faults, words = stream_reference(route, name, r, SAMPLES)
    assert np.array_equal(words, slot_walk(seq, faults, SAMPLES))
    accepted = int((~words[:, seq.nsteps:].any(axis=1)).sum())
    assert_share(name, accepted, SAMPLES)
    assert_share(name, SAMPLES - accepted, SAMPLES)
    if name == "flags64":
        assert_flags64_words(seq, words)
    vectors = []
    for key0 in syn.KEY0:
        tables = syn.decoder(*r, key0)
        for records in (0, 1) if route == "mstream" else (0,):
            got = tally_host(route, seq, words, tables, records)
            if route == "stream":
                assert got == ref.stream_tally(words, seq.block_kind, seq.flag_words, *tables)
                assert_decoder_counts(name, got, key0)
            else:
                assert got == ref.mstream_tally(words, seq.block_kind, seq.block_a, seq.block_b, seq.nframes, seq.flag_words, records, *tables)
                assert got[2] > 0 and got[3] > 0, (name, key0, got)
                if key0 == "zero":
                    assert got[2] < got[0] and got[3] < got[0], (name, got)
                if name == "overlap8-4" and key0 == "zero":                     # the fields of all four measurements
                    assert all(v > 0 for v in got[4:]), got
            assert got[0] == accepted
            vectors.append(tuple(got))
    assert len(set(vectors[::2] if route == "mstream" else vectors)) == 3       # the three ways of key 0 give three different count vectors
    if route == "mstream":                                                      # ... and the two settings of `records` where a CNOT joins two frames
        assert any(vectors[k] != vectors[k + 1] for k in (0, 2, 4)) == (seq.nframes > 1), name


def test_tables_hold_a_key_with_bit_30_and_half_of_the_single_row_keys():
    for r in syn.R_SETS:
        r1, keys1, flips1, r2, keys2, flips2 = syn.decoder(*r)
        seq = syn.overlap8_stream("last1", r)
        for width, keys, shift in ((r1, keys1, 32), (r2, keys2, 0)):
            assert width < 31 or ((keys >> np.uint64(30)) & np.uint64(1)).any()
            produced = np.unique((seq.type_eff[:, :, :2] >> np.uint64(shift)) & np.uint64((1 << width) - 1))
            produced = produced[produced != 0]
            held = np.isin(produced, keys).sum()
            assert 0 < len(produced) and len(produced) // 4 <= held <= len(produced) - len(produced) // 4 or width == 1 and held == 0


@pytest.mark.parametrize("route, name, r", RETRY_CASES, ids=RETRY_IDS)
def test_retried_host_statements_equal_their_restatements(route, name, r):
    reference = retry_reference(route, name, r, SAMPLES)
    seq, seed, first, limit, words, tries = reference
    want, want_tries = retry_restated(route, seq, seed, first, SAMPLES, limit)
    assert np.array_equal(words, want) and np.array_equal(tries, want_tries)
    tables = syn.decoder(*r)
    counts = host_counts(route, seq, words, tables)
    assert counts[:12] == ref.stream_tally(words[:, :seq.ldw], seq.block_kind, seq.flag_words, *tables)
    assert_retry_reference(route, name, reference, counts)
    if name == "long_regions":
        vectors = [tuple(counts)]
        assert_decoder_counts(name, counts, "zero")
        for key0 in syn.KEY0[1:]:
            other = host_counts(route, seq, words, syn.decoder(*r, key0))
            assert_decoder_counts(name, other, key0)
            vectors.append(tuple(other))
        assert len(set(vectors)) == 3
    if name == "long_regions-2":                                                # the exhausted samples' flags: bit 63 of a 64-row type is stored
        assert (words[:, seq.nsteps] >> np.uint64(63)).any()
    if name == "flags64-2":
        assert_flags64_words(seq, words)


def test_both_first_samples_occur_in_every_group_of_cases():
    for group in ("stream", "mstream") + ROUTES:
        for name in {case[1] for case in CASES if case[0] == group and case[1] not in ("attempts", "sixteen_sizes-full")}:
            assert {case_seed(*case)[1] for case in CASES if case[:2] == (group, name)} == set(FIRSTS), (group, name)
        assert {case_seed(*case)[1] for case in CASES if case[0] == group} == set(FIRSTS)


def test_sixteen_sizes_are_sixteen():
    r = syn.R_SETS[0]
    last = lambda n: n - (n - 1) // SEG * SEG
    seq = syn.sixteen_sizes("location", r)
    assert sorted({last(int(n)) for n in seq.type_regions[:, 1]}) == list(syn.SIZES16) and int(seq.type_regions[:, 1].max()) == 1024
    assert len(set(seq.wait_count.tolist())) == 16 and int(seq.wait_count.max()) == 512
    gate = syn.sixteen_sizes("gate", r)
    for cl in (0, 1):
        assert sorted({last(int(n)) for n in gate.site_regions[:, cl]}) == list(syn.SIZES16) and int(gate.site_regions[:, cl].max()) == 1024
    assert sorted(set(gate.wait_count.tolist()) - {0}) == [510, 511, 512]
    for variant, routes in (("location", ROUTES[:2]), ("location-staged", ROUTES[:2]), ("gate", ROUTES[2:]), ("gate-staged", ROUTES[2:])):
        for route in routes:
            wait_rows, block_tables, used = lds_plan(route, syn.sixteen_sizes(variant, r))
            assert block_tables == variant.endswith("staged") and (wait_rows or variant == "location"), (variant, route)
    assert lds_plan("retry", syn.sixteen_sizes("location-staged", r))[2] == 158816
    assert lds_plan("retry_wait", syn.sixteen_sizes("location-staged", r))[2] == 162768      # of 163 840: a fifteenth size does not fit
    # packed tables have nb + 1 entries, so the 32 + 3 tables of SIZES16 and the waits 510 .. 512 are 62 208 bytes: with the staged wait
    # rows that launch asks for 128 752 of the 163 840 bytes
    assert lds_plan("retry_gate_wait", gate) == (True, False, 128752)
    # the sixteen largest sizes: 35 tables of 141 696 bytes and 17 488 bytes of maps and bins, 4 656 bytes short of the budget, and no
    # wait row fits.  (The static_assert of gf2_retry_gate_wait.hip bounds 35 tables of 513 entries, 161 128 bytes with the fixed part:
    # sixteen sizes of a class are distinct, so no sequence gets closer than this one.)
    full, location_full = syn.sixteen_sizes("gate-full", r), syn.sixteen_sizes("location-full", r)
    for cl in (0, 1):
        assert sorted({last(int(n)) for n in full.site_regions[:, cl]}) == list(syn.SIZES_FULL)
    assert sorted({last(int(n)) for n in location_full.type_regions[:, 1]}) == sorted(set(location_full.wait_count.tolist())) == list(syn.SIZES_FULL)
    assert lds_plan("retry_gate_wait", full) == (False, False, 159184) and lds_plan("retry_gate", full) == (True, False, 146888)
    assert lds_plan("retry_wait", location_full) == (False, False, 146896) and lds_plan("retry", location_full) == (True, False, 82184)
    for route in ROUTES:                                                        # the long regions are read through L2
        assert not lds_plan(route, syn.long_regions(r))[1]


def lds_plan(route, seq):
    """(the wait rows are staged, the block tables are staged, the launch's bytes of LDS): the launch code's arithmetic on 160 KiB of
    LDS, restated -- inferred from the launch code, not observed: the library does not tell which instantiation it launched.  The packed
    inverse-CDF tables come first (nb + 1 entries of 8 bytes per distinct segment size, per class at gate level, and per distinct wait
    count), then the taken maps (256 lanes x 17 dwords), the bins and the 64-bit bins; then the wait rows (32 bytes each) if they fit;
    then the block tables (48 bytes a location) with the site table (4 bytes a site) if all of that still fits."""
    last = lambda n: n - (n - 1) // SEG * SEG
    groups = [seq.site_regions[:, 0], seq.site_regions[:, 1]] if "gate" in route else [seq.type_regions[:, 1]]
    sizes = [{last(int(n)) for n in group if n} | ({SEG} if group.max() > SEG else set()) for group in groups]
    if "wait" in route:
        sizes.append({int(w) for w in seq.wait_count if w})
    used = sum(sum(nb + 1 for nb in group) for group in sizes) * 8 + 256 * 17 * 4 + 16 * 4 + (16 if "wait" in route else 8)
    wait_rows = "wait" in route and used + 32 * int(seq.wait_count.sum()) <= 160 * 1024
    used += 32 * int(seq.wait_count.sum()) if wait_rows else 0
    tables = seq.type_eff.nbytes + (4 * len(seq.site_loc) if "gate" in route else 0)
    staged = used + tables <= 160 * 1024
    return wait_rows or "wait" not in route, staged, used + (tables if staged else 0)


# ---- 4: wrong kernels change the references ----------------------------------------------------------------------------------------------------

def wrong_location_draw(how):
    """tests/retry_ref.draw_region with one of three mistakes: "a" whole segments counted with the last segment's table, "b" the last
    segment counted with the whole-segment table, "c" the row index without 512 s."""
    def draw_region(ka, eff, t_any, t_12, tables):
        count, out = len(eff), np.zeros((len(ka), 3), dtype=np.uint64)
        nseg = (count + SEG - 1) // SEG
        for s in range(nseg):
            nb = min(SEG, count - SEG * s)
            table_of = (count - SEG * (nseg - 1)) if how == "a" else SEG if how == "b" else nb
            if nseg == 1:
                table_of = nb                                                   # (one segment: there is no other table to confuse it with)
            cdf = cdf_table(t_any, table_of)[:nb]
            d = mix64(ka + retry_ref._u64(STREAM_MULT * (s + 1)))
            K = ((d >> np.uint64(32))[:, None] >= cdf[None, :]).sum(axis=1).astype(np.int64)
            taken = np.zeros((len(ka), nb), dtype=bool)
            for k in range(int(K.max()) if len(ka) else 0):
                rows = np.nonzero(K > k)[0]
                v = mix64(d[rows] + retry_ref._u64(GOLDEN * (k + 1)))
                hi, c = v >> np.uint64(32), (v & np.uint64(0xFFFFFFFF)).astype(np.int64)
                j = nb - K[rows] + k
                t = ((hi * (j + 1).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
                pos = np.where(taken[rows, t], j, t)
                taken[rows, pos] = True
                where = pos if how == "c" else SEG * s + pos
                out[rows[c < t_12[1]]] ^= eff[where[c < t_12[1]], 0]
                out[rows[c >= t_12[0]]] ^= eff[where[c >= t_12[0]], 1]
        return out
    return draw_region


def gate_draw(ka, eff, site_loc, n1, n2, t_class, tables, slot_zero=False):
    """tests/retry_gate_ref.draw_region; slot_zero: every segment of a class is drawn from the class's slot 0 (mistake "d")."""
    out = np.zeros((len(ka), 3), dtype=np.uint64)
    for cl, (m, base) in enumerate(((n1, 0), (n2, n1))):
        for s in range((m + SEG - 1) // SEG):
            nb = min(SEG, m - SEG * s)
            cdf = cdf_table(t_class[cl], nb)
            d = mix64(ka + retry_ref._u64(STREAM_MULT * (GATE_SLOT_BASE[cl] + (0 if slot_zero else s) + 1)))
            K = ((d >> np.uint64(32))[:, None] >= cdf[None, :]).sum(axis=1).astype(np.int64)
            taken = np.zeros((len(ka), nb), dtype=bool)
            for k in range(int(K.max()) if len(ka) else 0):
                rows = np.nonzero(K > k)[0]
                v = mix64(d[rows] + retry_ref._u64(GOLDEN * (k + 1)))
                hi, lo = v >> np.uint64(32), v & np.uint64(0xFFFFFFFF)
                j = nb - K[rows] + k
                t = ((hi * (j + 1).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
                pos = np.where(taken[rows, t], j, t)
                taken[rows, pos] = True
                kappa = (1 + ((lo * np.uint64(retry_gate_ref.RADIX[cl])) >> np.uint64(32))).astype(np.int64)
                loc = site_loc[base + SEG * s + pos]
                for bit in range(4):
                    has = ((kappa >> bit) & 1).astype(bool)
                    out[rows[has]] ^= eff[loc[has] + (bit >> 1), bit & 1]
    return out


@pytest.mark.parametrize("how", ["a", "b", "c"])
def test_wrong_segment_tables_and_rows_change_the_retried_words(how, monkeypatch):
    r = syn.R_SETS[0]
    seq, seed, first, limit, words, tries = retry_reference("retry", "long_regions", r, SAMPLES)
    monkeypatch.setattr(retry_ref, "draw_region", wrong_location_draw(None))
    assert np.array_equal(retry_ref.retry_words(seq, seed, first, SAMPLES, seq.p, limit)[0], words)      # the copy without a mistake is the restatement
    monkeypatch.setattr(retry_ref, "draw_region", wrong_location_draw(how))
    wrong = retry_ref.retry_words(seq, seed, first, SAMPLES, seq.p, limit)[0]
    assert (wrong != words).any(axis=1).sum() >= 20, how


def test_one_segment_slot_for_a_whole_class_changes_the_gate_words(monkeypatch):
    r = syn.R_SETS[0]
    for name in ("long_regions", "sixteen_sizes"):
        seq, seed, first, limit, words, tries = retry_reference("retry_gate", name, r, SAMPLES)
        monkeypatch.setattr(retry_gate_ref, "draw_region", gate_draw)
        assert np.array_equal(retry_gate_ref.retry_gate_words(seq, seed, first, SAMPLES, *seq.p_gate, limit)[0], words)   # the copy without the mistake
        monkeypatch.setattr(retry_gate_ref, "draw_region", functools.partial(gate_draw, slot_zero=True))
        wrong = retry_gate_ref.retry_gate_words(seq, seed, first, SAMPLES, *seq.p_gate, limit)[0]
        assert (wrong != words).any(axis=1).sum() >= 20, name


@pytest.mark.parametrize("route, name", [("stream", "overlap8-last1"), ("stream", "overlap8-final8"), ("mstream", "overlap8-2"), ("mstream", "overlap8-4")])
def test_wrong_overlap_slots_change_the_streamed_words(route, name):
    seq, seed, first, faults, words = stream_reference(route, name, syn.R_SETS[0], SAMPLES)
    folded = slot_walk(seq, faults, SAMPLES, fold_eighth=True)                  # (e)
    assert (folded != words).any(axis=1).sum() >= 5, name
    if name != "overlap8-final8":                                               # (f): eight blocks with locations behind a block that ends on 512 k
        late = slot_walk(seq, faults, SAMPLES, close_late=True)
        assert (late != words).any(axis=1).sum() >= 5, name


@pytest.mark.parametrize("route, name", [("stream", "flags64"), ("mstream", "flags64")])
def test_a_dropped_straddle_changes_the_flag_words(route, name):
    seq, seed, first, faults, words = stream_reference(route, name, syn.R_SETS[0], SAMPLES)
    dropped = slot_walk(seq, faults, SAMPLES, drop_straddle=True)               # (j)
    assert (dropped != words).any(axis=1).sum() >= 5
    tables = syn.decoder(*syn.R_SETS[0])
    assert tally_host(route, seq, dropped, tables)[0] > tally_host(route, seq, words, tables)[0]   # ... and accepts samples that are rejected


def packed_mstream_tally(words, seq, records, tables, or_flip=False):
    """tests/gadget_tally_ref.mstream_tally with the records packed as mstream_kernel packs them, K | P << 31 in one word per side and
    frame, a hit XOR-ing key | flip << 31 into it.  or_flip: the flip bit is OR-ed in instead (mistake "h")."""
    sides = ref._sides(*tables)
    blocks = list(zip(seq.block_kind.tolist(), seq.block_a.tolist(), seq.block_b.tolist()))
    measured = []
    for kind, a, _ in blocks:
        if kind == MEASURE and a not in measured:
            measured.append(a)
    trials = sum(k == MEASURE for k, _, _ in blocks) // len(measured)
    counts = [0] * 20
    for row in words.tolist():
        if any(row[seq.nsteps:seq.ldw]):
            continue
        counts[0] += 1
        record = [[0, 0] for _ in range(seq.nframes)]
        outcomes = {frame: [] for frame in measured}
        s = 0
        for kind, a, b in blocks:
            if kind == CNOT:
                if records:
                    record[b][0] ^= record[a][0]
                    record[a][1] ^= record[b][1]
                continue
            if kind == NONE:
                continue
            for side in (0, 1) if kind == EC else (0,):
                shift, mask, table = sides[side]
                key = ((row[s] >> shift) & mask) ^ (record[a][side] & 0x7FFFFFFF)
                if key in table:
                    record[a][side] = (record[a][side] ^ key) | table[key] << 31 if or_flip else record[a][side] ^ (key | table[key] << 31)
                else:
                    counts[2 + side] += 1
            if kind == MEASURE:
                outcomes[a].append(((row[s] >> 31) & 1) ^ (record[a][0] >> 31))
            s += 1
        for m, frame in enumerate(measured):
            wrong = sum(outcomes[frame])
            for k, v in enumerate((2 * wrong > trials, wrong, outcomes[frame][0], 0 < wrong < trials)):
                counts[4 + 4 * m + k] += v
        counts[1] += any(2 * sum(outcomes[frame]) > trials for frame in measured)
    return counts


def test_wrong_tallies_change_the_counts():
    r = (31, 31)
    tables = syn.decoder(*r)
    seq, seed, first, faults, words = stream_reference("stream", "overlap8-last1", r, SAMPLES)
    right = ref.stream_tally(words, seq.block_kind, seq.flag_words, *tables)
    for narrow in ((30, 31), (31, 30)):                                         # (g) a key mask of 30 bits where r = 31
        short = (narrow[0],) + tables[1:3] + (narrow[1],) + tables[4:]
        assert ref.stream_tally(words, seq.block_kind, seq.flag_words, *short) != right
    # (i) zero_ok taken as 1 where key 0 is absent, or where it flips: the lookups of key 0 are skipped, which is what key 0 -> flip 0 gives
    for key0 in ("absent", "one"):
        assert ref.stream_tally(words, seq.block_kind, seq.flag_words, *syn.decoder(*r, key0)) != right
    for name in ("overlap8-2", "overlap8-4"):                                    # (h) the record's flip bit OR-ed into bit 31
        seq, seed, first, faults, words = stream_reference("mstream", name, r, SAMPLES)
        for records in (0, 1):
            right = ref.mstream_tally(words, seq.block_kind, seq.block_a, seq.block_b, seq.nframes, seq.flag_words, records, *tables)
            assert packed_mstream_tally(words, seq, records, tables) == right
            assert packed_mstream_tally(words, seq, records, tables, or_flip=True) != right
