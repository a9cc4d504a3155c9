"""
The six streamed kernels on the synthetic block sequences of tests/stream_synthetic.py (DESIGN.md section 5h "Synthetic block
sequences"): stream_kernel, mstream_kernel, retry_kernel, retry_wait_kernel, retry_gate_kernel and retry_gate_wait_kernel on the paths no
sequence of a real code reaches -- regions and classes of more than one sampler segment, sixteen packed inverse-CDF tables per class and
three wait tables beside them (the sixteen largest sizes: 159 184 of the 163 840 bytes of LDS), eight blocks in one segment, block ends on multiples of 512, decoder tables
with 31-bit keys that miss keys and lack key 0 or flip on it, flag rows 63 and across two flag words, more than 256 attempts.

Every comparison is exact: the stored words equal the host statement's words, the counts the host tally of those words.
tests/test_stream_synthetic.py ties each host statement used here to a restatement that shares nothing with the library, on the same
sequences, and shows that ten wrong kernels would change these references.  Every reference asserts that it is not vacuous before the
device is asked.  4096 samples per case, first samples 0 and 2^33 + 5 in turn, max_attempts = 256 but where a case says otherwise, raw
_native.Context entry points on a context of the module's own, every handle freed, every test under a time limit of its own.

Measured, one run on the MI355X machine, the references made first and the tests then run on the warm caches (host seconds are the
references' and their non-vacuity assertions; device seconds are what the tests take once the references exist, the tables' uploads
included):

  group                         cases   host    device   slowest case on the device
  stream, mstream               24      0.27    0.11     0.02   (stream-overlap8-last1-r31-31; every other case below 0.005)
  the four retried routes       76      0.38    0.39     0.01   (the long_regions cases; most others below 0.005)
  attempts beyond 256            4      (in the retried references)   0.22     0.06   (4096 samples of 50 attempts on average)
  padding and guards             6      (references shared)           0.03     below 0.005

The whole module takes 1.31 s there on warm caches, the context's creation (0.23 s) included, and about 4 s when it makes its references
itself.  The device seconds of a group are the sum of its listed cases and 0.004 s for each case pytest lists as below 0.005 s.  The
yardstick, the slowest test of tests/test_gpu_retry_gate_wait.py, took 7.03 s in a run of the whole suite on the same kind of machine
(test_one_round_follows_the_convolution_with_the_wait_noise).
"""
import contextlib
import functools

import numpy as np
import pytest

from quantum_css_codes_amd import _native
from tests import stream_synthetic as syn
from tests import test_stream_synthetic as cpu
from tests.state_check import DirtyBuffer, Layout
from tests.test_gpu_sampler_instantiations import own_time_limit  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

SAMPLES = 4096
R_IDS = lambda r: "r%d-%d" % r


@pytest.fixture(scope="module")
def ctx():
    context = _native.Context(0)
    yield context
    context.close()
    for fn in (cpu.stream_reference, cpu.retry_reference):                      # the references are dropped with the module
        fn.cache_clear()


@contextlib.contextmanager
def handle(made):
    """A device object, freed whatever the test finds."""
    try:
        yield made
    finally:
        made.free()


def stored(ctx, fill, width):
    """The (SAMPLES, width) words `fill(buffer, ldo)` stores."""
    buf = ctx.alloc(SAMPLES * width * 8).zero()
    try:
        fill(buf, width)
        return buf.download((SAMPLES, width), np.uint64)
    finally:
        buf.free()


# ---- stream_kernel and mstream_kernel ------------------------------------------------------------------------------------------------------

def streamed_device(ctx, route, seq):
    return ctx.stream_create(*seq.stream_args()) if route == "stream" else ctx.mstream_create(*seq.mstream_args())


def streamed_store(ctx, route, dev, seq, seed, first):
    fill = ctx.stream_outcomes_dev if route == "stream" else ctx.mstream_outcomes_dev
    return lambda buf, ldo: fill(dev, seed, first, SAMPLES, *seq.p, buf, ldo)


@functools.lru_cache(maxsize=None)
def streamed_counts(route, name, r):
    """{(key 0, records): counts} by the host tallies, non-vacuity asserted."""
    seq, seed, first, faults, words = cpu.stream_reference(route, name, r, SAMPLES)
    accepted = int((~words[:, seq.nsteps:].any(axis=1)).sum())
    cpu.assert_share(name, accepted, SAMPLES)
    cpu.assert_share(name, SAMPLES - accepted, SAMPLES)
    if name == "flags64":
        cpu.assert_flags64_words(seq, words)
    out = {}
    for key0 in syn.KEY0:
        for records in (0, 1) if route == "mstream" else (0,):
            got = out[key0, records] = cpu.tally_host(route, seq, words, syn.decoder(*r, key0), records)
            if route == "stream":
                cpu.assert_decoder_counts(name, got, key0)
            else:
                assert got[2] > 0 and got[3] > 0 and (key0 != "zero" or max(got[2:4]) < got[0]), (name, key0, got)
                assert name != "overlap8-4" or key0 != "zero" or all(v > 0 for v in got[4:]), got
    assert len({tuple(out[key0, 0]) for key0 in syn.KEY0}) == 3
    return out


@pytest.mark.parametrize("r", syn.R_SETS, ids=R_IDS)
@pytest.mark.parametrize("route, name", cpu.STREAM_CASES)
def test_streamed_words_and_counts_equal_the_host_statements(ctx, route, name, r):
    seq, seed, first, faults, words = cpu.stream_reference(route, name, r, SAMPLES)
    want = streamed_counts(route, name, r)
    with handle(streamed_device(ctx, route, seq)) as dev:
        assert np.array_equal(stored(ctx, streamed_store(ctx, route, dev, seq, seed, first), seq.ldw), words), (route, name)
        for (key0, records), counts in want.items():
            tables = syn.decoder(*r, key0)
            if route == "stream":
                got = ctx.mc_stream_decode(dev, *tables, seed, first, SAMPLES, *seq.p)
            else:
                got = ctx.mc_mstream_decode(dev, records, *tables, seed, first, SAMPLES, *seq.p)
            assert got.tolist() == counts, (route, name, key0, records, got.tolist(), counts)


# ---- the four retried kernels --------------------------------------------------------------------------------------------------------------

def retried_device(ctx, route, seq):
    return getattr(ctx, route + "_create")(*cpu.retry_tables(route, seq))


def retried_store(ctx, route, dev, seq, seed, first, limit):
    fill = getattr(ctx, route + "_outcomes_dev")
    return lambda buf, ldo: fill(dev, seed, first, SAMPLES, *cpu.retry_rates(route, seq), limit, buf, ldo)


@functools.lru_cache(maxsize=None)
def retried_counts(route, name, r):
    reference = cpu.retry_reference(route, name, r, SAMPLES)
    seq, words = reference[0], reference[4]
    counts = cpu.host_counts(route, seq, words, syn.decoder(*r))
    cpu.assert_retry_reference(route, name, reference, counts)
    if name == "long_regions":
        cpu.assert_decoder_counts(name, counts, "zero")
    if name == "flags64-2":
        cpu.assert_flags64_words(seq, words)
    return counts


def run_retried(ctx, route, name, r):
    seq, seed, first, limit, words, tries = cpu.retry_reference(route, name, r, SAMPLES)
    want = retried_counts(route, name, r)
    with handle(retried_device(ctx, route, seq)) as dev:
        got = stored(ctx, retried_store(ctx, route, dev, seq, seed, first, limit), words.shape[1])
        assert np.array_equal(got, words), (route, name, r)
        decode = getattr(ctx, "mc_" + route + "_decode")
        counts = decode(dev, *syn.decoder(*r), seed, first, SAMPLES, *cpu.retry_rates(route, seq), limit)
        assert counts.tolist() == want, (route, name, r, counts.tolist(), want)
        if name == "long_regions":                                              # ... and under the tables without key 0 and with key 0 -> flip 1
            for key0 in syn.KEY0[1:]:
                tables = syn.decoder(*r, key0)
                other = cpu.host_counts(route, seq, words, tables)
                cpu.assert_decoder_counts(name, other, key0)
                assert other != want
                assert decode(dev, *tables, seed, first, SAMPLES, *cpu.retry_rates(route, seq), limit).tolist() == other, (route, key0)


RETRY_CASES = [case for case in cpu.RETRY_CASES if case[1] != "attempts"]


@pytest.mark.parametrize("route, name, r", RETRY_CASES, ids=["%s-%s-r%d-%d" % ((route, name) + r) for route, name, r in RETRY_CASES])
def test_retried_words_and_counts_equal_the_host_statements(ctx, route, name, r):
    run_retried(ctx, route, name, r)


@pytest.mark.parametrize("route", cpu.ROUTES)
def test_attempts_beyond_256(ctx, route):
    """One retried region that fails 98 % of its attempts, max_attempts = 65536: some sample needs more than 256 attempts and none is
    exhausted (asserted on the host reference by assert_retry_reference)."""
    run_retried(ctx, route, "attempts", syn.R_SETS[0])


# ---- padding and guards ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ("stream", "mstream") + cpu.ROUTES)
def test_padding_and_guards_keep_the_fill_pattern(ctx, route):
    """A row pitch 3 words wider than needed in a window 8 bytes off 16-byte alignment of a dirty parent: the promised words equal the
    reference, the padding and both guards still hold the fill pattern.  The retried routes run long_regions at max_attempts = 2, where
    the stores of the exhausted path and the attempts word are exercised."""
    r = syn.R_SETS[0]
    if route in ("stream", "mstream"):
        seq, seed, first, faults, words = cpu.stream_reference(route, "overlap8-last1" if route == "stream" else "overlap8-4", r, SAMPLES)
        dev = streamed_device(ctx, route, seq)
        fill = streamed_store(ctx, route, dev, seq, seed, first)
    else:
        seq, seed, first, limit, words, tries = cpu.retry_reference(route, "long_regions-2", r, SAMPLES)
        retried_counts(route, "long_regions-2", r)
        dev = retried_device(ctx, route, seq)
        fill = retried_store(ctx, route, dev, seq, seed, first, limit)
    with handle(dev):
        buf = DirtyBuffer(ctx, Layout(SAMPLES, words.shape[1] + 3, 264))
        try:
            fill(buf.view, words.shape[1] + 3)
            buf.check(words, preserved=True, what="gf2_%s_outcomes_dev" % route)
        finally:
            buf.free()
