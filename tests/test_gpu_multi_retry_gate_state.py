"""
State between calls for the repeat-until-success sampler of multi-block programs under gate-level faults
(gf2_mretry_gate_outcomes_dev, gf2_mc_mretry_gate_decode), in the style of tests/test_gpu_multi_retry_state.py with the dirty buffers
of tests/state_check.py: the words are stored into a window of a dirty parent at an aligned and at an odd 8-byte offset, with a row
pitch wider than the words -- every promised word equals the host statement, the padding and both guards keep the fill pattern
exactly ("left as they were"), also with two attempts, where exhausted samples store their flags -- and neither entry point's result
depends on what earlier calls left in the context's workspace or on the order of the calls.
"""
import numpy as np
import pytest

from quantum_css_codes_amd import _native, stream_noise
from tests.state_check import DirtyBuffer, Layout
from tests.test_gpu_stream import make_code
from tests.test_multi_retry_gate import host_counts

pytestmark = pytest.mark.gpu

PROGRAM = (('X', 0), ('CNOT', 0, 1), ('MEASURE', 0), ('MEASURE', 1))
P = (2e-3, 3e-3)


@pytest.fixture
def fresh():
    """A context of its own (fresh workspace slots), closed at the end of the case."""
    context = _native.Context(0)
    yield context
    context.close()


@pytest.mark.parametrize("limit", [256, 2])
@pytest.mark.parametrize("lead", [256, 264])
def test_outputs_words_padding_preserved(fresh, lead, limit):
    prog = stream_noise.MultiProgram(make_code("steane"), PROGRAM)
    count = 300
    want, _ = prog.retry_gate_words_host(count, *P, seed=9, first_sample=1000, max_attempts=limit)
    assert want[:, :prog.nsteps].any() and want[:, prog.nsteps:prog.ldw].any() == (limit == 2)
    handle = fresh.mretry_gate_create(*prog._retry_gate_sequence())
    for pad in (0, 3):
        buf = DirtyBuffer(fresh, Layout(count, prog.ldw + 1 + pad, lead))
        fresh.mretry_gate_outcomes_dev(handle, 9, 1000, count, *P, limit, buf.view, prog.ldw + 1 + pad)
        buf.check(want, preserved=True, what="gf2_mretry_gate_outcomes_dev, pitch + %d, %d attempts" % (pad, limit))
        buf.free()
    handle.free()


def test_results_do_not_depend_on_earlier_calls(fresh):
    prog = stream_noise.MultiProgram(make_code("steane"), PROGRAM)
    handle = fresh.mretry_gate_create(*prog._retry_gate_sequence())
    tables = prog._tables()
    count = 3000
    words, _ = prog.retry_gate_words_host(count, *P, seed=4, first_sample=17, max_attempts=2)
    want = {records: host_counts(prog, words, records) for records in stream_noise.RECORDS}
    assert want['reference'][0] >= 100 and want['reference'][20] >= 100

    def decode(records):
        return fresh.mc_mretry_gate_decode(handle, stream_noise.RECORDS[records], *tables, 4, 17, count, *P, 2).tolist()

    def outcomes():
        buf = fresh.alloc(count * (prog.ldw + 1) * 8)
        try:
            fresh.mretry_gate_outcomes_dev(handle, 4, 17, count, *P, 2, buf, prog.ldw + 1)
            return buf.download((count, prog.ldw + 1), np.uint64)
        finally:
            buf.free()

    assert decode('reference') == want['reference']
    fresh.fill_workspace(0xFF)                                          # whatever the workspace holds, the counts are the same
    assert decode('propagated') == want['propagated']
    assert np.array_equal(outcomes(), words)
    fresh.mc_mretry_gate_decode(handle, 1, *tables, 5, 0, 20000, 4e-3, 1e-3, 256)     # a larger call with other rates and attempts in between
    fresh.fill_workspace(0x00)
    assert decode('reference') == want['reference'] and decode('propagated') == want['propagated']
    assert np.array_equal(outcomes(), words)
    handle.free()
