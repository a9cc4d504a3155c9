"""
State between calls for the multi-block streamed route (gf2_mstream_outcomes_dev, gf2_mc_mstream_decode), in the style of
tests/test_gpu_state.py with the dirty buffers of tests/state_check.py: the words are stored into a window of a dirty parent at an
aligned and at an odd 8-byte offset, with a row pitch wider than the words -- every promised word equals the host statement, the
padding and both guards keep the fill pattern exactly ("left as they were") -- and neither entry point's result depends on what
earlier calls left in the context's workspace or on the order of the calls.
"""
import numpy as np
import pytest

from quantum_css_codes_amd import _native, stream_noise
from tests import stream_ref
from tests.state_check import DirtyBuffer, Layout
from tests.test_gpu_stream import make_code

pytestmark = pytest.mark.gpu

PROGRAM = (('X', 0), ('CNOT', 0, 1), ('MEASURE', 0), ('MEASURE', 1))
P = (3e-4, 1.5e-4, 3e-4)


@pytest.fixture
def fresh():
    """A context of its own (fresh workspace slots), closed at the end of the case."""
    context = _native.Context(0)
    yield context
    context.close()


@pytest.mark.parametrize("lead", [256, 264])
def test_outputs_words_padding_preserved(fresh, lead):
    prog = stream_noise.MultiProgram(make_code("steane"), PROGRAM)
    count = 300
    want = prog.words_of_faults(*stream_ref.sampled_faults(prog.num_locations, 9, 1000, count, P))
    assert want[:, :prog.nsteps].any() and want[:, prog.nsteps:].any()
    handle = fresh.mstream_create(*prog._sequence())
    for pad in (0, 3):
        buf = DirtyBuffer(fresh, Layout(count, prog.ldw + pad, lead))
        fresh.mstream_outcomes_dev(handle, 9, 1000, count, *P, buf.view, prog.ldw + pad)
        buf.check(want, preserved=True, what="gf2_mstream_outcomes_dev, pitch + %d" % pad)
        buf.free()
    handle.free()


def test_results_do_not_depend_on_earlier_calls(fresh):
    prog = stream_noise.MultiProgram(make_code("steane"), PROGRAM)
    handle = fresh.mstream_create(*prog._sequence())
    tables = prog._tables()
    count = 3000
    words = prog.words_of_faults(*stream_ref.sampled_faults(prog.num_locations, 4, 17, count, P))
    want = {records: prog.tally_host(words, records=records, fields=True).tolist() for records in stream_noise.RECORDS}
    assert want['reference'][0] >= 100

    def decode(records):
        return fresh.mc_mstream_decode(handle, stream_noise.RECORDS[records], *tables, 4, 17, count, *P).tolist()

    assert decode('reference') == want['reference']
    fresh.fill_workspace(0xFF)                                          # whatever the workspace holds, the counts are the same
    assert decode('propagated') == want['propagated']
    assert np.array_equal(fresh.outcomes(fresh.mstream_outcomes_dev, handle, 4, 17, count, *P, prog.ldw), words)
    fresh.mc_mstream_decode(handle, 1, *tables, 5, 0, 20000, 1e-3, 1e-3, 1e-3)     # a larger call with other rates in between
    fresh.fill_workspace(0x00)
    assert decode('reference') == want['reference'] and decode('propagated') == want['propagated']
    handle.free()
