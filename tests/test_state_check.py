"""
The dirty-buffer helper of test_gpu_state.py judged on made-up results, without a GPU: every kind of wrong result the GPU tests
are there to catch must be rejected, and a right one accepted.  NumPy arrays stand in for the downloaded parents.
"""
import ctypes

import numpy as np
import pytest

from quantum_css_codes_amd import _native
from tests import state_check
from tests.state_check import FILL, Layout


@pytest.fixture(params=[256, 264], ids=["aligned", "offset-264"])
def case(request):
    """A 5 x 4 output of which the first 3 words of every row are promised, as a right result would leave it."""
    rng = np.random.default_rng(1)
    layout = Layout(5, 4, lead=request.param)
    want = rng.integers(0, 1 << 63, (5, 3), dtype=np.uint64)
    want[2] = 0                                              # an all-zero row: must be STORED, not skipped
    image = layout.image()
    layout.payload(image)[:, :3] = want
    return layout, want, image


def test_a_right_result_passes(case):
    layout, want, image = case
    got = layout.check(image, want)
    assert np.array_equal(got[:, :3], want) and (got[:, 3] == FILL).all()
    layout.check(image, want, preserved=True)
    zeroed = image.copy()
    layout.payload(zeroed)[1, 3] = 0                         # padding zeroed: allowed unless the header says "left as they were"
    layout.check(zeroed, want)
    with pytest.raises(AssertionError, match="outside the promised ones"):
        layout.check(zeroed, want, preserved=True)


def test_a_promised_word_left_at_the_fill_pattern_is_rejected(case):
    layout, want, image = case
    for (r, c) in ((0, 0), (2, 1), (4, 2)):                  # (2, 1): the zero row's store skipped
        bad = image.copy()
        layout.payload(bad)[r, c] = FILL
        with pytest.raises(AssertionError, match="row %d word %d still holds the fill pattern" % (r, c)):
            layout.check(bad, want)


def test_a_wrong_promised_word_is_rejected(case):
    layout, want, image = case
    bad = image.copy()
    layout.payload(bad)[3, 1] ^= np.uint64(1 << 40)
    with pytest.raises(AssertionError, match="1 promised word"):
        layout.check(bad, want)


def test_a_changed_guard_word_is_rejected(case):
    layout, want, image = case
    for at in (0, layout.lead_words - 1, layout.lead_words + layout.words, layout.total_words - 1):
        bad = image.copy()
        bad[at] = 0
        with pytest.raises(AssertionError, match="guard"):
            layout.check(bad, want)
        with pytest.raises(AssertionError, match="guard"):
            layout.check_accumulated(bad, np.zeros(20), np.zeros(20))


def test_a_padding_word_that_is_neither_fill_nor_zero_is_rejected(case):
    layout, want, image = case
    bad = image.copy()
    layout.payload(bad)[4, 3] = 1
    with pytest.raises(AssertionError, match="neither the fill pattern nor zero"):
        layout.check(bad, want)


def test_a_mask_of_promised_words(case):
    # entries the header leaves open (pivots past the rank): only the masked words are compared, the rest is padding
    layout, want, image = case
    full = np.zeros((5, 4), dtype=np.uint64)
    full[:, :3] = want
    mask = np.zeros((5, 4), dtype=bool)
    mask[:, :2] = True
    with pytest.raises(AssertionError, match="outside the promised ones"):
        layout.check(image, full, promised=mask)             # column 2 holds data: neither fill nor zero
    mask[:, :3] = True
    layout.check(image, full, promised=mask)


def test_histograms_must_be_added_to(case):
    layout = Layout(1, 40, lead=case[0].lead)
    prefill = state_check.ramp(40)
    assert prefill.all() and (np.diff(prefill.astype(np.int64)) != 0).all()
    counts = np.arange(40, dtype=np.uint64) % np.uint64(5)   # some bins stay empty
    right = layout.image(prefill + np.uint64(2) * counts)
    layout.check_accumulated(right, prefill, counts, times=2)
    overwritten = layout.image(counts)                       # = in place of +=, seen after the second call
    with pytest.raises(AssertionError, match="overwrote"):
        layout.check_accumulated(overwritten, prefill, counts, times=2)
    cleared = layout.image(np.uint64(2) * counts)            # the kernel cleared the bins first
    with pytest.raises(AssertionError, match="cleared"):
        layout.check_accumulated(cleared, prefill, counts, times=2)
    once = layout.image(prefill + counts)                    # the second call's counts replaced the first's
    with pytest.raises(AssertionError, match="overwrote"):
        layout.check_accumulated(once, prefill, counts, times=2)
    off = right.copy()
    layout.payload(off)[0, 7] += np.uint64(1)
    with pytest.raises(AssertionError, match="bin 7"):
        layout.check_accumulated(off, prefill, counts, times=2)


def test_layout_refuses_a_short_guard():
    with pytest.raises(ValueError):
        Layout(1, 1, lead=248)
    with pytest.raises(ValueError):
        Layout(1, 1, lead=260)


def test_argument_checks_that_need_no_device():
    # gf2_ctx_fill_workspace refuses a null context; the entry points that take the tiled layout, and the blocked eliminations,
    # refuse a pointer that is not 16-byte aligned before they look at anything else (no pointer here is ever dereferenced)
    lib = _native.lib()
    sizes = (ctypes.c_int64 * 4)()
    assert lib.gf2_ctx_fill_workspace(None, 0, sizes) == _native.GF2_E_ARG and b"null context" in lib.gf2_last_error()
    assert lib.gf2_retile_dev(None, 4096, 1, 2, 70, 4096 + 8) == _native.GF2_E_ARG and b"16-byte aligned" in lib.gf2_last_error()
    assert lib.gf2_retile_dev(None, 4096, 1, 2, 70, 8192) == _native.GF2_E_ARG and b"null context" in lib.gf2_last_error()
    assert lib.gf2_syndrome_dev(None, None, 4096 + 8, 1, 0, _native.LAYOUT_TILED, 8192, 1) == _native.GF2_E_ARG
    assert b"16-byte aligned" in lib.gf2_last_error()
    assert lib.gf2_syndrome_dev(None, None, 4096 + 8, 1, 2, _native.LAYOUT_SAMPLE_MAJOR, 8192, 1) == _native.GF2_E_ARG
    assert b"null argument" in lib.gf2_last_error()          # (sample-major errors may sit at any 8-byte-aligned address)
    for ex, ez in ((4096 + 8, 8192), (4096, 8192 + 8)):
        assert lib.gf2_sample_errors_dev(None, 70, 1, 0, 1, 0.1, 0.1, 0.1, ex, ez, 0, _native.LAYOUT_TILED) == _native.GF2_E_ARG
        assert b"16-byte aligned" in lib.gf2_last_error()
    assert lib.gf2_rref_batch_dev(None, 4096 + 8, 1, 300, 600, 10, None, 8192) == _native.GF2_E_ARG
    assert b"16-byte aligned" in lib.gf2_last_error()
    assert lib.gf2_rref_batch_dev(None, 4096 + 8, 1, 64, 1024, 16, None, 8192) == _native.GF2_E_ARG
    assert b"null context" in lib.gf2_last_error()           # (the small-matrix kernels take any 8-byte-aligned address)
    assert lib.gf2_normalize_dev(None, 4096 + 8, 3, 7, 1, 0, None, 8192, 8192) == _native.GF2_E_ARG
    assert b"16-byte aligned" in lib.gf2_last_error()
