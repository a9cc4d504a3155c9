"""
Dirty device buffers for the tests of state between calls (test_gpu_state.py).

An output buffer handed to the library is a window of a larger parent: a guard of at least 256 bytes, the payload, and a
guard of 256 bytes again, all of it filled with 0xA5A5A5A5A5A5A5A5 before the call.  After the call the whole parent comes back
to the host and `Layout` judges it:
  * every word the header promises is written equals the reference,
  * both guards still hold the fill pattern (nothing was written outside the buffer),
  * every other word of the payload (pitch padding, entries the header leaves open) is the fill pattern or zero -- or exactly
    the fill pattern where the header says "left as they were".
Histograms are accumulated into: the payload starts as a known non-zero ramp and must end as ramp + times * counts.

The judgement works on NumPy arrays alone (test_state_check.py feeds it made-up results without a GPU); `DirtyBuffer` is the
few lines that put the parent on a device through quantum_css_codes_amd._native.
"""
import numpy as np

FILL = np.uint64(0xA5A5A5A5A5A5A5A5)
GUARD_BYTES = 256


class Layout(object):
    """A payload of `rows` x `pitch` 64-bit words at byte offset `lead` (>= 256, a multiple of 8) of its parent."""

    def __init__(self, rows, pitch, lead=GUARD_BYTES):
        if lead < GUARD_BYTES or lead % 8 or rows < 1 or pitch < 1:
            raise ValueError("bad layout")
        self.rows, self.pitch, self.lead = int(rows), int(pitch), int(lead)
        self.lead_words = self.lead // 8
        self.words = self.rows * self.pitch
        self.total_words = self.lead_words + self.words + GUARD_BYTES // 8

    @property
    def nbytes(self):
        return self.words * 8

    @property
    def total_bytes(self):
        return self.total_words * 8

    def image(self, prefill=None):
        """The parent's contents before the call: the fill pattern everywhere, `prefill` (rows x pitch) in the payload if given."""
        img = np.full(self.total_words, FILL, dtype=np.uint64)
        if prefill is not None:
            img[self.lead_words:self.lead_words + self.words] = np.asarray(prefill, dtype=np.uint64).reshape(self.words)
        return img

    def payload(self, image, what="buffer"):
        """The payload (rows x pitch) of a parent that came back, after checking both guards."""
        image = np.asarray(image, dtype=np.uint64)
        assert image.shape == (self.total_words,), "%s: the parent has %s words, not %d" % (what, image.shape, self.total_words)
        front, back = image[:self.lead_words], image[self.lead_words + self.words:]
        assert (front == FILL).all(), "%s: %d word(s) of the guard in front of the buffer were written (first at word %d)" % (
            what, int((front != FILL).sum()), int(np.flatnonzero(front != FILL)[0]) - self.lead_words)
        assert (back == FILL).all(), "%s: %d word(s) of the guard behind the buffer were written (first at word %d past the end)" % (
            what, int((back != FILL).sum()), int(np.flatnonzero(back != FILL)[0]))
        return image[self.lead_words:self.lead_words + self.words].reshape(self.rows, self.pitch)

    def check(self, image, want, promised=None, preserved=False, what="buffer"):
        """Judges an output buffer.  want: the reference, rows x w with w <= pitch (the promised words are the first w of every
        row) or, with `promised` (a boolean rows x pitch mask), a rows x pitch array of which only the masked words count.
        preserved: the other words must hold the fill pattern exactly ("left as they were"), else the fill pattern or zero."""
        got = self.payload(image, what)
        want = np.asarray(want, dtype=np.uint64)
        if promised is None:
            assert want.ndim == 2 and want.shape[0] == self.rows and want.shape[1] <= self.pitch, (want.shape, self.rows, self.pitch)
            promised = np.zeros((self.rows, self.pitch), dtype=bool)
            promised[:, :want.shape[1]] = True
            full = np.zeros((self.rows, self.pitch), dtype=np.uint64)
            full[:, :want.shape[1]] = want
            want = full
        promised = np.asarray(promised, dtype=bool)
        assert want.shape == got.shape == promised.shape
        wrong = promised & (got != want)
        if wrong.any():
            r, c = [int(v[0]) for v in np.nonzero(wrong)]
            state = "still holds the fill pattern (never written)" if got[r, c] == FILL else "is 0x%016x" % int(got[r, c])
            raise AssertionError("%s: %d promised word(s) differ from the reference; row %d word %d %s, expected 0x%016x" % (
                what, int(wrong.sum()), r, c, state, int(want[r, c])))
        rest = got[~promised]
        ok = (rest == FILL) if preserved else ((rest == FILL) | (rest == 0))
        assert ok.all(), "%s: %d word(s) outside the promised ones hold neither %s (first: 0x%016x)" % (
            what, int((~ok).sum()), "the fill pattern" if preserved else "the fill pattern nor zero", int(rest[~ok][0]))
        return got

    def check_accumulated(self, image, prefill, counts, times=1, what="histogram"):
        """Judges bins that were accumulated into `times` times: payload == prefill + times * counts, bin by bin."""
        got = self.payload(image, what).reshape(self.words)
        prefill = np.asarray(prefill, dtype=np.uint64).reshape(self.words)
        counts = np.asarray(counts, dtype=np.uint64).reshape(self.words)
        want = prefill + np.uint64(times) * counts
        if np.array_equal(got, want):
            return got
        if np.array_equal(got, np.uint64(times) * counts):
            how = "the bins were cleared before they were counted into"
        elif np.array_equal(got, counts) or np.array_equal(got, prefill + counts):
            how = "the last call overwrote the bins instead of adding to them"
        else:
            how = "first at bin %d: got %d, expected %d + %d x %d" % (
                int(np.flatnonzero(got != want)[0]), int(got[got != want][0]), int(prefill[got != want][0]), times, int(counts[got != want][0]))
        raise AssertionError("%s: not prefill + %d x counts: %s" % (what, times, how))


def ramp(bins):
    """A known non-zero prefill for `bins` histogram bins: no bin zero, no two neighbours equal."""
    return (np.arange(bins, dtype=np.uint64) * np.uint64(3) + np.uint64(7)) % np.uint64(1009) + np.uint64(1)


class DirtyBuffer(object):
    """A Layout's parent on the device of `ctx` (a _native.Context): .view is what the library gets, .fetch() what comes back."""

    def __init__(self, ctx, layout, prefill=None):
        self.layout = layout
        self.parent = ctx.alloc(layout.total_bytes).upload(layout.image(prefill))
        self.view = self.parent.view(layout.lead, layout.nbytes)

    def fetch(self):
        return self.parent.download((self.layout.total_words,), np.uint64)

    def check(self, want, **kwargs):
        return self.layout.check(self.fetch(), want, **kwargs)

    def check_accumulated(self, prefill, counts, **kwargs):
        return self.layout.check_accumulated(self.fetch(), prefill, counts, **kwargs)

    def free(self):
        self.parent.free()


def dirty_input(ctx, array, lead=GUARD_BYTES):
    """An input array (uint64 words) uploaded at byte offset `lead` of a dirty parent: the view to hand to the library, and
    the parent (to free)."""
    array = np.ascontiguousarray(array, dtype=np.uint64)
    layout = Layout(1, max(1, array.size), lead)
    buf = DirtyBuffer(ctx, layout, prefill=array.reshape(-1) if array.size else None)
    return buf.view, buf
