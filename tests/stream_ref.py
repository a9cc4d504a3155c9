"""
What the tests of the streamed route (DESIGN.md section 5d "Streamed gadgets") compare against, sharing nothing with
quantum_css_codes_amd/stream_noise.py or the native library's streamed code:

  sampled_faults    the faults of the oracle's sampler run over L locations (c_oracle.sample_errors with n := L) as a fault list
                    per sample -- what gf2_stream_words_host takes -- read from the packed words without unpacking 2^20 columns
  dense_faults      the same faults as the (L, samples) vectors tests/ec_ref.py and tests/ft_ref.py propagate
  Reference         a restated gadget (ec_ref.Cycle or ft_ref.Rewritten) seen through the stream layout: its outcome words permuted
                    into [steps] [flag words], its tally as the dict StreamedGadget.error_rates returns
"""
import numpy as np

from oracle import c_oracle
from tests import ec_ref, ft_ref

_BITS = np.arange(64, dtype=np.uint64)


def sampled_faults(locations, seed, first, count, p):
    """(fault_first (count + 1), fault_location, fault_kind): sample i has the faults fault_first[i] .. fault_first[i + 1] - 1, in
    ascending location order, kind 1 (X), 2 (Z) or 3 (Y)."""
    if count == 0:
        return np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint8)
    e_x, e_z = c_oracle.sample_errors(locations, seed, first, count, *p)
    sample, word = np.nonzero(e_x | e_z)                               # row-major: samples ascend, words ascend within a sample
    kinds = ((e_x[sample, word][:, None] >> _BITS) & np.uint64(1)) + 2 * ((e_z[sample, word][:, None] >> _BITS) & np.uint64(1))
    hit, bit = np.nonzero(kinds)
    fault_first = np.concatenate([[0], np.cumsum(np.bincount(sample[hit], minlength=count))]).astype(np.int64)
    return fault_first, (64 * word[hit] + bit).astype(np.int32), kinds[hit, bit].astype(np.uint8)


def dense_faults(locations, fault_first, fault_location, fault_kind):
    """(f_x, f_z), each (L, samples) uint8."""
    count = len(fault_first) - 1
    sample = np.repeat(np.arange(count), np.diff(fault_first))
    f_x = np.zeros((locations, count), dtype=np.uint8)
    f_z = np.zeros((locations, count), dtype=np.uint8)
    f_x[fault_location, sample] = fault_kind & 1
    f_z[fault_location, sample] = fault_kind >> 1
    return f_x, f_z


class Reference(object):
    """An ec_ref.Cycle (cycle=True) or an ft_ref.Rewritten behind the stream layout."""

    def __init__(self, gadget, cycle):
        self.gadget, self.cycle = gadget, cycle
        self.locations, self.ldw = gadget.locations, gadget.ldr
        self.nsteps = gadget.rounds + 1 if cycle else gadget.nsteps

    def to_stream_layout(self, words):
        """ec_ref's [final frame] [round 1 .. rounds] [flag words] as [round 1 .. rounds] [final frame] [flag words]; ft_ref's layout
        is the stream layout already."""
        if not self.cycle:
            return words
        rounds = self.gadget.rounds
        return np.ascontiguousarray(words[..., list(range(1, rounds + 1)) + [0] + list(range(rounds + 1, self.ldw))])

    def from_stream_layout(self, words):
        if not self.cycle:
            return words
        rounds = self.gadget.rounds
        return np.ascontiguousarray(words[..., [rounds] + list(range(rounds)) + list(range(rounds + 1, self.ldw))])

    def effect_words(self):
        from tests import gadget_enumerate_ref
        return self.to_stream_layout(gadget_enumerate_ref.effect_words(self.gadget))

    def words(self, seed, first, count, p, chunk=16384):
        """The stream-layout words of samples [first, first + count) under the oracle's sampler."""
        parts = []
        for start in range(0, count, chunk):
            faults = sampled_faults(self.locations, seed, first + start, min(chunk, count - start), p)
            parts.append(self.gadget.outcome_words(*dense_faults(self.locations, *faults)))
        words = np.concatenate(parts) if parts else np.zeros((0, self.ldw), dtype=np.uint64)
        return self.to_stream_layout(words)

    def tally(self, words):
        """The dict StreamedGadget.error_rates returns, from ec_ref.tally / ft_ref.tally on the restated layout."""
        counts, _ = self.gadget.tally(self.from_stream_layout(np.asarray(words)))
        out = {name: int(v) for name, v in zip(ec_ref.FIELDS if self.cycle else ft_ref.FIELDS, counts)}
        out['samples'] = len(words)
        return out


def cycle_reference(code, rounds, idle_data=False):
    return Reference(ec_ref.Cycle(code, rounds, idle_data), True)


def program_reference(code, ops):
    return Reference(ft_ref.Rewritten(code, ops), False)
