#!/usr/bin/env python3
"""The timing of DESIGN.md section 5d "Multi-block programs", regenerated on one MI355X in one process: accepted samples per second of
the multi-block tally (gf2_mc_mstream_decode) on one-qubit programs against the streamed tally (gf2_mc_stream_decode) on the same
programs, the same seeds and the same rates, the two calls alternated ROUNDS times after a warm-up of either; then the multi-block
tally on a two-qubit and a four-qubit program, also per location-draw (samples x L per second), under both settings of `records`.
A call ends with the copy of its counts to the host, so the host clock around it measures the kernel and its launch; the number of
samples is grown until a call takes at least MIN_SECONDS.  The counts of the two routes are compared as they are timed.  The lines
are appended to profiles/time_mstream.log."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_css_codes_amd import stream_noise  # noqa: E402
from quantum_css_codes_amd.css_code import CSSCode  # noqa: E402

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
ROUNDS, MIN_SECONDS, P = 5, 0.5, 1e-4
ONE_QUBIT = ("", "XYZIZYX")
MULTI = ((('X', 0), ('CNOT', 0, 1), ('MEASURE', 0), ('MEASURE', 1)),
         (('X', 0), ('CNOT', 0, 1), ('CNOT', 2, 3), ('Y', 3), ('CNOT', 1, 2), ('MEASURE', 3), ('MEASURE', 0)))


def timed(call):
    start = time.perf_counter()
    counts = call()
    return time.perf_counter() - start, counts


def grown(call):
    """The smallest power-of-two sample count from 2^22 on at which call(samples) takes MIN_SECONDS (at most 2^32)."""
    samples = 1 << 22
    while samples < 1 << 32 and timed(lambda: call(samples))[0] < MIN_SECONDS:
        samples *= 2
    return samples


def main():
    log = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "time_mstream.log"), "a")

    def say(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    code = CSSCode(STEANE, STEANE)
    say("steane, p_x = p_y = p_z = %g, %d alternated rounds per pair, at least %.1f s per call" % (P, ROUNDS, MIN_SECONDS))
    for ops in ONE_QUBIT:
        one = stream_noise.stream_for(code, "program", tuple(ops))
        multi = stream_noise.multi_program_for(code, [(op, 0) for op in ops] + [('MEASURE', 0)])
        old = lambda n, seed=0: one.counts(n, P, P, P, seed=seed)
        new = lambda n, seed=0: multi.counts(n, P, P, P, seed=seed)
        samples = grown(old)
        new(samples)                                                    # warm-up of the other route at the timed size
        times = {"stream": [], "mstream": []}
        for r in range(ROUNDS):
            t_old, c_old = timed(lambda: old(samples, r))
            t_new, c_new = timed(lambda: new(samples, r))
            assert [int(c_new[k]) for k in (0, 2, 3, 4, 5, 6, 7)] == [int(c_old[k]) for k in (0, 6, 7, 8, 9, 10, 11)]
            times["stream"].append(int(c_old[0]) / t_old)
            times["mstream"].append(int(c_new[0]) / t_new)
        med = {k: statistics.median(v) for k, v in times.items()}
        say("one qubit %r MEASURE: L = %d, N = 2^%d, accepted %.4f; accepted samples/s: gf2_mc_stream_decode %.4g (min %.4g max %.4g), "
            "gf2_mc_mstream_decode %.4g (min %.4g max %.4g); ratio of medians new / old = %.3f"
            % (ops, multi.num_locations, samples.bit_length() - 1, int(c_new[0]) / samples, med["stream"], min(times["stream"]), max(times["stream"]),
               med["mstream"], min(times["mstream"]), max(times["mstream"]), med["mstream"] / med["stream"]))
    for instructions in MULTI:
        multi = stream_noise.multi_program_for(code, instructions)
        samples = grown(lambda n: multi.counts(n, P, P, P))
        for records in ('reference', 'propagated'):
            rates = []
            for r in range(ROUNDS):
                t, c = timed(lambda: multi.counts(samples, P, P, P, seed=r, records=records))
                rates.append((samples / t, int(c[0]) / t))
            say("Q = %d, %d blocks, L = %d, N = 2^%d, records = %s: accepted %.4f; samples/s %.4g, accepted samples/s %.4g, location-draws/s %.4g (medians of %d)"
                % (multi.nframes, len(multi.block_type), multi.num_locations, samples.bit_length() - 1, records, int(c[0]) / samples,
                   statistics.median(x for x, _ in rates), statistics.median(y for _, y in rates),
                   statistics.median(x for x, _ in rates) * multi.num_locations, ROUNDS))
    log.close()


if __name__ == "__main__":
    main()
