#!/usr/bin/env python3
"""The timing of DESIGN.md section 5d "Repeat-until-success of multi-block programs", regenerated on one MI355X in one process.
Whole calls that end with the copy of the counts to the host, so the host clock around a call measures the kernel, its launch and
the per-call tables; the routes of a pair alternate on the same seeds ROUNDS times after a warm-up of either, and the number of
samples is grown until a call takes at least MIN_SECONDS (for the one-qubit pairs a call of either route at one size, so that the
counts can be compared; for Q = 2 and 4 each route at its own size).

  one qubit    gf2_mc_mretry_decode against gf2_mc_retry_decode on the programs MEASURE and XYZIZYX MEASURE: samples per second of
               either and the ratio new / old; the counts of the two are compared as they are timed
  Q = 2, 4     gf2_mc_mretry_decode against the post-selected gf2_mc_mstream_decode on the two programs of profiles/time_mstream.py
               in accepted samples per second, at p_kind = 1e-4 and 1e-3; attempts per preparation beside the exact mean

The lines are appended to profiles/time_mretry.log."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_css_codes_amd import stream_noise  # noqa: E402
from quantum_css_codes_amd.css_code import CSSCode  # noqa: E402
from tests import retry_ref  # noqa: E402

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
ROUNDS, MIN_SECONDS, RATES = 5, 0.5, (1e-4, 1e-3)
ONE_QUBIT = ("", "XYZIZYX")
MULTI = ((('X', 0), ('CNOT', 0, 1), ('MEASURE', 0), ('MEASURE', 1)),
         (('X', 0), ('CNOT', 0, 1), ('CNOT', 2, 3), ('Y', 3), ('CNOT', 1, 2), ('MEASURE', 3), ('MEASURE', 0)))


def timed(call):
    start = time.perf_counter()
    counts = call()
    return time.perf_counter() - start, counts


def grown(*calls):
    """The smallest power-of-two sample count from 2^20 on at which every call(samples) takes MIN_SECONDS (at most 2^32)."""
    samples = 1 << 20
    while samples < 1 << 32 and min(timed(lambda: call(samples))[0] for call in calls) < MIN_SECONDS:
        samples *= 2
    return samples


def spread(values):
    return "%.4g (min %.4g max %.4g)" % (statistics.median(values), min(values), max(values))


def main():
    log = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "time_mretry.log"), "a")

    def say(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    code = CSSCode(STEANE, STEANE)
    say("steane, p_x = p_y = p_z = p, max_attempts = 256, %d alternated rounds per pair, at least %.1f s per call" % (ROUNDS, MIN_SECONDS))
    for ops in ONE_QUBIT:
        one = stream_noise.stream_for(code, "program", tuple(ops))
        multi = stream_noise.multi_program_for(code, [(op, 0) for op in ops] + [('MEASURE', 0)])
        for p in RATES:
            old = lambda n, seed=0: one.retry_counts(n, p, p, p, seed=seed)
            new = lambda n, seed=0: multi.retry_counts(n, p, p, p, seed=seed)
            samples = grown(old, new)
            times = {"retry": [], "mretry": []}
            for r in range(ROUNDS):
                t_old, c_old = timed(lambda: old(samples, r))
                t_new, c_new = timed(lambda: new(samples, r))
                assert [int(c_new[k]) for k in (0, 2, 3, 4, 5, 6, 7, 20, 21)] == [int(c_old[k]) for k in (0, 6, 7, 8, 9, 10, 11, 12, 13)]
                times["retry"].append(samples / t_old)
                times["mretry"].append(samples / t_new)
            say("one qubit %r MEASURE, p = %g: L = %d, %d preparations, N = 2^%d, accepted %.6f, attempts per preparation %.4f; samples/s: "
                "gf2_mc_retry_decode %s, gf2_mc_mretry_decode %s; ratio of medians new / old = %.3f"
                % (ops, p, multi.num_locations, multi.preparations, samples.bit_length() - 1, int(c_new[0]) / samples,
                   int(c_new[21]) / samples / multi.preparations, spread(times["retry"]), spread(times["mretry"]),
                   statistics.median(times["mretry"]) / statistics.median(times["retry"])))
    for instructions in MULTI:
        multi = stream_noise.multi_program_for(code, instructions)
        for p in RATES:
            exact = retry_ref.attempts_mean_var(multi, (p, p, p))[0] / multi.preparations
            old = lambda n, seed=0: multi.counts(n, p, p, p, seed=seed)
            new = lambda n, seed=0: multi.retry_counts(n, p, p, p, seed=seed)
            n_old, n_new = grown(old), grown(new)                               # each route at its own size: a call of either takes MIN_SECONDS
            rates = {"mstream": [], "mretry": [], "mretry samples": []}
            for r in range(ROUNDS):
                t_old, c_old = timed(lambda: old(n_old, r))
                t_new, c_new = timed(lambda: new(n_new, r))
                rates["mstream"].append(int(c_old[0]) / t_old)
                rates["mretry"].append(int(c_new[0]) / t_new)
                rates["mretry samples"].append(n_new / t_new)
            slow = statistics.median(rates["mstream"])
            say("Q = %d, %d blocks, L = %d, %d preparations, p = %g, records = reference: post-selected N = 2^%d accepts %.3g, retried N = 2^%d accepts "
                "%.6f (exhausted %d); attempts per preparation %.4f (exact mean %.4f); accepted samples/s: gf2_mc_mstream_decode %s, "
                "gf2_mc_mretry_decode %s, ratio of medians %s; location-draws/s of the retried route, first attempts only %.4g"
                % (multi.nframes, len(multi.block_type), multi.num_locations, multi.preparations, p, n_old.bit_length() - 1, int(c_old[0]) / n_old,
                   n_new.bit_length() - 1, int(c_new[0]) / n_new, int(c_new[20]), int(c_new[21]) / n_new / multi.preparations, exact,
                   spread(rates["mstream"]), spread(rates["mretry"]), "%.3g" % (statistics.median(rates["mretry"]) / slow) if slow else "inf",
                   statistics.median(rates["mretry samples"]) * multi.num_locations))
    log.close()


if __name__ == "__main__":
    main()
