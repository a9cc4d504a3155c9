#!/usr/bin/env python3
"""The timing of DESIGN.md section 5d "Repeat-until-success of multi-block programs under gate-level faults", regenerated on one
MI355X in one process.  Whole calls that end with the copy of the counts to the host, as profiles/time_mretry.py times them: the
routes of a pair alternate on the same seeds ROUNDS times after a warm-up of either, and the number of samples is grown until a call
of either route takes at least MIN_SECONDS.

  (i)  one qubit   gf2_mc_mretry_gate_decode against gf2_mc_retry_gate_decode on the programs MEASURE and XYZIZYX MEASURE at p_1 = p_2 =
                   p: samples per second of either and the ratio new / old; the counts of the two are compared as they are timed
  (ii) Q = 2, 4    gf2_mc_mretry_gate_decode at p_1 = p_2 = 1e-3 per gate against gf2_mc_mretry_decode at p_kind = 2.303e-4 per
                   location on the two programs of profiles/time_mretry.py: the pairing of profiles/time_retry_gate.py, which gives
                   both routes the same expected number of faults per sample; samples per second and the ratio gates / locations

The lines are appended to profiles/time_mretry_gate.log."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_css_codes_amd import stream_noise  # noqa: E402
from quantum_css_codes_amd.css_code import CSSCode  # noqa: E402

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
ROUNDS, MIN_SECONDS, RATES = 5, 0.5, (1e-4, 1e-3)
P_GATE, P_KIND = 1e-3, 2.303e-4
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
    log = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "time_mretry_gate.log"), "a")

    def say(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    code = CSSCode(STEANE, STEANE)
    say("steane, max_attempts = 256, %d alternated rounds per pair, at least %.1f s per call" % (ROUNDS, MIN_SECONDS))
    for ops in ONE_QUBIT:
        one = stream_noise.stream_for(code, "program", tuple(ops))
        multi = stream_noise.multi_program_for(code, [(op, 0) for op in ops] + [('MEASURE', 0)])
        for p in RATES:
            old = lambda n, seed=0: one.retry_gate_counts(n, p, p, seed=seed)
            new = lambda n, seed=0: multi.retry_gate_counts(n, p, p, seed=seed)
            samples = grown(old, new)
            times = {"old": [], "new": []}
            for r in range(ROUNDS):
                t_old, c_old = timed(lambda: old(samples, r))
                t_new, c_new = timed(lambda: new(samples, r))
                assert [int(c_new[k]) for k in (0, 2, 3, 4, 5, 6, 7, 20, 21)] == [int(c_old[k]) for k in (0, 6, 7, 8, 9, 10, 11, 12, 13)]
                times["old"].append(samples / t_old)
                times["new"].append(samples / t_new)
            say("(i) one qubit %r MEASURE, p_1 = p_2 = %g: L = %d, %d sites, %d preparations, N = 2^%d, accepted %.6f, attempts per preparation "
                "%.4f; samples/s: gf2_mc_retry_gate_decode %s, gf2_mc_mretry_gate_decode %s; ratio of medians new / old = %.3f"
                % (ops, p, multi.num_locations, sum(int(multi.type_site_regions[r].sum()) for r in regions_of(multi)), multi.preparations,
                   samples.bit_length() - 1, int(c_new[0]) / samples, int(c_new[21]) / samples / multi.preparations, spread(times["old"]),
                   spread(times["new"]), statistics.median(times["new"]) / statistics.median(times["old"])))
    for instructions in MULTI:
        multi = stream_noise.multi_program_for(code, instructions)
        old = lambda n, seed=0: multi.retry_counts(n, P_KIND, P_KIND, P_KIND, seed=seed)
        new = lambda n, seed=0: multi.retry_gate_counts(n, P_GATE, P_GATE, seed=seed)
        samples = grown(old, new)
        sites = sum(int(multi.type_site_regions[r].sum()) for r in regions_of(multi))
        times = {"old": [], "new": []}
        for r in range(ROUNDS):
            t_old, c_old = timed(lambda: old(samples, r))
            t_new, c_new = timed(lambda: new(samples, r))
            times["old"].append(samples / t_old)
            times["new"].append(samples / t_new)
        say("(ii) Q = %d, %d blocks, L = %d, %d sites, %d preparations, records = reference, N = 2^%d: locations at p_kind = %g expect %.3f "
            "faults per first pass, gates at p = %g expect %.3f; attempts per preparation %.4f (locations) %.4f (gates), exhausted %d and %d; "
            "samples/s: gf2_mc_mretry_decode %s, gf2_mc_mretry_gate_decode %s; ratio of medians gates / locations = %.3f"
            % (multi.nframes, len(multi.block_type), multi.num_locations, sites, multi.preparations, samples.bit_length() - 1, P_KIND,
               3 * P_KIND * multi.num_locations, P_GATE, P_GATE * sites, int(c_old[21]) / samples / multi.preparations,
               int(c_new[21]) / samples / multi.preparations, int(c_old[20]), int(c_new[20]), spread(times["old"]), spread(times["new"]),
               statistics.median(times["new"]) / statistics.median(times["old"])))
    log.close()


def regions_of(multi):
    """The rows of type_site_regions of every block of the sequence, a type's as often as it occurs."""
    first = np.concatenate([[0], np.cumsum(multi.type_nregions)])
    return [r for t in multi.block_type for r in range(int(first[t]), int(first[t + 1]))]


if __name__ == "__main__":
    main()
