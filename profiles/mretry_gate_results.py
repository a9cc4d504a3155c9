#!/usr/bin/env python3
"""The results of DESIGN.md section 5d "Repeat-until-success of multi-block programs under gate-level faults", regenerated: the four
program / code rows of profiles/mretry_results.py -- `CNOT 0 1; MEASURE 1` and `X 0; CNOT 0 1; MEASURE 0; MEASURE 1` on the Steane
and the Reed-Muller [[15,1,3]] code -- with every preparation retried, at p_1 = p_2 = p for p from 1e-4 to 5e-3, a grid that brackets
the Reed-Muller crossings: per measured bit the rate of `wrong` among accepted samples with its binomial standard error under
records = 'reference' and under 'propagated' (the same samples: the words do not depend on `records`), the difference of the two in
units of the standard error of a difference of two counts on the same samples, ft_noise.raw_circuit_gate_error_rate for the bare
program, the exhausted samples and the attempts per preparation.

N = 2^27 samples per point on the device.  `--host` runs the host statement (no GPU) at 2^16 samples per point and, first, the
single-event census of every program: every site x kappa through MultiProgram.words_of_faults and the host tally -- the events, the
accepted ones and, per measurement, the accepted ones with a wrong bit, one-operand and CNOT events apart, and the first-order
coefficient c_1 = wrong one-operand events / 3 + wrong CNOT events / 15 that `wrong` / p must approach at low p.  `--samples N` sets N.
The lines are appended to profiles/mretry_gate_results[_host].log."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_css_codes_amd import ft_noise, stream_noise  # noqa: E402

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
PROGRAMS = ((('CNOT', 0, 1), ('MEASURE', 1)), (('X', 0), ('CNOT', 0, 1), ('MEASURE', 0), ('MEASURE', 1)))
RATES = (1e-4, 2e-4, 5e-4, 1e-3, 1.5e-3, 2e-3, 3e-3, 5e-3)


def rm15_checks():
    cols = np.arange(1, 16)
    h1 = np.array([(cols >> b) & 1 for b in range(4)])
    return h1, np.vstack([h1] + [h1[a] & h1[b] for a in range(4) for b in range(a + 1, 4)])


def text_of(instructions):
    return "; ".join(" ".join(str(v) for v in inst) for inst in instructions)


def host_counts(prog, samples, p, seed, records):
    """The host statement and the host tally, in chunks: the twenty-two counts."""
    total = np.zeros(22, dtype=np.uint64)
    for first in range(0, samples, 1 << 14):
        count = min(1 << 14, samples - first)
        words, _ = prog.retry_gate_words_host(count, p, p, seed=seed, first_sample=first)
        total[:20] += prog.tally_host(words[:, :prog.ldw], records=records, fields=True)
        total[20] += np.uint64(words[:, prog.nsteps:prog.ldw].any(axis=1).sum())
        total[21] += words[:, prog.ldw].sum()
    return total


def census(prog, records):
    """Per class of sites (one-operand, CNOT): the twenty counts of the host tally over every single event of the program."""
    out = []
    first_region = np.concatenate([[0], np.cumsum(prog.type_nregions)])
    first_site = np.concatenate([[0], np.cumsum(prog.type_site_regions.sum(axis=1))])
    for cl, kappas in ((0, 3), (1, 15)):
        first, where, what = [0], [], []
        for b, t in enumerate(prog.block_type):
            for r in range(int(first_region[t]), int(first_region[t + 1])):
                n1 = int(prog.type_site_regions[r, 0])
                lo = int(first_site[r]) + (n1 if cl else 0)
                for loc in prog.type_site_loc[lo:lo + int(prog.type_site_regions[r, cl])].tolist():
                    for kappa in range(1, kappas + 1):
                        for operand in range(cl + 1):
                            kind = (kappa >> (2 * operand)) & 3
                            if kind:
                                where.append(int(prog.block_start[b]) + loc + operand)
                                what.append(kind)
                        first.append(len(where))
        counts = np.zeros(20, dtype=np.uint64)
        for at in range(0, len(first) - 1, 1 << 15):
            part = np.array(first[at:at + (1 << 15) + 1], dtype=np.int64)
            words = prog.words_of_faults(part - part[0], np.array(where[part[0]:part[-1]], dtype=np.int32),
                                         np.array(what[part[0]:part[-1]], dtype=np.uint8))
            counts += prog.tally_host(words, records=records, fields=True)
        out.append((len(first) - 1, counts))
    return out


def main():
    host = "--host" in sys.argv
    samples = int(sys.argv[sys.argv.index("--samples") + 1]) if "--samples" in sys.argv else 1 << (16 if host else 27)
    if host:
        from oracle import cpu_ref
        make = cpu_ref.CSSCode
    else:
        from quantum_css_codes_amd.css_code import CSSCode as make
    log = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "mretry_gate_results%s.log" % ("_host" if host else "")), "a")

    def say(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    how = "host statement" if host else "device"
    for code_name, code in (("steane", make(STEANE, STEANE)), ("rm15", make(*rm15_checks()))):
        for instructions in PROGRAMS:
            prog = stream_noise.MultiProgram(code, instructions)
            name = "%s '%s'" % (code_name, text_of(instructions))
            say("%s retried under gate-level faults: L = %d, %d blocks, %d steps, %d preparations (%s, N = %d per rate, seed = 100 + index of the "
                "rate, max_attempts = 256)" % (name, prog.num_locations, len(prog.block_type), prog.nsteps, prog.preparations, how, samples))
            if host:
                for records in ('reference', 'propagated'):
                    (events_1, one), (events_2, two) = census(prog, records)
                    say("%s single events, records = %s: %d one-operand events, %d accepted; %d CNOT events, %d accepted"
                        % (name, records, events_1, int(one[0]), events_2, int(two[0])))
                    for m, qubit in enumerate(prog.measured):
                        a, b = int(one[4 + 4 * m]), int(two[4 + 4 * m])
                        say("    MEASURE %d: accepted events with a wrong bit: %d one-operand, %d CNOT; c_1 = %d / 3 + %d / 15 = %.4f"
                            % (qubit, a, b, a, b, a / 3.0 + b / 15.0))
            for index, p in enumerate(RATES):
                got = {}
                for records in ('reference', 'propagated'):
                    got[records] = host_counts(prog, samples, p, 100 + index, records) if host else \
                        prog.retry_gate_counts(samples, p, p, seed=100 + index, records=records)
                accepted = int(got['reference'][0])
                raw = ft_noise.raw_circuit_gate_error_rate(instructions, p, p)
                say("%s retried p_1 = p_2 = %g: accepted %d of %d, exhausted %d, attempts per preparation %.4f"
                    % (name, p, accepted, samples, int(got['reference'][20]), int(got['reference'][21]) / samples / prog.preparations))
                for m, qubit in enumerate(prog.measured):
                    parts = []
                    for records in ('reference', 'propagated'):
                        wrong = int(got[records][4 + 4 * m])
                        r = wrong / accepted
                        parts.append("%s wrong %d: %.6g +- %.2g" % (records, wrong, r, math.sqrt(r * (1.0 - r) / accepted)))
                    a, b = int(got['reference'][4 + 4 * m]), int(got['propagated'][4 + 4 * m])
                    # the two tallies run over the same samples: the difference of the counts is at most as noisy as sqrt(a + b)
                    z = (b - a) / math.sqrt(a + b) if a + b else 0.0
                    say("    MEASURE %d: %s; propagated - reference = %+d samples = %+.2f sqrt(a + b); bare program %.6g; rewritten / bare %.3f; "
                        "wrong / p %.4f" % (qubit, "; ".join(parts), b - a, z, raw[m], a / accepted / raw[m], a / accepted / p))
    log.close()


if __name__ == "__main__":
    main()
