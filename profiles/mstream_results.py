#!/usr/bin/env python3
"""The results of DESIGN.md section 5d "Multi-block programs", regenerated: the rewritten programs `CNOT 0 1; MEASURE 1` and
`X 0; CNOT 0 1; MEASURE 0; MEASURE 1` on the Steane and the Reed-Muller [[15,1,3]] code at p_x = p_y = p_z = p for p = 5e-5, 1e-4 and
2e-4 -- per measured bit the rate of `wrong` among accepted samples with its binomial standard error under records = 'reference'
and under 'propagated' (the same samples: the words do not depend on `records`), the difference of the two in units of the
standard error of a difference of two counts on the same samples, and ft_noise.raw_circuit_error_rate for the bare program -- then
the host single-fault census of every program: how many of the 3 L single faults are accepted, how many of those give a wrong bit,
and in which blocks they lie.

N = 2^28 samples per point on the device.  `--host` runs the host statements (no GPU) on the restated sampler's faults at 2^18
samples per point, `--samples N` sets N.  The lines are appended to profiles/mstream_results[_host].log."""
import collections
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_css_codes_amd import ft_noise, stream_noise  # noqa: E402

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
PROGRAMS = ((('CNOT', 0, 1), ('MEASURE', 1)), (('X', 0), ('CNOT', 0, 1), ('MEASURE', 0), ('MEASURE', 1)))
RATES = (5e-5, 1e-4, 2e-4)


def rm15_checks():
    cols = np.arange(1, 16)
    h1 = np.array([(cols >> b) & 1 for b in range(4)])
    return h1, np.vstack([h1] + [h1[a] & h1[b] for a in range(4) for b in range(a + 1, 4)])


def text_of(instructions):
    return "; ".join(" ".join(str(v) for v in inst) for inst in instructions)


def host_counts(prog, samples, p, seed, records):
    """The host statements on the restated sampler's faults, in chunks."""
    from tests import stream_ref
    total = np.zeros(20, dtype=np.uint64)
    for first in range(0, samples, 1 << 14):
        count = min(1 << 14, samples - first)
        words = prog.words_of_faults(*stream_ref.sampled_faults(prog.num_locations, seed, first, count, (p, p, p)))
        total += prog.tally_host(words, records=records, fields=True)
    return total


def census(prog, say, name):
    """Every single fault of the program on the host: accepted, and wrong per measured bit, by the block it lies in."""
    total = prog.num_locations
    first = np.arange(3 * total + 1, dtype=np.int64)
    where = np.tile(np.arange(total, dtype=np.int32), 3)
    kinds = np.repeat(np.array([1, 2, 3], dtype=np.uint8), total)
    words = prog.words_of_faults(first, where, kinds)
    block_of = np.searchsorted(prog.block_start, where, side="right") - 1
    for records in ('reference', 'propagated'):
        counts, classes = prog.tally_host(words, records=records, fields=True, classes=True)
        say("%s single faults, records = %s: %d faults (3 L), %d accepted, %d of them give a wrong bit (per measured bit: %s), %d flip a trial"
            % (name, records, 3 * total, int(counts[0]), int(counts[1]), [int(counts[4 + 4 * m]) for m in range(len(prog.measured))],
               int(sum(counts[5 + 4 * m] for m in range(len(prog.measured))))))
        for m, qubit in enumerate(prog.measured):
            bad = np.flatnonzero((classes >> (2 + m)) & 1)
            by_block = collections.Counter((int(block_of[f]), prog.types[prog.block_type[block_of[f]]].name, int(prog.block_a[block_of[f]])) for f in bad)
            by_kind = collections.Counter("?XZY"[int(kinds[f])] for f in bad)
            say("    MEASURE %d wrong: %d faults %s; by block (index, type, frame): %s"
                % (qubit, len(bad), dict(by_kind), ", ".join("%d %s on frame %d: %d" % (b + (c,)) for b, c in sorted(by_block.items()))))


def main():
    host = "--host" in sys.argv
    samples = int(sys.argv[sys.argv.index("--samples") + 1]) if "--samples" in sys.argv else 1 << (18 if host else 28)
    if host:
        from oracle import cpu_ref
        make = cpu_ref.CSSCode
    else:
        from quantum_css_codes_amd.css_code import CSSCode as make
    log = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "mstream_results%s.log" % ("_host" if host else "")), "a")

    def say(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    how = "host statements" if host else "device"
    for code_name, code in (("steane", make(STEANE, STEANE)), ("rm15", make(*rm15_checks()))):
        for instructions in PROGRAMS:
            prog = stream_noise.MultiProgram(code, instructions)
            name = "%s '%s'" % (code_name, text_of(instructions))
            say("%s: L = %d, %d blocks, %d steps (%s, N = %d per rate, seed = index of the rate)"
                % (name, prog.num_locations, len(prog.block_type), prog.nsteps, how, samples))
            for index, p in enumerate(RATES):
                got = {}
                for records in ('reference', 'propagated'):
                    got[records] = host_counts(prog, samples, p, index, records) if host else \
                        prog.counts(samples, p, p, p, seed=index, records=records)
                accepted = int(got['reference'][0])
                raw = ft_noise.raw_circuit_error_rate(instructions, p, p, p)
                say("%s p = %g: accepted %d of %d (%.5f)" % (name, p, accepted, samples, accepted / samples))
                for m, qubit in enumerate(prog.measured):
                    parts = []
                    for records in ('reference', 'propagated'):
                        wrong = int(got[records][4 + 4 * m])
                        r = wrong / accepted
                        parts.append("%s wrong %d: %.6g +- %.2g" % (records, wrong, r, math.sqrt(r * (1.0 - r) / accepted)))
                    a, b = int(got['reference'][4 + 4 * m]), int(got['propagated'][4 + 4 * m])
                    # the two tallies run over the same samples: the difference of the counts is at most as noisy as sqrt(a + b)
                    z = (b - a) / math.sqrt(a + b) if a + b else 0.0
                    say("    MEASURE %d: %s; propagated - reference = %+d samples = %+.2f sqrt(a + b); bare program %.6g"
                        % (qubit, "; ".join(parts), b - a, z, raw[m]))
            census(prog, say, name)
    log.close()


if __name__ == "__main__":
    main()
