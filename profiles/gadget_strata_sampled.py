#!/usr/bin/env python3
"""The results of DESIGN.md "Sampled strata of the measurement", regenerated: for the Reed-Muller [[15,1,3]] program MEASURE and the
Steane program X X X MEASURE, the exact strata 0 .. 2 merged with sampled strata 3 .. W, W the smallest weight that leaves the
mass T of the weights above W below 1 % of the estimate at p = 1e-3 (the strata 3 .. 16 are all drawn, the first W that suffices is kept);
rate(p, 'wrong') at p = 1e-4 and 1e-3 with kinds (1, 1, 1) against ft_noise.raw_program_error_rate.  `--host` runs the host
statements (no GPU; the weight-2 strata of the larger programs take minutes); `--samples N` sets N per stratum (default 2^20).
The lines are appended to profiles/gadget_strata_sampled[_host].log."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_css_codes_amd import ft_noise, montecarlo  # noqa: E402

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
KINDS = (1, 1, 1)
P_VALUES = (1e-4, 1e-3)
MAX_WEIGHT = 16


def rm15_checks():
    cols = np.arange(1, 16)
    h1 = np.array([(cols >> b) & 1 for b in range(4)])
    return h1, np.vstack([h1] + [h1[a] & h1[b] for a in range(4) for b in range(a + 1, 4)])


def smallest_top(exact, sampled):
    """(W, the sampled strata 3 .. W, their merge with the exact ones): the smallest W that leaves the mass T of the weights above W
    below 1 % of the estimate at p = 1e-3 (MAX_WEIGHT if none does)."""
    for k in range(1, len(sampled.weights) + 1):
        part = montecarlo.SampledPostSelectedStrata(sampled.nb, sampled.weights[:k], sampled.samples[:k], sampled.counts[:k], sampled.fields,
                                                    sampled.kinds)
        merged = exact.merged(part)
        got = merged.rate(1e-3, 'wrong')
        d, d_t = merged.acceptance(1e-3)
        if d_t - d < 0.01 * got.estimate:
            break
    return int(part.weights[-1]), part, merged


def main():
    host = "--host" in sys.argv
    samples = int(sys.argv[sys.argv.index("--samples") + 1]) if "--samples" in sys.argv else 1 << 20
    if host:
        from oracle import cpu_ref
        make = cpu_ref.CSSCode
    else:
        from quantum_css_codes_amd.css_code import CSSCode as make
    log = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "gadget_strata_sampled%s.log" % ("_host" if host else "")), "a")

    def say(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    for name, code, ops in (("rm15", make(*rm15_checks()), ""), ("steane", make(STEANE, STEANE), "XXX")):
        prog = ft_noise.program_for(code, ops)
        exact = prog.enumerate_strata([0, 1, 2], max_configurations=1 << 40, host=host)
        whole = prog.strata(list(range(3, MAX_WEIGHT + 1)), samples, kinds=KINDS, seed=0, host=host)
        top, sampled, merged = smallest_top(exact, whole)
        say("%s %r L=%d: exact strata 0..2, sampled strata 3..%d (%s, N = %d per stratum, seed 0, kinds %r); accepted per stratum %s; wrong %s"
            % (name, ops, prog.num_locations, top, "host statement" if host else "device", samples, KINDS, sampled.counts[:, 0].tolist(),
               sampled.counts[:, 1].tolist()))
        for p in P_VALUES:
            alone = exact.rate(p, KINDS, 'wrong')
            got = merged.rate(p, 'wrong')
            d, d_t = merged.acceptance(p)
            say("%s %r p=%g: exact strata alone [%.4g, %.4g]; merged estimate %.6g +- %.2g, bounds [%.6g, %.6g], T = %.2g; "
                "acceptance [%.4f, %.4f]; bare program %.6g"
                % (name, ops, p, alone[1], alone[2], got.estimate, got.stderr, got.lower, got.upper, d_t - d, d, d_t,
                   ft_noise.raw_program_error_rate(ops, p / 3, p / 3, p / 3)))
    log.close()


if __name__ == "__main__":
    main()
