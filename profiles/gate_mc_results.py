#!/usr/bin/env python3
"""The results of DESIGN.md section 5e "Direct Monte-Carlo under gate-level faults", regenerated: the Reed-Muller [[15,1,3]] gate-free
program MEASURE under depolarising gate faults p_1 = p_2 = p at p = 1, 2, 2.5, 3, 3.2, 3.5, 4 and 5 x 10^-3 -- the direct rate of
`wrong` among accepted samples with its binomial standard error, the acceptance, the merged-strata figure of "Sampled strata under
gate-level faults" where that section has one (profiles/gate_strata_sampled.log) and the bare qubit's 2 p / 3 -- then where the direct
rate crosses 2 p / 3, by linear interpolation between the two neighbouring rates, with the error bar the two standard errors give;
and the one-round Steane cycle's `logical_any` at p = 1e-4, 1e-3 and 3.2e-3 against the merged figures of the same log.

N = 2^32 samples per rate on the device: at p = 3.2e-3 0.62 % of them are accepted and 2.3e-3 of those are wrong, 6e4 wrong
samples, a relative standard error of 0.41 % (1 % takes 2^30).  `--host` runs the host statement (no GPU) at 2^22
samples per rate, `--samples N` sets N.  The lines are appended to profiles/gate_mc_results[_host].log."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_css_codes_amd import ec_noise, ft_noise  # noqa: E402

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
RM15_P = (1e-3, 2e-3, 2.5e-3, 3e-3, 3.2e-3, 3.5e-3, 4e-3, 5e-3)
STEANE_P = (1e-4, 1e-3, 3.2e-3)
# profiles/gate_strata_sampled.log: merged estimate +- standard error (exact weights 0 .. 2, sampled weights 3 .. 16)
RM15_MERGED = {1e-3: (2.17506e-4, 5.8e-6), 3.2e-3: (2.36033e-3, 8.5e-5)}
STEANE_MERGED = {1e-4: (6.36653e-5, 1.4e-10), 1e-3: (9.62104e-4, 1.2e-7), 3.2e-3: (5.51942e-3, 3.4e-6)}


def rm15_checks():
    cols = np.arange(1, 16)
    h1 = np.array([(cols >> b) & 1 for b in range(4)])
    return h1, np.vstack([h1] + [h1[a] & h1[b] for a in range(4) for b in range(a + 1, 4)])


def rate_of(counts, field):
    r = counts[field] / counts['accepted']
    return r, math.sqrt(r * (1.0 - r) / counts['accepted'])


def main():
    host = "--host" in sys.argv
    samples = int(sys.argv[sys.argv.index("--samples") + 1]) if "--samples" in sys.argv else 1 << (22 if host else 32)
    if host:
        from oracle import cpu_ref
        make = cpu_ref.CSSCode
    else:
        from quantum_css_codes_amd.css_code import CSSCode as make
    log = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "gate_mc_results%s.log" % ("_host" if host else "")), "a")

    def say(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    how = "host statement" if host else "device"
    gadget = ft_noise.program_for(make(*rm15_checks()), "")
    _, n1, n2, _ = gadget.gate_sites()
    say("rm15 '' MEASURE n1=%d n2=%d: direct Monte-Carlo under gate-level faults, every gate on its own (%s, N = %d per rate, seed = index of the rate)"
        % (n1, n2, how, samples))
    points = []
    for index, p in enumerate(RM15_P):
        counts = gadget.gate_error_rates(samples, p, p, seed=index, host=host)
        r, se = rate_of(counts, 'wrong')
        bare = 2.0 * p / 3.0
        merged = "merged strata %.6g +- %.2g (direct - merged = %+.2f combined standard errors)" % (
            RM15_MERGED[p] + ((r - RM15_MERGED[p][0]) / math.hypot(se, RM15_MERGED[p][1]),)) if p in RM15_MERGED else "merged strata: none"
        say("rm15 '' MEASURE p1=p2=%g: %.4g faulty gates per sample; accepted %d of %d (%.5f); wrong %d: direct rate %.6g +- %.2g (%.2f %%); %s; "
            "bare qubit 2p/3 = %.6g; direct - bare = %+.3g = %+.1f standard errors"
            % (p, (n1 + n2) * p, counts['accepted'], samples, counts['accepted'] / samples, counts['wrong'], r, se, 100.0 * se / r if r else 0.0, merged,
               bare, r - bare, (r - bare) / se if se else 0.0))
        points.append((p, r - bare, se))
    crossings = [(lo, hi) for lo, hi in zip(points, points[1:]) if lo[1] < 0.0 <= hi[1]]
    if not crossings:
        say("rm15 '' MEASURE: the direct rate does not cross 2p/3 from below among these rates (direct - bare from %+.3g to %+.3g)"
            % (points[0][1], points[-1][1]))
    for (p_lo, d_lo, se_lo), (p_hi, d_hi, se_hi) in crossings:
        t = -d_lo / (d_hi - d_lo)                                             # the zero of the chord through the two differences
        p_star = p_lo + t * (p_hi - p_lo)
        err = (p_hi - p_lo) / (d_hi - d_lo) * math.hypot((1.0 - t) * se_lo, t * se_hi)     # first order in the two standard errors
        say("rm15 '' MEASURE: the direct rate crosses 2p/3 between p = %g and %g: p* = %.4g +- %.2g (chord through the two differences, one "
            "standard error; the curvature of the rate between them is left out)" % (p_lo, p_hi, p_star, err))
    gadget = ec_noise.circuit_for(make(STEANE, STEANE), 1)
    _, n1, n2, _ = gadget.gate_sites()
    for index, p in enumerate(STEANE_P):
        counts = gadget.gate_error_rates(samples, p, p, seed=100 + index, host=host)
        r, se = rate_of(counts, 'logical_any')
        m, m_se = STEANE_MERGED[p]
        say("steane cycle, 1 round n1=%d n2=%d p1=p2=%g (%s, N = %d): accepted %.5f; direct logical_any %.6g +- %.2g; merged strata %.6g +- %.2g; "
            "direct - merged = %+.2f combined standard errors" % (n1, n2, p, how, samples, counts['accepted'] / samples, r, se, m, m_se,
                                                                    (r - m) / math.hypot(se, m_se)))
    log.close()


if __name__ == "__main__":
    main()
