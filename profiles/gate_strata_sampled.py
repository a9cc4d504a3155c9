#!/usr/bin/env python3
"""The results of DESIGN.md section 5e "Sampled strata under gate-level faults", regenerated: for the Reed-Muller [[15,1,3]] gate-free
program MEASURE and the one-round Steane cycle, the exact strata of weights 0 .. E under gate-level faults merged with the sampled
strata (a, b) of every weight E + 1 .. 16, and rate(odds, field) at depolarising gate faults p_1 = p_2 = 1e-4, 1e-3 and 3.2e-3 with its
standard error and bounds.  E = 2 on the device; `--host` runs the host statements (no GPU) with E = 1 for the program, whose exact
weight 2 takes the host minutes; `--samples N` sets N per stratum (default 2^20 on the device, 2^16 on the host).
The lines are appended to profiles/gate_strata_sampled[_host].log."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_css_codes_amd import ec_noise, ft_noise  # noqa: E402
from quantum_css_codes_amd.montecarlo import GateStrata  # noqa: E402

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
P_VALUES = (1e-4, 1e-3, 3.2e-3)
MAX_WEIGHT = 16


def rm15_checks():
    cols = np.arange(1, 16)
    h1 = np.array([(cols >> b) & 1 for b in range(4)])
    return h1, np.vstack([h1] + [h1[a] & h1[b] for a in range(4) for b in range(a + 1, 4)])


def main():
    host = "--host" in sys.argv
    samples = int(sys.argv[sys.argv.index("--samples") + 1]) if "--samples" in sys.argv else 1 << (16 if host else 20)
    if host:
        from oracle import cpu_ref
        make = cpu_ref.CSSCode
    else:
        from quantum_css_codes_amd.css_code import CSSCode as make
    log = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "gate_strata_sampled%s.log" % ("_host" if host else "")), "a")

    def say(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    for name, gadget, field, top in (("rm15 '' MEASURE", ft_noise.program_for(make(*rm15_checks()), ""), 'wrong', 1 if host else 2),
                                     ("steane cycle, 1 round", ec_noise.circuit_for(make(STEANE, STEANE), 1), 'logical_any', 2)):
        _, n1, n2, _ = gadget.gate_sites()
        exact = gadget.enumerate_gate_strata(list(range(top + 1)), max_configurations=1 << 40, host=host)
        strata = [(w - b, b) for w in range(top + 1, MAX_WEIGHT + 1) for b in range(w + 1)]
        sampled = gadget.gate_strata(strata, samples, seed=0, host=host)
        merged = exact.merged(sampled)
        by_weight = lambda col: [int(sampled.counts[[s for s, (a, b) in enumerate(strata) if a + b == w], :, col].sum())
                                 for w in range(top + 1, MAX_WEIGHT + 1)]
        say("%s n1=%d n2=%d: exact weights 0..%d, sampled strata (a, b) of weights %d..%d (%d strata, %s, N = %d per stratum, seed 0); "
            "accepted per weight %s; %s %s" % (name, n1, n2, top, top + 1, MAX_WEIGHT, len(strata), "host statement" if host else "device", samples,
                                                by_weight(0), field, by_weight(sampled.fields.index(field))))
        for p in P_VALUES:
            odds = GateStrata.depolarising_odds(p, p)
            alone = exact.rate(odds, field)
            got = merged.rate(odds, field)
            d, d_t = merged.acceptance(odds)
            say("%s p1=p2=%g: exact weights alone [%.4g, %.4g]; merged estimate %.6g +- %.2g, bounds [%.6g, %.6g], T = %.2g; acceptance [%.4f, %.4f]"
                % (name, p, alone[1], alone[2], got.estimate, got.stderr, got.lower, got.upper, d_t - d, d, d_t))
    log.close()


if __name__ == "__main__":
    main()
