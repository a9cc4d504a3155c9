#!/usr/bin/env python3
"""The gate-fault enumeration against the location enumeration of the same build, in one process (DESIGN.md section 5e "Speed"):
configurations per second of gf2_ec_gate_enumerate on the one-round Steane cycle at total weight 3 (every b: 1.1 x 10^9
configurations) against gf2_ec_enumerate at w = 3 (1.6 x 10^8), and of gf2_ft_gate_enumerate on the gate-free Steane program at
weight 2 (4.2 x 10^7) against gf2_ft_enumerate at w = 2 (1.1 x 10^7).  Every timing is whole calls between the context's HIP
events (gf2_timer_*: tables, launches and the copy back of the counts); after a warm-up the paths alternate, and the median of
the repeats is reported with the spread.  `--one ec|ft` runs one gate-fault enumeration once (for a kernel trace)."""
import math
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_css_codes_amd import _native, ec_noise, ft_noise  # noqa: E402
from quantum_css_codes_amd.css_code import CSSCode  # noqa: E402

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
REPEATS = 5
BUDGET = 1 << 40


def timed(ctx, fn, work):
    ctx.timer_start()
    fn()
    return work / (ctx.timer_stop() * 1e-3)


def main():
    ctx = _native.default_context()
    code = CSSCode(STEANE, STEANE)
    cycle = ec_noise.circuit_for(code, 1)
    prog = ft_noise.program_for(code, "")
    gate = lambda gadget, w: gadget.enumerate_gate_strata([w], max_configurations=BUDGET)
    sites = lambda gadget, w: sum(math.comb(gadget.gate_sites()[1], w - b) * math.comb(gadget.gate_sites()[2], b) * 3**(w - b) * 15**b
                                  for b in range(w + 1))
    work = {"ec_gate": sites(cycle, 3), "ec": 27 * math.comb(cycle.num_locations, 3), "ft_gate": sites(prog, 2),
            "ft": 9 * math.comb(prog.num_locations, 2)}
    paths = {"ec_gate": lambda: gate(cycle, 3), "ec": lambda: cycle.enumerate_strata([3], max_configurations=BUDGET),
             "ft_gate": lambda: gate(prog, 2), "ft": lambda: prog.enumerate_strata([2], max_configurations=BUDGET)}
    if len(sys.argv) > 2 and sys.argv[1] == "--one":
        paths[sys.argv[2] + "_gate"]()
        ctx.sync()
        return
    for fn in paths.values():                                               # warm-up: tables, code objects
        fn()
    got = {key: [] for key in paths}
    for _ in range(REPEATS):                                                 # alternate
        for key, fn in paths.items():
            got[key].append(timed(ctx, fn, work[key]))
    med = {key: statistics.median(vals) for key, vals in got.items()}
    for rule, gadget, w, what in (("ec", cycle, 3, "steane cycle rounds=1"), ("ft", prog, 2, "steane program ''")):
        g = rule + "_gate"
        print("%s L=%d ldr=%d weight %d: gf2_%s_gate_enumerate %.4g configurations, %.3e /s (%.3e .. %.3e); gf2_%s_enumerate %.4g "
              "configurations, %.3e /s (%.3e .. %.3e); ratio %.2f; median of %d"
              % (what, gadget.num_locations, gadget.ldr, w, rule, work[g], med[g], min(got[g]), max(got[g]), rule, work[rule], med[rule],
                 min(got[rule]), max(got[rule]), med[g] / med[rule], REPEATS), flush=True)


if __name__ == "__main__":
    main()
