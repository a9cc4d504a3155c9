#!/usr/bin/env python3
"""The direct Monte-Carlo under gate-level faults against the location model's direct sampler of the same build, in one process
(DESIGN.md section 5e "Direct Monte-Carlo under gate-level faults", "Speed"): samples per second of gf2_mc_ec_decode_gate /
gf2_mc_ft_decode_gate at p_1 = p_2 = p against gf2_mc_ec_decode / gf2_mc_ft_decode at the rate per location that gives the same
expected number of faults per sample, p (n_1 + n_2) / L split evenly over X, Y, Z -- the one-round Steane cycle (LDR 3, staged in
LDS) and the gate-free Steane program (LDR 8, through L2) at p = 1e-3 and 3.2e-3, 2^30 samples each.  Every timing is one whole call
between the context's HIP events (gf2_timer_*: tables, launch and the copy back of the counts); after a warm-up the two alternate and
the median of the repeats is reported with the spread.  The lines are appended to profiles/time_gate_mc.log."""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_css_codes_amd import _native, ec_noise, ft_noise  # noqa: E402
from quantum_css_codes_amd.css_code import CSSCode  # noqa: E402

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
REPEATS = 5
SAMPLES = 1 << 30


def timed(ctx, fn):
    ctx.timer_start()
    fn()
    return SAMPLES / (ctx.timer_stop() * 1e-3)


def main():
    ctx = _native.default_context()
    code = CSSCode(STEANE, STEANE)
    log = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "time_gate_mc.log"), "a")
    cycle, program = ec_noise.circuit_for(code, 1), ft_noise.program_for(code, "")
    for name, gadget, location_fn in (("steane cycle", cycle, cycle.logical_error_rates), ("steane '' MEASURE", program, program.measurement_error_rates)):
        _, n1, n2, _ = gadget.gate_sites()
        for p in (1e-3, 3.2e-3):
            each = p * (n1 + n2) / gadget.num_locations / 3.0               # the same expected number of faults per sample
            paths = {"gates": lambda: gadget.gate_error_rates(SAMPLES, p, p, seed=1), "locations": lambda: location_fn(SAMPLES, each, each, each, seed=1)}
            for fn in paths.values():                                       # warm-up: tables, code objects
                fn()
            got = {key: [] for key in paths}
            for _ in range(REPEATS):                                         # alternate
                for key, fn in paths.items():
                    got[key].append(timed(ctx, fn))
            med = {key: statistics.median(vals) for key, vals in got.items()}
            text = ("%s L=%d n1=%d n2=%d ldr=%d, %d samples, %.3g faults per sample, median of %d: gate faults p1 = p2 = %g %.3e /s (%.3e .. %.3e; "
                    "%d accepted); location faults p = %.4g %.3e /s (%.3e .. %.3e; %d accepted); gates / locations = %.2f"
                    % (name, gadget.num_locations, n1, n2, gadget.ldr, SAMPLES, p * (n1 + n2), REPEATS, p, med["gates"], min(got["gates"]),
                       max(got["gates"]), paths["gates"]()['accepted'], 3.0 * each, med["locations"], min(got["locations"]), max(got["locations"]),
                       paths["locations"]()['accepted'], med["gates"] / med["locations"]))
            print(text, flush=True)
            log.write(text + "\n")
    log.close()


if __name__ == "__main__":
    main()
