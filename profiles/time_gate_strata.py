#!/usr/bin/env python3
"""The sampled strata under gate-level faults against the sampled strata over locations of the same build, in one process (DESIGN.md
section 5e "Sampled strata under gate-level faults", "Speed"): samples per second of gf2_mc_ec_decode_gate_strata /
gf2_mc_ft_decode_gate_strata at (a, b) against gf2_mc_ec_decode_strata / gf2_mc_ft_decode_strata at the equal total weight a + b -- the
one-round Steane cycle (staged in LDS) at weights 3 and 8, the gate-free Steane program (through L2) at weight 3 -- 2^30 samples each.
Every timing is one whole call between the context's HIP events (gf2_timer_*: tables, launch and the copy back of the counts); after a
warm-up the two alternate and the median of the repeats is reported with the spread.  The line is appended to
profiles/time_gate_strata.log."""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_css_codes_amd import _native, ec_noise, ft_noise  # noqa: E402
from quantum_css_codes_amd.css_code import CSSCode  # noqa: E402

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
REPEATS = 5
SAMPLES = 1 << 30                                                           # 11 to 47 ms per call: its fixed cost (tables, site_loc, counts) is a few per cent at most


def timed(ctx, fn):
    ctx.timer_start()
    fn()
    return SAMPLES / (ctx.timer_stop() * 1e-3)


def main():
    ctx = _native.default_context()
    code = CSSCode(STEANE, STEANE)
    log = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "time_gate_strata.log"), "a")
    for name, gadget, stratum in (("steane cycle", ec_noise.circuit_for(code, 1), (2, 1)), ("steane cycle", ec_noise.circuit_for(code, 1), (4, 4)),
                                  ("steane '' MEASURE", ft_noise.program_for(code, ""), (2, 1))):
        weight = sum(stratum)
        paths = {"gates": lambda: gadget.gate_strata([stratum], SAMPLES, seed=1), "locations": lambda: gadget.strata([weight], SAMPLES, seed=1)}
        for fn in paths.values():                                           # warm-up: tables, code objects
            fn()
        got = {key: [] for key in paths}
        for _ in range(REPEATS):                                             # alternate
            for key, fn in paths.items():
                got[key].append(timed(ctx, fn))
        med = {key: statistics.median(vals) for key, vals in got.items()}
        text = ("%s L=%d ldr=%d, %d samples, median of %d: gate strata (a, b) = %r %.3e /s (%.3e .. %.3e; %d accepted); location strata w = %d "
                "%.3e /s (%.3e .. %.3e; %d accepted); gates / locations = %.2f"
                % (name, gadget.num_locations, gadget.ldr, SAMPLES, REPEATS, stratum, med["gates"], min(got["gates"]), max(got["gates"]),
                   int(paths["gates"]().counts[0, :, 0].sum()), weight, med["locations"], min(got["locations"]), max(got["locations"]),
                   int(paths["locations"]().counts[0, 0]), med["gates"] / med["locations"]))
        print(text, flush=True)
        log.write(text + "\n")
    log.close()


if __name__ == "__main__":
    main()
