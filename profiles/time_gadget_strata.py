#!/usr/bin/env python3
"""The sampled strata of the logical measurement against the direct sampler of the same build, in one process (DESIGN.md "Sampled
strata of the measurement", "Speed"): samples per second of gf2_mc_ft_decode_strata at w = 3 and at w = 16 and of gf2_mc_ft_decode at
p = (0.0002, 0.0001, 0.0002) -- the path this build had before the strata, the baseline -- on the FTProgram of the Steane code and
X X X MEASURE (L = 2584, ldr = 11, effects through L2), 2^22 samples each.
Every timing is one whole call between the context's HIP events (gf2_timer_*: tables, launch and the copy back of the counts); after
a warm-up the three alternate and the median of the repeats is reported."""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_css_codes_amd import _native, ft_noise  # noqa: E402
from quantum_css_codes_amd.css_code import CSSCode  # noqa: E402

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
REPEATS = 5
SAMPLES = 1 << 22
P = (0.0002, 0.0001, 0.0002)


def timed(ctx, fn):
    ctx.timer_start()
    fn()
    return SAMPLES / (ctx.timer_stop() * 1e-3)


def main():
    ctx = _native.default_context()
    prog = ft_noise.program_for(CSSCode(STEANE, STEANE), "XXX")
    paths = {"w=3": lambda: prog.strata([3], SAMPLES, seed=1),
             "w=16": lambda: prog.strata([16], SAMPLES, seed=1),
             "direct": lambda: prog.measurement_error_rates(SAMPLES, *P, seed=1)}
    for fn in paths.values():                                               # warm-up: tables, code objects
        fn()
    got = {key: [] for key in paths}
    for _ in range(REPEATS):                                                 # alternate
        for key, fn in paths.items():
            got[key].append(timed(ctx, fn))
    med = {key: statistics.median(vals) for key, vals in got.items()}
    accepted = {key: int(paths[key]().counts[0, 0]) for key in ("w=3", "w=16")}
    print("steane XXX L=%d ldr=%d, %d samples, median of %d: gf2_mc_ft_decode_strata w=3 %.3e /s (%.3e .. %.3e; %d accepted); "
          "w=16 %.3e /s (%.3e .. %.3e; %d accepted); gf2_mc_ft_decode %.3e /s (%.3e .. %.3e); w=3 / direct = %.2f, w=16 / direct = %.2f"
          % (prog.num_locations, prog.ldr, SAMPLES, REPEATS, med["w=3"], min(got["w=3"]), max(got["w=3"]), accepted["w=3"], med["w=16"],
             min(got["w=16"]), max(got["w=16"]), accepted["w=16"], med["direct"], min(got["direct"]), max(got["direct"]),
             med["w=3"] / med["direct"], med["w=16"] / med["direct"]), flush=True)


if __name__ == "__main__":
    main()
