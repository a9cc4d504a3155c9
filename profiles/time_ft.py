#!/usr/bin/env python3
"""The logical measurement's tally against the store path of the same build, in one process (DESIGN.md "Logical measurement"):
samples per second of gf2_mc_ft_decode (nothing stored per sample) and of gf2_ft_outcomes_dev (ldr words stored per sample, into a
buffer allocated beforehand) on the FTProgram of the Steane code and X X X MEASURE (L = 2584, ldr = 11, effects through L2), and for
comparison of gf2_mc_ec_decode on the 5-round Steane cycle (L = 1650, ldr = 8: the longest Steane cycle its 8 words hold; 6 rounds
need 9), 2^22 samples at p = (0.0002, 0.0001, 0.0002).
Every timing is one whole call between the context's HIP events (gf2_timer_*: for a tally that is tables, launch and the copy back
of the counts); after a warm-up the three alternate and the median of the repeats is reported.  `--one tally|store|cycle` runs one
path once (for a kernel trace)."""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_css_codes_amd import _native, ec_noise, ft_noise  # noqa: E402
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
    code = CSSCode(STEANE, STEANE)
    prog = ft_noise.program_for(code, "XXX")
    cycle = ec_noise.circuit_for(code, 5)
    buf = ctx.alloc(SAMPLES * prog.ldr * 8)
    paths = {"tally": lambda: prog.measurement_error_rates(SAMPLES, *P, seed=1),
             "store": lambda: ctx.ft_outcomes_dev(prog.device(), 1, 0, SAMPLES, *P, buf, prog.ldr),
             "cycle": lambda: cycle.logical_error_rates(SAMPLES, *P, seed=1)}
    if len(sys.argv) > 2 and sys.argv[1] == "--one":
        paths[sys.argv[2]]()
        ctx.sync()
        buf.free()
        return
    for fn in paths.values():                                               # warm-up: tables, code objects
        fn()
    got = {key: [] for key in paths}
    for _ in range(REPEATS):                                                 # alternate
        for key, fn in paths.items():
            got[key].append(timed(ctx, fn))
    counts = prog.measurement_error_rates(SAMPLES, *P, seed=1)
    med = {key: statistics.median(vals) for key, vals in got.items()}
    print("steane XXX L=%d ldr=%d, %d samples (%d accepted, %d wrong): tally %.3e /s (%.3e .. %.3e); store %.3e /s (%.3e .. %.3e); "
          "tally/store = %.2f" % (prog.num_locations, prog.ldr, SAMPLES, counts['accepted'], counts['wrong'], med["tally"], min(got["tally"]),
                                  max(got["tally"]), med["store"], min(got["store"]), max(got["store"]), med["tally"] / med["store"]), flush=True)
    print("steane cycle rounds=5 L=%d ldr=%d: gf2_mc_ec_decode %.3e /s (%.3e .. %.3e); median of %d"
          % (cycle.num_locations, cycle.ldr, med["cycle"], min(got["cycle"]), max(got["cycle"]), REPEATS), flush=True)
    buf.free()


if __name__ == "__main__":
    main()
