#!/usr/bin/env python3
"""The error-correction cycle's tally against the store path of the same build, in one process (DESIGN.md "Error-correction cycle"):
samples per second of gf2_mc_ec_decode (nothing stored per sample) and of gf2_circuit_outcomes_dev (ldr words stored per sample, into
a buffer allocated beforehand) on the same ECCircuit -- the Steane code at rounds 1 (L = 330, effects staged in LDS), 2 and 4
(effects through L2), 2^22 samples at p = (0.001, 0.0005, 0.001).  Every timing is one whole call between the context's HIP events
(gf2_timer_*: for the tally that is tables, launch and the copy back of the counts); after a warm-up the two alternate and the
median of the repeats is reported.  `--one tally|store ROUNDS` runs one path once (for a kernel trace)."""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_css_codes_amd import _native, ec_noise  # noqa: E402
from quantum_css_codes_amd.css_code import CSSCode  # noqa: E402

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
REPEATS = 5
SAMPLES = 1 << 22
P = (0.001, 0.0005, 0.001)


def paths_of(ctx, circ, buf):
    return {"tally": lambda: circ.logical_error_rates(SAMPLES, *P, seed=1),
            "store": lambda: ctx.circuit_outcomes_dev(circ.device(), 1, 0, SAMPLES, *P, buf, circ.ldr)}


def timed(ctx, fn):
    ctx.timer_start()
    fn()
    return SAMPLES / (ctx.timer_stop() * 1e-3)


def main():
    ctx = _native.default_context()
    code = CSSCode(STEANE, STEANE)
    one = sys.argv[2:4] if len(sys.argv) > 3 and sys.argv[1] == "--one" else None
    for rounds in ((int(one[1]),) if one else (1, 2, 4)):
        circ = ec_noise.circuit_for(code, rounds)
        buf = ctx.alloc(SAMPLES * circ.ldr * 8)
        paths = paths_of(ctx, circ, buf)
        if one:
            paths[one[0]]()
            ctx.sync()
            buf.free()
            return
        for fn in paths.values():                                           # warm-up: tables, code objects
            fn()
        got = {key: [] for key in paths}
        for _ in range(REPEATS):                                             # alternate
            for key, fn in paths.items():
                got[key].append(timed(ctx, fn))
        accepted = circ.logical_error_rates(SAMPLES, *P, seed=1)['accepted']
        med = {key: statistics.median(vals) for key, vals in got.items()}
        print("steane rounds=%d L=%d ldr=%d, %d samples (%d accepted): tally %.3e /s (%.3e .. %.3e); store %.3e /s (%.3e .. %.3e); "
              "median of %d; tally/store = %.2f" % (rounds, circ.num_locations, circ.ldr, SAMPLES, accepted, med["tally"], min(got["tally"]),
                                                    max(got["tally"]), med["store"], min(got["store"]), max(got["store"]), REPEATS,
                                                    med["tally"] / med["store"]), flush=True)
        buf.free()


if __name__ == "__main__":
    main()
