#!/usr/bin/env python3
"""Exact strata of the two post-selected gadgets against the direct samplers of the same build, in one process (DESIGN.md "Exact
strata of the cycle" and "Exact strata of the measurement"): configurations per second of gf2_ft_enumerate on the Steane program
X X X MEASURE (L = 2584, ldr = 11, effects through L2) at w = 2 (3.0 x 10^7 configurations) and of gf2_ec_enumerate on the one-round
Steane cycle (L = 330, ldr = 3, effects staged in LDS) at w = 3 (1.6 x 10^8); the host statements' configurations per second on a
window of the same strata (wall clock: they run no GPU work); and samples per second of gf2_mc_ft_decode / gf2_mc_ec_decode on the
same circuits, 2^22 samples at p = (0.0002, 0.0001, 0.0002).  Every device timing is one whole call between the context's HIP
events (gf2_timer_*: tables, launches and the copy back of the counts); after a warm-up the paths alternate and the median of the
repeats is reported.  `--one ft|ec` runs one enumeration once (for a kernel trace)."""
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_css_codes_amd import _native, ec_noise, ft_noise  # noqa: E402
from quantum_css_codes_amd.css_code import CSSCode  # noqa: E402

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
REPEATS = 5
SAMPLES = 1 << 22
P = (0.0002, 0.0001, 0.0002)
BUDGET = 1 << 40


def timed(ctx, fn, work):
    ctx.timer_start()
    fn()
    return work / (ctx.timer_stop() * 1e-3)


def main():
    ctx = _native.default_context()
    code = CSSCode(STEANE, STEANE)
    prog = ft_noise.program_for(code, "XXX")
    cycle = ec_noise.circuit_for(code, 1)
    work = {"ft": 9 * math.comb(prog.num_locations, 2), "ec": 27 * math.comb(cycle.num_locations, 3), "ft_mc": SAMPLES, "ec_mc": SAMPLES}
    paths = {"ft": lambda: prog.enumerate_strata([2], max_configurations=BUDGET),
             "ec": lambda: cycle.enumerate_strata([3], max_configurations=BUDGET),
             "ft_mc": lambda: prog.measurement_error_rates(SAMPLES, *P, seed=1),
             "ec_mc": lambda: cycle.logical_error_rates(SAMPLES, *P, seed=1)}
    if len(sys.argv) > 2 and sys.argv[1] == "--one":
        paths[sys.argv[2]]()
        ctx.sync()
        return
    for fn in paths.values():                                               # warm-up: tables, code objects
        fn()
    got = {key: [] for key in paths}
    for _ in range(REPEATS):                                                 # alternate
        for key, fn in paths.items():
            got[key].append(timed(ctx, fn, work[key]))
    med = {key: statistics.median(vals) for key, vals in got.items()}
    host = {}
    for key, gadget, w, ranks in (("ft", prog, 2, 1 << 18), ("ec", cycle, 3, 1 << 17)):
        first = math.comb(gadget.num_locations, w) // 2
        start = time.perf_counter()
        gadget.enumerate_strata([w], first_rank=first, count=ranks, host=True)
        host[key] = ranks * 3**w / (time.perf_counter() - start)
    ft, ec = paths["ft"]().counts[0], paths["ec"]().counts[0]
    print("steane XXX L=%d ldr=%d w=2: gf2_ft_enumerate %.4g configurations (%d accepted, %d wrong), %.3e /s (%.3e .. %.3e); host statement "
          "%.3e /s; gf2_mc_ft_decode %.3e samples/s (%.3e .. %.3e); median of %d"
          % (prog.num_locations, prog.ldr, work["ft"], int(ft[:, :, 0].sum()), int(ft[:, :, 1].sum()), med["ft"], min(got["ft"]), max(got["ft"]),
             host["ft"], med["ft_mc"], min(got["ft_mc"]), max(got["ft_mc"]), REPEATS), flush=True)
    print("steane cycle rounds=1 L=%d ldr=%d w=3: gf2_ec_enumerate %.4g configurations (%d accepted, %d logical_any), %.3e /s (%.3e .. %.3e); "
          "host statement %.3e /s; gf2_mc_ec_decode %.3e samples/s (%.3e .. %.3e); median of %d"
          % (cycle.num_locations, cycle.ldr, work["ec"], int(ec[:, :, 0].sum()), int(ec[:, :, 3].sum()), med["ec"], min(got["ec"]), max(got["ec"]),
             host["ec"], med["ec_mc"], min(got["ec_mc"]), max(got["ec_mc"]), REPEATS), flush=True)


if __name__ == "__main__":
    main()
