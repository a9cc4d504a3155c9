#!/usr/bin/env python3
"""The listing kernel against the counting kernel of the same build on the same strata, in one process (DESIGN.md "Malignant fault
sets of the cycle" and "Malignant fault sets of the measurement"): configurations per second of gf2_ec_enumerate_list (select: a
logical flip) against gf2_ec_enumerate on the one-round Steane cycle (L = 330, ldr = 3) at w = 3 (1.6 x 10^8 configurations), and of
gf2_ft_enumerate_list (select: wrong) against gf2_ft_enumerate on the gate-free Reed-Muller [[15,1,3]] program (L = 3867, ldr = 9) at
w = 2 (6.7 x 10^7).  Every timing is one whole call between the context's HIP events (gf2_timer_*: tables, launches, the copy back
and, for a list, the sort on the host); the list is called with room for exactly its records.  After a warm-up the paths alternate
and the median of the repeats is reported with the extremes; one more call of each path with the context's per-launch events
on (gf2_profile_*) gives the time of its launches alone.  `--one ec|ec_list|ft|ft_list` runs one path once (for a kernel trace)."""
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
EC_FLIPS = ec_noise.CLASS_FLIP_X | ec_noise.CLASS_FLIP_Z


def rm15_checks():
    cols = np.arange(1, 16)
    h1 = np.array([(cols >> b) & 1 for b in range(4)])
    return h1, np.vstack([h1] + [h1[a] & h1[b] for a in range(4) for b in range(a + 1, 4)])


def timed(ctx, fn, work):
    ctx.timer_start()
    fn()
    return work / (ctx.timer_stop() * 1e-3)


def main():
    ctx = _native.default_context()
    cycle = ec_noise.circuit_for(CSSCode(STEANE, STEANE), 1)
    prog = ft_noise.program_for(CSSCode(*rm15_checks()), "")
    ec_total, ft_total = math.comb(cycle.num_locations, 3), math.comb(prog.num_locations, 2)
    ec_args = (cycle.device(), cycle.rounds) + tuple(cycle._tables())
    ft_args = (prog.device(), prog.nsteps, prog.measure_mask) + tuple(prog._tables())
    ec_found = ctx.ec_enumerate_list(*ec_args, 3, 0, ec_total, EC_FLIPS, 0)[0]
    ft_found = ctx.ft_enumerate_list(*ft_args, 2, 0, ft_total, ft_noise.CLASS_WRONG, 0)[0]
    work = {"ec": 27 * ec_total, "ec_list": 27 * ec_total, "ft": 9 * ft_total, "ft_list": 9 * ft_total}
    paths = {"ec": lambda: ctx.ec_enumerate(*ec_args, 3, 0, ec_total),
             "ec_list": lambda: ctx.ec_enumerate_list(*ec_args, 3, 0, ec_total, EC_FLIPS, ec_found),
             "ft": lambda: ctx.ft_enumerate(*ft_args, 2, 0, ft_total),
             "ft_list": lambda: ctx.ft_enumerate_list(*ft_args, 2, 0, ft_total, ft_noise.CLASS_WRONG, ft_found)}
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
    kernel = {}                                                              # of one more call each: its launches alone, between events of their own
    ctx.profile(True)
    for key, fn in paths.items():
        ctx.profile_reset()
        fn()
        kernel[key] = ctx.profile_get(_native.K_SAMPLER)[0]
    ctx.profile(False)
    ec, ft = paths["ec"](), paths["ft"]()
    for name, gadget, w, count, list_key, found, flips in (("steane cycle rounds=1", cycle, 3, "ec", "ec_list", ec_found, int(ec[:, :, 3].sum())),
                                                           ("rm15 program ''", prog, 2, "ft", "ft_list", ft_found, int(ft[:, :, 1].sum()))):
        assert found == flips, (name, found, flips)                          # the list is as long as the counting kernel's count
        print("%s L=%d ldr=%d w=%d: %.4g configurations, %d listed (%.3g %%): counting %.3e /s (%.3e .. %.3e), listing %.3e /s (%.3e .. %.3e), "
              "listing / counting = %.3f; whole calls between HIP events, median of %d; of one call, the launches alone: counting %.3f ms of "
              "%.3f ms, listing %.3f ms of %.3f ms (the rest: tables, the copy back and the sort of %.1f MB of records on the host)"
              % (name, gadget.num_locations, gadget.ldr, w, work[count], found, 100.0 * found / work[count], med[count], min(got[count]),
                 max(got[count]), med[list_key], min(got[list_key]), max(got[list_key]), med[list_key] / med[count], REPEATS, kernel[count],
                 1e3 * work[count] / med[count], kernel[list_key], 1e3 * work[count] / med[list_key], 16e-6 * found), flush=True)


if __name__ == "__main__":
    main()
