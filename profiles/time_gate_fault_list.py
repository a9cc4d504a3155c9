#!/usr/bin/env python3
"""The gate-level listing kernel against the counting kernel of the same build on the same ranges, in one process (DESIGN.md section
5e "Malignant fault sets under gate-level faults"): configurations per second of gf2_ec_gate_enumerate_list (select: a logical flip)
against gf2_ec_gate_enumerate on the one-round Steane cycle (126 + 102 sites, ldr = 3) at (w, b) = (3, 1) (1.1 x 10^8
configurations), and of gf2_ft_gate_enumerate_list (select: wrong) against gf2_ft_gate_enumerate on the gate-free Steane program
(603 + 491 sites, ldr = 8) at weight 2, the three b one after the other (4.2 x 10^7).  Every timing is one whole call (or the three
of a weight) between the context's HIP events (gf2_timer_*: tables, launches, the copy back and, for a list, the sort on the host);
the list is called with room for exactly its records.  After a warm-up the paths alternate and the median of the repeats is reported
with the extremes; one more call of each path with the context's per-launch events on (gf2_profile_*) gives the time of its launches
alone."""
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


def timed(ctx, fn, work):
    ctx.timer_start()
    fn()
    return work / (ctx.timer_stop() * 1e-3)


def main():
    ctx = _native.default_context()
    code = CSSCode(STEANE, STEANE)
    cycle, prog = ec_noise.circuit_for(code, 1), ft_noise.program_for(code, "")
    ec_sites, ft_sites = cycle.gate_sites()[:3], prog.gate_sites()[:3]
    ec_args = (cycle.device(), cycle.rounds) + tuple(cycle._tables()) + tuple(ec_sites)
    ft_args = (prog.device(), prog.nsteps, prog.measure_mask) + tuple(prog._tables()) + tuple(ft_sites)
    total = lambda sites, w, b: math.comb(sites[1], w - b) * math.comb(sites[2], b)
    ec_total = total(ec_sites, 3, 1)
    ft_totals = [total(ft_sites, 2, b) for b in range(3)]
    ec_found = ctx.ec_gate_enumerate_list(*ec_args, 3, 1, 0, ec_total, EC_FLIPS, 0)[0]
    ft_found = [ctx.ft_gate_enumerate_list(*ft_args, 2, b, 0, ft_totals[b], ft_noise.CLASS_WRONG, 0)[0] for b in range(3)]
    ec_work, ft_work = 9 * 15 * ec_total, sum(n * 3**(2 - b) * 15**b for b, n in enumerate(ft_totals))
    work = {"ec": ec_work, "ec_list": ec_work, "ft": ft_work, "ft_list": ft_work}
    paths = {"ec": lambda: ctx.ec_gate_enumerate(*ec_args, 3, 1, 0, ec_total),
             "ec_list": lambda: ctx.ec_gate_enumerate_list(*ec_args, 3, 1, 0, ec_total, EC_FLIPS, ec_found),
             "ft": lambda: [ctx.ft_gate_enumerate(*ft_args, 2, b, 0, ft_totals[b]) for b in range(3)],
             "ft_list": lambda: [ctx.ft_gate_enumerate_list(*ft_args, 2, b, 0, ft_totals[b], ft_noise.CLASS_WRONG, ft_found[b]) for b in range(3)]}
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
    for name, where, count, list_key, found, flips in (("steane cycle rounds=1", "(w, b) = (3, 1)", "ec", "ec_list", ec_found, int(ec[:, 3].sum())),
                                                       ("steane program ''", "w = 2, b = 0, 1, 2", "ft", "ft_list", sum(ft_found),
                                                        sum(int(c[:, 1].sum()) for c in ft))):
        assert found == flips, (name, found, flips)                          # the list is as long as the counting kernel's count
        print("%s %s: %.4g configurations, %d listed (%.3g %%): counting %.3e /s (%.3e .. %.3e), listing %.3e /s (%.3e .. %.3e), "
              "listing / counting = %.3f; whole calls between HIP events, median of %d; of one call, the launches alone: counting %.3f ms of "
              "%.3f ms, listing %.3f ms of %.3f ms (the rest: tables, the copy back and the sort of %.1f MB of records on the host), "
              "launches alone listing / counting = %.3f"
              % (name, where, work[count], found, 100.0 * found / work[count], med[count], min(got[count]), max(got[count]), med[list_key],
                 min(got[list_key]), max(got[list_key]), med[list_key] / med[count], REPEATS, kernel[count], 1e3 * work[count] / med[count],
                 kernel[list_key], 1e3 * work[count] / med[list_key], 16e-6 * found, kernel[count] / kernel[list_key]), flush=True)


if __name__ == "__main__":
    main()
