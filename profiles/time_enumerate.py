#!/usr/bin/env python3
"""Exact strata against the stratified sampler of the same build, in one process (DESIGN.md "Exact strata"): configurations per second
of gf2_circuit_enumerate and samples per second of gf2_mc_circuit_decode_strata on the same circuit and weight -- the Steane
encode_zero circuit (L = 21, effects staged in LDS) at w = 4 (4.8 x 10^5 configurations: mostly the call's fixed cost) and w = 8, and the 1025-location circuit of tests/test_gpu_strata.py (effects
through L2) at w = 3.  The sampler draws as many samples as the stratum has configurations (at most 2^30).  Every timing is one
call between the context's HIP events (gf2_timer_*: tables, launches and the copy back of the counts); after a warm-up the two
alternate and the median of the rounds is reported.  `--one enumerate|sampler CASE` runs one path once (for a kernel trace)."""
import math
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_css_codes_amd import _native, circuit_noise  # noqa: E402
from quantum_css_codes_amd.css_code import CSSCode  # noqa: E402

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
ROUNDS = 5


def long_gates():
    rng = np.random.default_rng(5)
    rows = []
    for g in range(525):
        a, b = rng.choice(7, 2, replace=False)
        rows.append((circuit_noise.GATE_IDLE, a, 0) if g % 21 == 0 else (circuit_noise.GATE_CNOT, a, b))
    return np.array(rows, dtype=np.int32)


def cases(code):
    return {"steane-encode_zero-w4": (circuit_noise.circuit_for(code, code.encode_zero_gates()), 4),
            "steane-encode_zero-w8": (circuit_noise.circuit_for(code, code.encode_zero_gates()), 8),
            "1025-locations-w3": (circuit_noise.circuit_for(code, long_gates()), 3)}


def paths_of(circ, w):
    configs = 3**w * math.comb(circ.num_locations, w)
    samples = min(configs, 1 << 30)
    return configs, samples, {"enumerate": lambda: circ.enumerate_strata([w], max_configurations=1 << 40),
                              "sampler": lambda: circ.logical_error_strata([w], samples, seed=1)}


def timed(ctx, fn, work):
    ctx.timer_start()
    fn()
    return work / (ctx.timer_stop() * 1e-3)


def main():
    ctx = _native.default_context()
    code = CSSCode(STEANE, STEANE)
    if len(sys.argv) > 3 and sys.argv[1] == "--one":
        circ, w = cases(code)[sys.argv[3]]
        paths_of(circ, w)[2][sys.argv[2]]()
        return
    for name, (circ, w) in cases(code).items():
        configs, samples, paths = paths_of(circ, w)
        work = {"enumerate": configs, "sampler": samples}
        for fn in paths.values():                                           # warm-up: tables, code objects
            fn()
        got = {key: [] for key in paths}
        for _ in range(ROUNDS):                                             # alternate
            for key, fn in paths.items():
                got[key].append(timed(ctx, fn, work[key]))
        med = {key: statistics.median(vals) for key, vals in got.items()}
        print("%s L=%d w=%d: enumerate %.4g configurations, %.3e /s (%.3e .. %.3e); sampler %.4g samples, %.3e /s (%.3e .. %.3e); "
              "median of %d; enumerate/sampler = %.2f" % (name, circ.num_locations, w, configs, med["enumerate"], min(got["enumerate"]),
                                                          max(got["enumerate"]), samples, med["sampler"], min(got["sampler"]),
                                                          max(got["sampler"]), ROUNDS, med["enumerate"] / med["sampler"]), flush=True)


if __name__ == "__main__":
    main()
