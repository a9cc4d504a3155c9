#!/usr/bin/env python3
"""Circuit-level fault Monte-Carlo against the code-capacity path it was modelled on, in one process: five runs each, alternating,
of CSSCode.encoder_logical_error_rates('zero', ...) and CSSCode.logical_error_rates on the same code object, same count and rates
(p = 10^-3 per kind), wall clock around calls that end in a device-to-host copy, after a warm-up.  Also the idle circuit (one IDLE
gate per qubit), which draws exactly what the code-capacity path draws.  `--one NAME` runs the encoder once (for a kernel trace)."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_css_codes_amd import bin_matrix, circuit_noise  # noqa: E402
from quantum_css_codes_amd.css_code import CSSCode  # noqa: E402

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])


def dual_pair(rng, n, r1):
    while True:
        h1 = rng.integers(0, 2, (r1, n))
        if bin_matrix.rank(h1) == r1:
            break
    null = bin_matrix.nullspace(h1)
    return h1, null[: null.shape[0] - 1]


def make(name):
    if name == "steane":
        return CSSCode(STEANE, STEANE), 10**8
    n, r1, cap = {"63": (63, 31, None), "127": (127, 63, 2)}[name]
    return CSSCode(*dual_pair(np.random.default_rng(n + r1), n, r1), max_table_weight=cap), 10**7


def rates(fn, count, runs=5):
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        out.append(count / (time.perf_counter() - t0))
    return out


def main():
    p = (1e-3, 1e-3, 1e-3)
    if len(sys.argv) > 2 and sys.argv[1] == "--one":
        code, count = make(sys.argv[2])
        code.encoder_logical_error_rates('zero', count, *p, seed=1)
        code.logical_error_rates(count, *p, seed=1)
        return
    for name in ("steane", "63", "127"):
        code, count = make(name)
        gates = code.encode_zero_gates()
        idle = [(2, q, 0) for q in range(code.n)]
        total = circuit_noise.circuit_for(code, gates).num_locations
        paths = {"encoder": lambda: code.encoder_logical_error_rates('zero', count, *p, seed=1),
                 "capacity": lambda: code.logical_error_rates(count, *p, seed=1),
                 "idle": lambda: code.circuit_logical_error_rates(idle, count, *p, seed=1)}
        for fn in paths.values():                                           # warm-up: tables, workspaces, code objects
            fn()
        got = {key: [] for key in paths}
        for _ in range(5):                                                  # alternate
            for key, fn in paths.items():
                got[key] += rates(fn, count, runs=1)
        line = "n=%3d L=%5d (L/n = %.1f) %.0e samples:" % (code.n, total, total / code.n, count)
        for key, vals in got.items():
            line += "  %s min/median/max %.3e / %.3e / %.3e per s;" % (key, min(vals), statistics.median(vals), max(vals))
        line += "  capacity/encoder = %.2f, capacity/idle = %.2f" % (statistics.median(got["capacity"]) / statistics.median(got["encoder"]),
                                                                   statistics.median(got["capacity"]) / statistics.median(got["idle"]))
        print(line, flush=True)


if __name__ == "__main__":
    main()
