#!/usr/bin/env python3
"""Stratified kernels against the binomial ones of the same build, in one process: gf2_mc_decode_strata at weight w against
gf2_mc_decode_hashed at p_t = w / n (the same mean number of errors per sample; the binomial kernel additionally walks a CDF table
and its lanes run different trip counts), and gf2_mc_circuit_decode_strata against gf2_mc_circuit_decode on the code's encode_zero
circuit at p_t = w / L.  Codes: Steane, RM15 and the n = 63 pair of tests/test_gpu_tables.py.  Every timing is one call of 10^8
samples between the context's HIP events (gf2_timer_*: tables, kernel and the copy back of the counts); after a warm-up of each
path the two alternate, and the median of the rounds is reported.  `--one NAME W` runs each of the four paths once (for a kernel
trace)."""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_css_codes_amd import _native, bin_matrix, circuit_noise, montecarlo  # noqa: E402
from quantum_css_codes_amd.css_code import CSSCode  # noqa: E402

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
COUNT = 10**8
ROUNDS = 7


def dual_pair(rng, n, r1):
    while True:
        h1 = rng.integers(0, 2, (r1, n))
        if bin_matrix.rank(h1) == r1:
            break
    null = bin_matrix.nullspace(h1)
    return h1, null[: null.shape[0] - 1]


def make(name):
    if name == "steane":
        return CSSCode(STEANE, STEANE)
    if name == "rm15":
        cols = np.arange(1, 16)
        h1 = np.array([(cols >> b) & 1 for b in range(4)])
        return CSSCode(h1, np.vstack([h1] + [h1[a] & h1[b] for a in range(4) for b in range(a + 1, 4)]))
    return CSSCode(*dual_pair(np.random.default_rng(63 + 31), 63, 31))


def paths_of(code, w):
    total = circuit_noise.circuit_for(code, code.encode_zero_gates()).num_locations
    p, pc = w / code.n / 3, w / total / 3
    return total, {
        "strata": lambda: code.logical_error_strata([w], COUNT, seed=1),
        "hashed": lambda: montecarlo.decode_local(code, COUNT, p, p, p, seed=1, hashed=True),
        "circuit strata": lambda: code.encoder_logical_error_strata('zero', [w], COUNT, seed=1),
        "circuit": lambda: code.encoder_logical_error_rates('zero', COUNT, pc, pc, pc, seed=1)}


def timed(ctx, fn):
    ctx.timer_start()
    fn()
    return COUNT / (ctx.timer_stop() * 1e-3)


def main():
    ctx = _native.default_context()
    if len(sys.argv) > 3 and sys.argv[1] == "--one":
        for fn in paths_of(make(sys.argv[2]), int(sys.argv[3]))[1].values():
            fn()
        return
    for name in ("steane", "rm15", "63"):
        code = make(name)
        for w in (1, 2, 4):
            total, paths = paths_of(code, w)
            for fn in paths.values():                                       # warm-up: tables, code objects, the sampler's tables
                fn()
            got = {key: [] for key in paths}
            for _ in range(ROUNDS):                                         # alternate
                for key, fn in paths.items():
                    got[key].append(timed(ctx, fn))
            med = {key: statistics.median(vals) for key, vals in got.items()}
            line = "n=%3d L=%4d w=%d, %.0e samples, median of %d (min .. max) samples/s:" % (code.n, total, w, COUNT, ROUNDS)
            for key, vals in got.items():
                line += "  %s %.3e (%.3e .. %.3e);" % (key, med[key], min(vals), max(vals))
            line += "  strata/hashed = %.2f, circuit strata/circuit = %.2f" % (med["strata"] / med["hashed"], med["circuit strata"] / med["circuit"])
            print(line, flush=True)


if __name__ == "__main__":
    main()
