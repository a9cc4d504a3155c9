#!/usr/bin/env python3
"""The repeat-until-success tally against the post-selected streamed tally of the same build, in one process (DESIGN.md section 5d
"Repeat-until-success"): accepted samples per second of gf2_mc_retry_decode and of gf2_mc_stream_decode on Steane cycles of 1, 5, 50
and 1000 rounds at p_x = p_y = p_z = 1e-4 and 1e-3, and the mean attempts per preparation beside the exact value, the mean of 1 / q
over the cycle's two preparations (q from the exact distribution of a preparation's flags, computed here from the block table).
Every timing is one whole call between the context's HIP events (gf2_timer_*: tables, launches and the copy back of the counts);
after a warm-up the two routes alternate and the median of the repeats is reported.  A route that accepts no sample of a run has
no rate: the line says so."""
import math
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_css_codes_amd import _native, stream_noise  # noqa: E402
from quantum_css_codes_amd.css_code import CSSCode  # noqa: E402

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
REPEATS = 5
CASES = ((1, 1 << 24), (5, 1 << 23), (50, 1 << 21), (1000, 1 << 17))              # rounds, samples
RATES = (1e-4, 1e-3)


def pass_probability(block, region, p):
    """P(no flag row of one attempt of the region fires): the product over the subsets s of flag rows of the characters, by the
    Walsh-Hadamard identity P(0) = 2^-m sum_s prod_l (1 - 2 P(s . f_l = 1)) with f_l the flags of location l's fault."""
    first, count, _ = (int(v) for v in block.regions[region])
    flags = block.effects[first:first + count, :, 2]
    mask = int(np.bitwise_or.reduce(flags.reshape(-1)))
    low = (mask & -mask).bit_length() - 1
    f_x, f_z = (flags[:, 0] >> np.uint64(low)).astype(np.int64), (flags[:, 1] >> np.uint64(low)).astype(np.int64)
    m = (mask >> low).bit_length()
    total = 0.0
    for s in range(1 << m):
        par = lambda f: np.array([bin(int(v) & s).count("1") & 1 for v in f])
        odd_x, odd_z = par(f_x), par(f_z)
        odd = p * (odd_x + odd_z + (odd_x ^ odd_z))                              # X, Z and Y faults that flip s . f
        total += math.exp(float(np.log1p(-2.0 * odd).sum()))
    return total / (1 << m)


def timed(ctx, fn):
    ctx.timer_start()
    out = fn()
    return out, ctx.timer_stop() * 1e-3


def main():
    ctx = _native.default_context()
    steane = CSSCode(STEANE, STEANE)
    block = stream_noise.stream_for(steane, "cycle", (1, False)).types[0]
    preps = [r for r, row in enumerate(block.regions.tolist()) if row[2]]
    for p in RATES:
        inverse = statistics.mean(1.0 / pass_probability(block, r, p) for r in preps)
        for rounds, samples in CASES:
            gadget = stream_for(steane, rounds)
            paths = {"retried": lambda: gadget.retry_error_rates(samples, p, p, p, seed=1),
                     "post-selected": lambda: gadget.error_rates(samples, p, p, p, seed=1)}
            got = {key: fn() for key, fn in paths.items()}                      # warm-up: tables, code objects; and the counts
            secs = {key: [] for key in paths}
            for _ in range(REPEATS):                                             # alternate
                for key, fn in paths.items():
                    secs[key].append(timed(ctx, fn)[1])
            rate = {key: got[key]['accepted'] / statistics.median(secs[key]) for key in paths}
            retried = got["retried"]
            ratio = "%.3g" % (rate["retried"] / rate["post-selected"]) if rate["post-selected"] > 0 else "no post-selected sample accepted"
            print("steane cycle, %d rounds, p_kind %g: %d samples; retried %d accepted (%d exhausted), %.4f attempts per preparation (exact "
                  "1/q: %.4f), %.3e accepted /s (%.3e .. %.3e); post-selected %d accepted, %.3e accepted /s (%.3e .. %.3e); "
                  "retried / post-selected = %s; median of %d"
                  % (rounds, p, samples, retried['accepted'], retried['exhausted'],
                     retried['attempts'] / (samples * retried['preparations']), inverse, rate["retried"],
                     retried['accepted'] / max(secs["retried"]), retried['accepted'] / min(secs["retried"]), got["post-selected"]['accepted'],
                     rate["post-selected"], got["post-selected"]['accepted'] / max(secs["post-selected"]),
                     got["post-selected"]['accepted'] / min(secs["post-selected"]), ratio, REPEATS), flush=True)


def stream_for(code, rounds):
    return stream_noise.stream_for(code, "cycle", (rounds, False))


if __name__ == "__main__":
    main()
