#!/usr/bin/env python3
"""The gate-level repeat-until-success tally with waiting faults against the gate-level retried tally of the same build, in one process
(DESIGN.md section 5d "Repeat-until-success with waiting faults under gate-level faults"): accepted samples per second of
gf2_mc_retry_gate_wait_decode at q = 0 and at q = p_1 / 3 per kind and of gf2_mc_retry_gate_decode on Steane cycles of 1, 50 and 1000
rounds at p_1 = p_2 = 1e-3.  At q = 0 the two kernels draw the same samples (the fourteen counts are compared here), so that ratio is
the pure price of the extra draw per attempt.  Every timing is one whole call between the context's HIP events (gf2_timer_*: tables,
launches and the copy back of the counts); after a warm-up the three routes alternate and the median of the repeats is reported with
min and max.  The lines are appended to profiles/time_retry_gate_wait.log."""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_css_codes_amd import _native, stream_noise  # noqa: E402
from quantum_css_codes_amd.css_code import CSSCode  # noqa: E402

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
REPEATS = 5
CASES = ((1, 1 << 24), (50, 1 << 21), (1000, 1 << 17))                            # rounds, samples: profiles/time_retry_gate.py's
P = 1e-3


def main():
    log = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "time_retry_gate_wait.log"), "a")
    ctx = _native.default_context()
    steane = CSSCode(STEANE, STEANE)
    for rounds, samples in CASES:
        gadget = stream_noise.stream_for(steane, "cycle", (rounds, False))
        q = P / 3.0
        paths = {"plain": lambda: gadget.retry_gate_counts(samples, P, P, seed=1),
                 "q = 0": lambda: gadget.retry_gate_wait_counts(samples, P, P, 0.0, 0.0, 0.0, seed=1),
                 "q = p/3": lambda: gadget.retry_gate_wait_counts(samples, P, P, q, q, q, seed=1)}
        got = {key: [int(v) for v in fn()] for key, fn in paths.items()}        # warm-up: tables, code objects; and the counts
        assert got["q = 0"] == got["plain"] + [0], "q = 0 must draw the gate-level retried route's samples"
        assert got["q = p/3"][12:14] == got["plain"][12:14]
        secs = {key: [] for key in paths}
        for _ in range(REPEATS):                                                 # alternate
            for key, fn in paths.items():
                ctx.timer_start()
                fn()
                secs[key].append(ctx.timer_stop() * 1e-3)
        rate = {key: got[key][0] / statistics.median(secs[key]) for key in paths}
        span = lambda key: "%.3e accepted /s (%.3e .. %.3e)" % (rate[key], got[key][0] / max(secs[key]), got[key][0] / min(secs[key]))
        text = ("steane cycle, %d rounds, p_1 = p_2 = %g: %d samples, %.4f attempts per preparation; gate-level retried %s; waiting faults at "
                "q = 0 %s, at q_kind = p_1 / 3 %s (%.4f wait faults per sample); q = 0 / plain = %.3f, q = p/3 / plain = %.3f; median of %d"
                % (rounds, P, samples, got["plain"][13] / (samples * gadget.preparations), span("plain"), span("q = 0"), span("q = p/3"),
                   got["q = p/3"][14] / samples, rate["q = 0"] / rate["plain"], rate["q = p/3"] / rate["plain"], REPEATS))
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()


if __name__ == "__main__":
    main()
