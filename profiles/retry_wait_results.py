#!/usr/bin/env python3
"""The results of DESIGN.md section 5d "Repeat-until-success with waiting faults", regenerated: what the retries cost the waiting data
block.  (a) The Steane cycle at 100 rounds, p_x = p_y = p_z = p_kind = 1e-4 and 1e-3, memory error rates q_kind in {0, p/10, p, 10 p}:
logical_x, logical_z and logical_any per accepted sample and, for either side, the rate per round r that solves f = (1 - (1 - 2 r)^rounds)
/ 2 -- or "saturated" when f is within five standard errors of 1/2, as it is after 100 rounds at p_kind = 1e-3 and q = 10 p, which is
why that rate is also run at 10 rounds.  Every q = 0 row is checked against the plain retried route's counts of the same seed for
equality.  (b) The Reed-Muller [[15,1,3]] program with no gate at p_kind = 1e-3 and 3e-3, the same q: `wrong` per accepted sample
beside the bare qubit's raw_program_error_rate.  `--samples N` sets the samples per row of (a) (default 2^28; (b) takes a quarter).
The lines are appended to profiles/retry_wait_results.log."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_css_codes_amd import _native, ft_noise, stream_noise  # noqa: E402
from quantum_css_codes_amd.css_code import CSSCode  # noqa: E402

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
CYCLES = ((1e-4, 100), (1e-3, 100), (1e-3, 10))                                   # p_kind, rounds


def rm15_checks():
    cols = np.arange(1, 16)
    h1 = np.array([(cols >> b) & 1 for b in range(4)])
    return h1, np.vstack([h1] + [h1[a] & h1[b] for a in range(4) for b in range(a + 1, 4)])


def main():
    samples = int(sys.argv[sys.argv.index("--samples") + 1]) if "--samples" in sys.argv else 1 << 28
    log = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "retry_wait_results.log"), "a")

    def say(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    ctx = _native.default_context()
    steane = CSSCode(STEANE, STEANE)

    def per_round(errors, accepted, rounds):
        f = errors / accepted
        se = math.sqrt(f * (1.0 - f) / accepted)
        return "saturated" if 0.5 - f < 5.0 * se else "%.4e" % (0.5 * (1.0 - (1.0 - 2.0 * f) ** (1.0 / rounds)))

    for p, rounds in CYCLES:
        cycle = stream_noise.stream_for(steane, "cycle", (rounds, False))
        plain = cycle.retry_error_rates(samples, p, p, p, seed=61)
        for factor in (0.0, 0.1, 1.0, 10.0):
            q = factor * p
            ctx.timer_start()
            got = cycle.retry_wait_error_rates(samples, p, p, p, q, q, q, seed=61)
            secs = ctx.timer_stop() * 1e-3
            if factor == 0.0:
                assert all(got[key] == plain[key] for key in plain) and got['wait_faults'] == 0, "q = 0 must give the plain retried route's counts"
            n = got['accepted']
            say("steane cycle, %d rounds, p_kind %g, q_kind %g%s: %d samples, %d accepted, %.4f attempts per preparation, %.4f wait faults per "
                "sample, %.2f s; per accepted sample logical_x %.4e, logical_z %.4e, logical_any %.4e +- %.1e; per round x %s, z %s"
                % (rounds, p, q, " (counts equal to the plain retried route's)" if factor == 0.0 else "", samples, n,
                   got['attempts'] / (samples * got['preparations']), got['wait_faults'] / samples, secs, got['logical_x'] / n, got['logical_z'] / n,
                   got['logical_any'] / n, math.sqrt(got['logical_any'] / n * (1.0 - got['logical_any'] / n) / n),
                   per_round(got['logical_x'], n, rounds), per_round(got['logical_z'], n, rounds)))
    program = stream_noise.stream_for(CSSCode(*rm15_checks()), "program", ())
    for p in (1e-3, 3e-3):
        bare = ft_noise.raw_program_error_rate((), p, p, p)
        for factor in (0.0, 0.1, 1.0, 10.0):
            q = factor * p
            ctx.timer_start()
            got = program.retry_wait_error_rates(samples // 4, p, p, p, q, q, q, seed=62)
            secs = ctx.timer_stop() * 1e-3
            f = got['wrong'] / got['accepted']
            se = math.sqrt(f * (1.0 - f) / got['accepted'])
            say("rm15 '' MEASURE, p_kind %g, q_kind %g: %d samples, %d accepted, %d exhausted, %.4f attempts per preparation, %.4f wait faults per "
                "sample, %.2f s; wrong %d = %.4e +- %.1e per accepted sample; bare qubit %.4e; encoded / bare = %.3f"
                % (p, q, samples // 4, got['accepted'], got['exhausted'], got['attempts'] / (samples // 4 * got['preparations']),
                   got['wait_faults'] / (samples // 4), secs, got['wrong'], f, se, bare, f / bare))


if __name__ == "__main__":
    main()
