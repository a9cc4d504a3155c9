#!/usr/bin/env python3
"""The result of DESIGN.md section 5d "Repeat-until-success under gate-level faults", regenerated: the Reed-Muller [[15,1,3]] program
with no gate at depolarising gate faults p_1 = p_2 = 3.0e-3 and 3.2e-3 through the retried route (gf2_mc_retry_gate_decode), `wrong`
per accepted sample with its binomial standard error, beside the figures the direct post-selected sampler logged from 2^32 samples per
rate (profiles/gate_mc_results.log, DESIGN.md section 5e "Direct Monte-Carlo under gate-level faults") and the z of each
difference.  `--samples N` sets the samples per rate (default 2^26: the retried standard error, sqrt(r / N) = 5.4e-6 and 5.8e-6, is
then below the logged 7.4e-6 and 9.2e-6).  The lines are appended to profiles/retry_gate_results.log."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_css_codes_amd import _native, stream_noise  # noqa: E402
from quantum_css_codes_amd.css_code import CSSCode  # noqa: E402

# p: (rate, standard error) of `wrong` per accepted sample, the direct sampler's
LOGGED = {3.0e-3: (1.9916e-3, 0.0074e-3), 3.2e-3: (2.2762e-3, 0.0092e-3)}


def rm15_checks():
    cols = np.arange(1, 16)
    h1 = np.array([(cols >> b) & 1 for b in range(4)])
    return h1, np.vstack([h1] + [h1[a] & h1[b] for a in range(4) for b in range(a + 1, 4)])


def main():
    samples = int(sys.argv[sys.argv.index("--samples") + 1]) if "--samples" in sys.argv else 1 << 26
    log = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "retry_gate_results.log"), "a")

    def say(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    ctx = _native.default_context()
    gadget = stream_noise.stream_for(CSSCode(*rm15_checks()), "program", ())
    for p, (want, want_se) in LOGGED.items():
        ctx.timer_start()
        got = gadget.retry_gate_error_rates(samples, p, p, seed=51)
        secs = ctx.timer_stop() * 1e-3
        rate = got['wrong'] / got['accepted']
        se = math.sqrt(rate * (1.0 - rate) / got['accepted'])
        say("rm15 '' MEASURE, p_1 = p_2 = %g, retried: %d samples, %d accepted, %d exhausted, %.4f attempts per preparation, %.2f s; wrong %d = "
            "%.4fe-3 +- %.4fe-3 per accepted sample; direct sampler (logged) %.4fe-3 +- %.4fe-3; z of the difference %+.2f"
            % (p, samples, got['accepted'], got['exhausted'], got['attempts'] / (samples * got['preparations']), secs, got['wrong'], rate * 1e3,
               se * 1e3, want * 1e3, want_se * 1e3, (rate - want) / math.hypot(se, want_se)))


if __name__ == "__main__":
    main()
