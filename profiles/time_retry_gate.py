#!/usr/bin/env python3
"""The repeat-until-success tally under gate-level faults against its two neighbours of the same build, in one process (DESIGN.md
section 5d "Repeat-until-success under gate-level faults", "Speed"): accepted samples per second of gf2_mc_retry_gate_decode
  - against the post-selected gate sampler (gf2_mc_ec_decode_gate / gf2_mc_ft_decode_gate of gf2_gate_mc.hip) at the same p_1 = p_2:
    the Reed-Muller [[15,1,3]] program with no gate at 3e-3, the one-round Steane cycle at 1e-3 and 3.2e-3;
  - against the location version (gf2_mc_retry_decode) at the rate per location that gives the same expected number of faults per
    sample, p (n_1 + n_2) / L split evenly over X, Y, Z: Steane cycles of 1, 50 and 1000 rounds at p = 1e-3.
Every timing is one whole call between the context's HIP events (gf2_timer_*: tables, launches and the copy back of the counts); after
a warm-up the two routes of a row alternate and the median of the repeats is reported with min and max.  The lines are appended to
profiles/time_retry_gate.log."""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_css_codes_amd import _native, ec_noise, ft_noise, stream_noise  # noqa: E402
from quantum_css_codes_amd.css_code import CSSCode  # noqa: E402

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
REPEATS = 5


def rm15_checks():
    cols = np.arange(1, 16)
    h1 = np.array([(cols >> b) & 1 for b in range(4)])
    return h1, np.vstack([h1] + [h1[a] & h1[b] for a in range(4) for b in range(a + 1, 4)])


def timed(ctx, fn):
    ctx.timer_start()
    fn()
    return ctx.timer_stop() * 1e-3


def compare(ctx, say, name, paths):
    """paths: two (label, fn) whose fn returns a dict with 'accepted'; the first is the new kernel."""
    got = {key: fn() for key, fn in paths}                                     # warm-up: tables, code objects; and the counts
    secs = {key: [] for key, _ in paths}
    for _ in range(REPEATS):                                                    # alternate
        for key, fn in paths:
            secs[key].append(timed(ctx, fn))
    rate = {key: got[key]['accepted'] / statistics.median(secs[key]) for key, _ in paths}
    parts = []
    for key, _ in paths:
        extra = ", %.4f attempts per preparation, %d exhausted" % (got[key]['attempts'] / (got[key]['samples'] * got[key]['preparations']),
                                                                   got[key]['exhausted']) if 'attempts' in got[key] else ""
        parts.append("%s: %d samples, %d accepted%s, %.3e accepted /s (%.3e .. %.3e)"
                     % (key, got[key]['samples'], got[key]['accepted'], extra, rate[key], got[key]['accepted'] / max(secs[key]),
                        got[key]['accepted'] / min(secs[key])))
    (new, _), (old, _) = paths
    ratio = "%.3g" % (rate[new] / rate[old]) if rate[old] > 0 else "no sample accepted by the other route"
    say("%s; %s; %s / %s = %s; median of %d" % (name, "; ".join(parts), new, old, ratio, REPEATS))


def main():
    ctx = _native.default_context()
    log = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "time_retry_gate.log"), "a")

    def say(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    steane, rm15 = CSSCode(STEANE, STEANE), CSSCode(*rm15_checks())
    # against post-selection at the same rates
    program, selected = stream_noise.stream_for(rm15, "program", ()), ft_noise.program_for(rm15, "")
    compare(ctx, say, "rm15 '' MEASURE, p_1 = p_2 = 0.003",
            (("retried gates", lambda: program.retry_gate_error_rates(1 << 22, 3e-3, 3e-3, seed=1)),
             ("post-selected gates", lambda: selected.gate_error_rates(1 << 30, 3e-3, 3e-3, seed=1))))
    cycle, resident = stream_noise.stream_for(steane, "cycle", (1, False)), ec_noise.circuit_for(steane, 1)
    for p in (1e-3, 3.2e-3):
        compare(ctx, say, "steane cycle, 1 round, p_1 = p_2 = %g" % p,
                (("retried gates", lambda: cycle.retry_gate_error_rates(1 << 26, p, p, seed=1)),
                 ("post-selected gates", lambda: resident.gate_error_rates(1 << 30, p, p, seed=1))))
    # against the location version at the same expected number of faults per sample
    for rounds, samples in ((1, 1 << 24), (50, 1 << 21), (1000, 1 << 17)):
        gadget = stream_noise.stream_for(steane, "cycle", (rounds, False))
        p = 1e-3
        each = p * len(gadget.type_site_loc) / len(gadget.type_eff) / 3.0       # one block type: sites and locations of a round
        compare(ctx, say, "steane cycle, %d rounds, %.3g faults per sample" % (rounds, p * len(gadget.type_site_loc) * rounds),
                (("retried gates p = %g" % p, lambda: gadget.retry_gate_error_rates(samples, p, p, seed=1)),
                 ("retried locations p_kind = %.4g" % each, lambda: gadget.retry_error_rates(samples, each, each, each, seed=1))))
    log.close()


if __name__ == "__main__":
    main()
