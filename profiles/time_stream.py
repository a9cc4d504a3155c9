#!/usr/bin/env python3
"""The streamed tally against the resident tallies of the same build, in one process (DESIGN.md "Streamed gadgets"): samples per
second of gf2_mc_stream_decode and of gf2_mc_ec_decode / gf2_mc_ft_decode on the same gadget, the same samples and the same rates
where both run -- the Steane cycle of 5 rounds, the Reed-Muller [[15,1,3]] cycle of 3 rounds, the Steane programs MEASURE and
X^7 MEASURE, 2^22 samples at p = (0.0002, 0.0001, 0.0002) -- with the two routes' counts compared; then gf2_mc_stream_decode alone
on Steane cycles of 5, 50, 500 and 3000 rounds at p = (2e-7, 1e-7, 1e-7), a rate at which most samples of the longest run are
accepted, so that no early exit of rejected samples shortens the walk: is the time per sample linear in the rounds?
Every timing is one whole call between the context's HIP events (gf2_timer_*: tables, launches and the copy back of the counts);
after a warm-up the routes alternate and the median of the repeats is reported."""
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_css_codes_amd import _native, ec_noise, ft_noise, stream_noise  # noqa: E402
from quantum_css_codes_amd.css_code import CSSCode  # noqa: E402

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
REPEATS = 5
SAMPLES = 1 << 22
P = (0.0002, 0.0001, 0.0002)
P_LONG = (2e-7, 1e-7, 1e-7)
LONG = ((5, 1 << 22), (50, 1 << 21), (500, 1 << 19), (3000, 1 << 17))           # rounds, samples


def rm15():
    cols = np.arange(1, 16)
    h1 = np.array([(cols >> b) & 1 for b in range(4)])
    return CSSCode(h1, np.vstack([h1] + [h1[a] & h1[b] for a in range(4) for b in range(a + 1, 4)]))


def timed(ctx, fn, samples):
    ctx.timer_start()
    fn()
    return samples / (ctx.timer_stop() * 1e-3)


def main():
    ctx = _native.default_context()
    steane = CSSCode(STEANE, STEANE)
    pairs = (("steane cycle, 5 rounds", stream_noise.stream_for(steane, "cycle", (5, False)), ec_noise.circuit_for(steane, 5)),
             ("rm15 cycle, 3 rounds", stream_noise.stream_for(rm15(), "cycle", (3, False)), None),
             ("steane program MEASURE", stream_noise.stream_for(steane, "program", ()), ft_noise.program_for(steane, "")),
             ("steane program X^7 MEASURE", stream_noise.stream_for(steane, "program", tuple("X" * 7)), ft_noise.program_for(steane, "X" * 7)))
    for name, gadget, resident in pairs:
        if resident is None:
            resident = ec_noise.circuit_for(gadget.code, 3)
        tally = resident.logical_error_rates if gadget.what == "cycle" else resident.measurement_error_rates
        paths = {"streamed": lambda: gadget.error_rates(SAMPLES, *P, seed=1), "resident": lambda: tally(SAMPLES, *P, seed=1)}
        same = paths["streamed"]() == paths["resident"]()                       # warm-up: tables, code objects; and the counts
        got = {key: [] for key in paths}
        for _ in range(REPEATS):                                                 # alternate
            for key, fn in paths.items():
                got[key].append(timed(ctx, fn, SAMPLES))
        med = {key: statistics.median(vals) for key, vals in got.items()}
        counts = paths["streamed"]()
        print("%s: L=%d, %d words, tables %d B, %d samples (%d accepted), counts %s: streamed %.3e /s (%.3e .. %.3e); resident %.3e /s "
              "(%.3e .. %.3e); streamed/resident = %.2f; median of %d"
              % (name, gadget.num_locations, gadget.ldw, gadget.type_eff.nbytes, SAMPLES, counts['accepted'], "equal" if same else "DIFFER",
                 med["streamed"], min(got["streamed"]), max(got["streamed"]), med["resident"], min(got["resident"]), max(got["resident"]),
                 med["streamed"] / med["resident"], REPEATS), flush=True)
        if not same:
            sys.exit(1)
    for rounds, samples in LONG:
        gadget = stream_noise.stream_for(steane, "cycle", (rounds, False))
        run = lambda: gadget.error_rates(samples, *P_LONG, seed=1)
        counts = run()
        rates = [timed(ctx, run, samples) for _ in range(REPEATS)]
        med = statistics.median(rates)
        print("steane cycle, %d rounds streamed: L=%d (%d segments), %d samples (%d accepted, %d logical_any): %.3e /s (%.3e .. %.3e); "
              "%.2f ps per sample and round; median of %d"
              % (rounds, gadget.num_locations, (gadget.num_locations + 511) // 512, samples, counts['accepted'], counts['logical_any'], med,
                 min(rates), max(rates), 1e12 / (med * rounds), REPEATS), flush=True)


if __name__ == "__main__":
    main()
