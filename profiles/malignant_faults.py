#!/usr/bin/env python3
"""The results of DESIGN.md "Malignant fault sets of the cycle" and "Malignant fault sets of the measurement", regenerated: the
weight-2 lists (malignant_faults) of the gate-free Reed-Muller [[15,1,3]] and Steane programs (select: wrong) and of the one- and
two-round Steane cycles (select: a logical flip), each reduced to what a reader can act on -- the pairs grouped by the step of the
gadget each pick falls in, by the part of the step (ECGates.gate_paths) and by gate kind and fault kind, the locations that take
part in most pairs (FaultList.location_counts), and for the two-round cycle the share of pairs whose picks lie in different rounds.
`--host` runs the host statements (no GPU, exact; seconds)."""
import collections
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_css_codes_amd import ec_noise, ft_noise  # noqa: E402

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
GATE_NAMES = {ec_noise.GATE_H: "H", ec_noise.GATE_CNOT: "CNOT", ec_noise.GATE_IDLE: "IDLE", ec_noise.GATE_RESET: "RESET"}
TOP = 12


def rm15_checks():
    cols = np.arange(1, 16)
    h1 = np.array([(cols >> b) & 1 for b in range(4)])
    return h1, np.vstack([h1] + [h1[a] & h1[b] for a in range(4) for b in range(a + 1, 4)])


def table(title, counter, total):
    print("  %s (%d groups; the %d largest):" % (title, len(counter), min(TOP, len(counter))))
    for key, n in counter.most_common(TOP):
        print("    %6d  %5.1f %%  %s" % (n, 100.0 * n / total, key))


def role(gadget, gate, qubit):
    kind, a, b = (int(v) for v in gadget.gadget.gates[gate])
    name = GATE_NAMES[kind]
    return name if kind != ec_noise.GATE_CNOT else "CNOT %s" % ("control" if qubit == a else "target")


def reduce(name, gadget, faults):
    found = len(faults)
    print("%s: L = %d, weight %d, %d listed of %d configurations; [n_x][n_y] %s; coefficient at kinds (1, 1, 1): %s"
          % (name, gadget.num_locations, faults.weight, found, 3**faults.weight * sum(n for _, n in faults.ranges), faults.composition_counts().tolist(),
             faults.coefficient((1, 1, 1))), flush=True)
    paths = gadget.gadget.gate_paths()
    picks = [[(int(gadget.locations[l][0]), int(gadget.locations[l][1]), ec_noise.KINDS[k]) for l, k in zip(row_l, row_k)]
             for row_l, row_k in zip(faults.locations().tolist(), faults.kinds().tolist())]
    table("by step of each pick", collections.Counter(" + ".join(paths[g][0] for g, _, _ in row) for row in picks), found)
    table("by part of the step", collections.Counter(" + ".join(" / ".join(paths[g]) for g, _, _ in row) for row in picks), found)
    table("by part, steps merged", collections.Counter(" + ".join(sorted(" / ".join(paths[g][1:]) for g, _, _ in row)) for row in picks), found)
    table("by gate and fault kind", collections.Counter(" + ".join("%s %s" % (kind, role(gadget, g, q)) for g, q, kind in row) for row in picks), found)
    counts = faults.location_counts()
    print("  the %d locations in most listed sets (%d locations take part in none):" % (TOP, int((counts == 0).sum())))
    for l in np.argsort(-counts, kind="stable")[:TOP].tolist():
        g, q = (int(v) for v in gadget.locations[l])
        print("    %6d  location %4d: gate %4d %s qubit %d, %s" % (int(counts[l]), l, g, role(gadget, g, q), q, " / ".join(paths[g])))
    return picks, paths


def main():
    host = "--host" in sys.argv
    if host:
        from oracle import cpu_ref
        make = cpu_ref.CSSCode
    else:
        from quantum_css_codes_amd.css_code import CSSCode as make
    steane, rm15 = make(STEANE, STEANE), make(*rm15_checks())
    for name, code in (("rm15 program ''", rm15), ("steane program ''", steane)):
        prog = ft_noise.program_for(code, "")
        reduce(name, prog, prog.malignant_faults(2, max_configurations=1 << 40, host=host))
    for rounds in (1, 2):
        circ = ec_noise.circuit_for(steane, rounds)
        picks, paths = reduce("steane cycle rounds=%d" % rounds, circ, circ.malignant_faults(2, max_configurations=1 << 40, host=host))
        if rounds == 2:
            across = sum(1 for row in picks if len({paths[g][0] for g, _, _ in row}) > 1)
            print("  pairs with picks in different rounds: %d of %d (%.1f %%)" % (across, len(picks), 100.0 * across / len(picks)), flush=True)


if __name__ == "__main__":
    main()
