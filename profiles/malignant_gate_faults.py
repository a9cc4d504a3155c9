#!/usr/bin/env python3
"""The results of DESIGN.md section 5e "Malignant fault sets under gate-level faults", regenerated: the weight-2 lists of every CNOT
count b (malignant_gate_faults) of the one- and two-round Steane cycles (select: a logical flip) and of the gate-free Steane program,
`X X X MEASURE` and the gate-free Reed-Muller [[15,1,3]] program (select: wrong), each reduced to what a reader can act on -- the
number listed per (b, c), the gates that take part, the pairs grouped by the step of the gadget each pick falls in, by the part of the
step (ECGates.gate_paths) and by gate and Pauli, each group with the share of its pairs that carry a two-operand CNOT kind, and for
the two-round cycle the share of pairs with one pick in each round.

The series check: with the depolarising odds to first order, x = 1/3 and y_1 = y_2 = 1/15 per unit of p, the lists' coefficients
L_w (flips) and A_w (accepted) of weights 1 and 2 give the p^2 coefficient of the conditional rate, c_2 = L_2 + L_1 - L_1 A_1 (the
middle term: the p^2 part of the weight-1 odds p / (1 - p); the last: the quotient by P(accepted)), which must equal
GateStrata.series(('depolarising', 1))[2] of enumerate_gate_strata([0, 1, 2]) -- 16516/45 for the one-round cycle, 47228/225 for the
Reed-Muller program.  `--host` runs the host statements (no GPU, exact; a minute)."""
import collections
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quantum_css_codes_amd import ec_noise, ft_noise  # noqa: E402

STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
GATE_NAMES = {ec_noise.GATE_H: "H", ec_noise.GATE_CNOT: "CNOT", ec_noise.GATE_IDLE: "IDLE", ec_noise.GATE_RESET: "RESET"}
ODDS = (Fraction(1, 3), Fraction(1, 15), Fraction(1, 15))                   # depolarising, p_2 = p_1 = p, to first order in p
BUDGET = 1 << 40
TOP = 12


def rm15_checks():
    cols = np.arange(1, 16)
    h1 = np.array([(cols >> b) & 1 for b in range(4)])
    return h1, np.vstack([h1] + [h1[a] & h1[b] for a in range(4) for b in range(a + 1, 4)])


def two_operand(paulis):
    return len(paulis) == 2 and 'I' not in paulis


def table(title, groups, total):
    """groups: key -> [pairs, pairs with a two-operand kind]."""
    order = sorted(groups.items(), key=lambda item: -item[1][0])
    print("  %s (%d groups; the %d largest; in brackets the share of the group with a two-operand kind):" % (title, len(order), min(TOP, len(order))))
    for key, (n, two) in order[:TOP]:
        print("    %6d  %5.1f %%  [%5.1f %%]  %s" % (n, 100.0 * n / total, 100.0 * two / n, key))


def grouped(records, key):
    groups = collections.defaultdict(lambda: [0, 0])
    for row in records:
        entry = groups[key(row)]
        entry[0] += 1
        entry[1] += any(two_operand(paulis) for _, _, _, paulis in row)
    return groups


def reduce(name, gadget, field, host):
    mask = gadget.flip_mask
    strata = gadget.enumerate_gate_strata([0, 1, 2], max_configurations=BUDGET, host=host)
    one = gadget.malignant_gate_faults(1, select=1, max_configurations=BUDGET, host=host)
    two = gadget.malignant_gate_faults(2, max_configurations=BUDGET, host=host)
    _, n1, n2, site_gate = gadget.gate_sites()
    found = len(two)
    l_1, a_1, l_2 = one.coefficient(ODDS, mask), one.coefficient(ODDS), two.coefficient(ODDS, mask)
    series = strata.series(('depolarising', 1), field)
    c_2 = l_2 + l_1 - l_1 * a_1
    print("%s: %d one-operand gates, %d CNOTs; weight 2, select %s: %d listed of %d configurations; [b][c] %s"
          % (name, n1, n2, field, found, strata.configurations()[2], two.counts().tolist()), flush=True)
    print("  weight 1: [b][c] %s listed; L_1 = %s, A_1 = %s; weight 2: L_2 = %s (b = 0, 1, 2: %s); c_2 = L_2 + L_1 - L_1 A_1 = %s; series %s: %s"
          % (one.counts(mask).tolist(), l_1, a_1, l_2, ", ".join(str(part.coefficient(ODDS, mask)) for part in two), c_2,
             [str(c) for c in series], "agree" if (series[1], series[2]) == (l_1, c_2) else "DIFFER"))
    assert (series[1], series[2]) == (l_1, c_2), (series, l_1, c_2)
    assert two.counts(mask).tolist() == strata.counts[2][:, :, strata.fields.index(field)].astype(np.int64).tolist()
    if not found:
        return [], []
    heat = two.gate_counts(site_gate)
    paths = gadget.gadget.gate_paths()
    records = gadget.describe_gate_faults(two)
    share = sum(1 for row in records if any(two_operand(p) for _, _, _, p in row))
    print("  %d of the %d gates take part in a listed pair; %d pairs (%.1f %%) carry a two-operand kind; their share of L_2: %.1f %%"
          % (int((heat > 0).sum()), len(heat), share, 100.0 * share / found,
             100.0 * float(sum(int(n) * ODDS[0]**(2 - b) * ODDS[1]**b for b, part in enumerate(two) for n in part.counts(mask)[1:]) / l_2)))
    gate_name = lambda gate: GATE_NAMES[gate[0]]
    table("by step of each pick", grouped(records, lambda row: " + ".join(sorted(paths[g][0] if paths[g] else "-" for g, _, _, _ in row))), found)
    table("by part of the step", grouped(records, lambda row: " + ".join(sorted(" / ".join(paths[g]) for g, _, _, _ in row))), found)
    table("by part, steps merged", grouped(records, lambda row: " + ".join(sorted(" / ".join(paths[g][1:]) for g, _, _, _ in row))), found)
    table("by gate and Pauli", grouped(records, lambda row: " + ".join(sorted("%s %s" % (gate_name(gate), p) for _, gate, _, p in row))), found)
    print("  the %d gates in most listed pairs:" % TOP)
    for g in np.argsort(-heat, kind="stable")[:TOP].tolist():
        kind, a, b = (int(v) for v in gadget.gadget.gates[g])
        print("    %6d  gate %4d: %s %s, %s" % (int(heat[g]), g, GATE_NAMES[kind], (a, b) if kind == ec_noise.GATE_CNOT else (a,), " / ".join(paths[g])))
    return records, paths


def main():
    host = "--host" in sys.argv
    if host:
        from oracle import cpu_ref
        make = cpu_ref.CSSCode
    else:
        from quantum_css_codes_amd.css_code import CSSCode as make
    steane, rm15 = make(STEANE, STEANE), make(*rm15_checks())
    for rounds in (1, 2):
        circ = ec_noise.circuit_for(steane, rounds)
        records, paths = reduce("steane cycle rounds=%d" % rounds, circ, 'logical_any', host)
        if rounds == 2:
            across = sum(1 for row in records if len({paths[g][0] for g, _, _, _ in row}) > 1)
            print("  pairs with one pick in each round: %d of %d (%.1f %%)" % (across, len(records), 100.0 * across / len(records)), flush=True)
    for name, code, ops in (("steane program ''", steane, ""), ("steane program 'XXX'", steane, "XXX"), ("rm15 program ''", rm15, "")):
        reduce(name, ft_noise.program_for(code, ops), 'wrong', host)


if __name__ == "__main__":
    main()
