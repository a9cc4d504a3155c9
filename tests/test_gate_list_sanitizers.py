"""
gf2_ec_gate_enumerate_list_host and gf2_ft_gate_enumerate_list_host (csrc/gf2_host.cpp) under ThreadSanitizer and AddressSanitizer +
UBSan on the CPU box.  The test compiles csrc/gf2_host.cpp together with the stand-alone driver tests/gate_list_host_check.cpp with
-fsanitize=..., the sanitizer's runtime linked into the program, and runs that program as it is: no interpreter loads the code, and
nothing is preloaded.  The cases are written here, inputs beside the records tests/gate_list_ref.py expects: windows of every (w, b)
up to weight 3 of the two-round Steane cycle and of the gate-free Steane program (the restated gadgets' effect words and site table,
so the driver's input never went through native code) with several selects, each with capacity 0, one record too few, exactly enough
and three more, a weight-4 window on a short table, and the refused arguments; the driver holds every array, the record buffer
included, in a heap block of exactly its size and runs the cases on one thread, then on two at once.
"""
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import cpu_ref
from tests import ec_ref, ft_ref
from tests import gadget_enumerate_ref as ger
from tests import gate_enumerate_ref as gate_ref
from tests import gate_list_ref as list_ref
from tests.test_ec_sanitizers import SANITIZERS, message, stream
from tests.test_ft_sanitizers import STEANE, table
from tests.test_host_sanitizers import CSRC, ROOT, without_aslr

DRIVER = os.path.join(ROOT, "tests", "gate_list_host_check.cpp")


class _ShortGates(object):
    """The first `ngates` gates of a restated gadget: its layout and tally, fewer sites and effect rows."""

    def __init__(self, gadget, ngates):
        self.gates, self.ldr, self._tally = np.asarray(gadget.gates)[:ngates], gadget.ldr, gadget.tally
        self.locations = int(sum(2 if kind == gate_ref.CNOT else 1 for kind, _, _ in self.gates.tolist()))

    def tally(self, words):
        return self._tally(words)


def list_cases():
    code = cpu_ref.CSSCode(STEANE, STEANE)
    (table1, entries1), (table2, entries2) = table(code._c1_syndromes, code.x_operator_matrix()[0]), table(code._c2_syndromes, code.z_operator_matrix()[0])
    tail = lambda: table1 + table2
    out, cases = [], 0
    cyc = ec_ref.Cycle(code, 2)
    prog = ft_ref.Rewritten(code, "")
    for tag, gadget, head, selects in ((1, cyc, [cyc.rounds], (1, 6, 0x1f, 0x18)), (2, prog, [prog.nsteps, prog.measure_mask], (1, 2, 0x3f, 0x0c))):
        eff = ger.effect_words(gadget)
        L = gadget.locations
        site_loc, n1, n2, _ = gate_ref.sites(gadget.gates)
        sites = np.array(site_loc, dtype=np.int64)
        total = lambda w, b: math.comb(n1, w - b) * math.comb(n2, b)
        windows = [(0, 0, 0, 1), (1, 0, 0, n1), (1, 1, n2 - 5, 5), (2, 0, 0, 200), (2, 1, 3 * n1 - 3, 70), (2, 2, total(2, 2) - 90, 90),
                   (3, 0, total(3, 0) - 5, 5), (3, 1, 2 * math.comb(n1, 2) - 3, 7), (3, 2, 5 * n1 - 3, 7), (3, 3, total(3, 3) // 2, 2), (2, 1, 5, 0)]

        def add(short, eff, sites, n1, n2, w, b, first, count, select):
            nonlocal out, cases
            want = list_ref.list_range(short, eff, w, b, first, count, select)
            for capacity in sorted({0, max(0, len(want) - 1), len(want), len(want) + 3}):
                out += [tag, short.locations, gadget.ldr] + head + [code.r_1, entries1, code.r_2, entries2, n1, n2, w, b, first, count, select,
                                                                    capacity, eff, sites]
                out += tail() + [message(""), len(want)] + ([want] if len(want) <= capacity else [])
                cases += 1

        for k, (w, b, first, count) in enumerate(windows):
            for select in (selects[k % 4], selects[(k + 1) % 4]):
                add(gadget, eff, sites, n1, n2, w, b, first, count, select)
        # weight 4 on a short table: the gadget's first gates up to its fifth CNOT, the last ranks of (4, 2)
        kinds = np.asarray(gadget.gates)[:, 0]
        short = _ShortGates(gadget, int(np.nonzero(np.cumsum(kinds == gate_ref.CNOT) == 5)[0][0]) + 1)
        s_loc, s1, s2, _ = gate_ref.sites(short.gates)
        assert s2 == 5 and s1 >= 4 and s1 + 2 * s2 == short.locations
        s_all = math.comb(s1, 2) * math.comb(s2, 2)
        add(short, eff[:short.locations], np.array(s_loc, dtype=np.int64), s1, s2, 4, 2, s_all - 40, 40, 1)
        refusals = ((1, 0, 0, 1, 3, 0, 4, "select"), (1, 0, 0, 1, 3, selects[2] + 1, 4, "class bits"), (1, 0, 0, 1, 3, 1, -1, "capacity"),
                    (5, 0, 0, 1, 3, 1, 4, "weight"), (2, 3, 0, 1, 3, 1, 4, "CNOT picks"), (2, 1, total(2, 1), 1, 3, 1, 4, "leave"),
                    (2, 1, -1, 1, 3, 1, 0, "leave"), (1, 0, 0, 1, 32, 1, 4, "<= 31"))
        for w, b, first, count, r1, select, capacity, text in refusals:
            out += [tag, L, gadget.ldr] + head + [r1, entries1, code.r_2, entries2, n1, n2, w, b, first, count, select, capacity, eff, sites]
            out += tail() + [message(text)]
            cases += 1
        twice = sites.copy()
        twice[0] = twice[1]
        out += [tag, L, gadget.ldr] + head + [3, entries1, code.r_2, entries2, n1, n2, 1, 0, 0, 1, 1, 4, eff, twice] + tail() + [message("partition")]
        out += [tag, L, gadget.ldr] + head + [3, entries1, code.r_2, entries2, n1 + 2, n2 - 1, 1, 0, 0, 1, 1, 4, eff,
                                              np.concatenate((sites, sites[:1]))] + tail() + [message("partition")]
        cases += 2
    four = np.arange(4, dtype=np.int64)
    for ldr, rounds, text in ((9, 2, "ldr <= 8"), (cyc.ldr, 7, "rounds <= 6"), (3, 2, "F >= 1")):
        out += [1, 4, ldr, rounds, 3, entries1, 3, entries2, 4, 0, 1, 0, 0, 1, 1, 4, np.zeros((4, 2, ldr), dtype="<u8"), four] + tail() + [message(text)]
        cases += 1
    for ldr, nsteps, mask, text in ((17, 6, 0b010101, "ldr <= 16"), (8, 6, 0b010100, "odd number"), (8, 6, 1 << 6, "at or above nsteps"), (8, 8, 0b010101, "F >= 1")):
        out += [2, 4, ldr, nsteps, mask, 3, entries1, 3, entries2, 4, 0, 1, 0, 0, 1, 1, 4, np.zeros((4, 2, ldr), dtype="<u8"), four] + tail() + [message(text)]
        cases += 1
    return out, cases


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    path = tmp_path_factory.mktemp("gate_list_host") / "cases.bin"
    parts, count = list_cases()
    stream(parts + [0]).tofile(str(path))
    return str(path), count


@pytest.mark.parametrize("kind", ["tsan", "asan"])
def test_gate_list_host_entry_points_under_sanitizer(kind, cases, tmp_path):
    flags, runtimes, marker = SANITIZERS[kind]
    for name in runtimes:                                     # the runtime goes into the program itself
        static = subprocess.run(["g++", "-print-file-name=lib%s.a" % name], capture_output=True, text=True).stdout.strip()
        if not (os.path.isabs(static) and os.path.exists(static)):
            pytest.skip("lib%s.a is not installed" % name)
        flags = flags + ["-static-lib%s" % name]
    program = str(tmp_path / ("gate_list_host_check_%s" % kind))
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include")] + flags +
                   [DRIVER, os.path.join(CSRC, "gf2_host.cpp"), "-o", program], check=True, capture_output=True, text=True)
    path, count = cases
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", TSAN_OPTIONS="exitcode=66 report_signal_unsafe=0",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    run = subprocess.run([program, path], env=env, capture_output=True, text=True, timeout=600, preexec_fn=without_aslr)
    report = run.stdout[-2000:] + run.stderr[-4000:]
    assert run.returncode == 0, report
    assert "gate list host ok: %d cases" % count in run.stdout, report
    assert marker not in run.stderr and "runtime error" not in run.stderr, report
