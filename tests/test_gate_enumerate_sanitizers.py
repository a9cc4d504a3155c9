"""
gf2_ec_gate_enumerate_host and gf2_ft_gate_enumerate_host (csrc/gf2_host.cpp) under ThreadSanitizer and AddressSanitizer + UBSan on the
CPU box.  The test compiles csrc/gf2_host.cpp together with the stand-alone driver tests/gate_enumerate_host_check.cpp with
-fsanitize=..., the sanitizer's runtime linked into the program, and runs that program as it is: no interpreter loads the code, and
nothing is preloaded.  The cases are written here, inputs beside the counts tests/gate_enumerate_ref.py expects: windows of every
(w, b) up to weight 3 and one of weight 4 of the Steane cycle and of the gate-free Steane program (the restated gadgets' effect words
and site table, so the driver's input never went through native code), ranges at both ends and across a wrap of the one-operand
part, and the refused arguments; the driver holds every array in a heap block of exactly its size and runs the cases on one
thread, then on two at once.
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
from tests.test_ec_sanitizers import SANITIZERS, message, stream
from tests.test_ft_sanitizers import STEANE, table
from tests.test_host_sanitizers import CSRC, ROOT, without_aslr

DRIVER = os.path.join(ROOT, "tests", "gate_enumerate_host_check.cpp")


def enumerate_cases():
    code = cpu_ref.CSSCode(STEANE, STEANE)
    (table1, entries1), (table2, entries2) = table(code._c1_syndromes, code.x_operator_matrix()[0]), table(code._c2_syndromes, code.z_operator_matrix()[0])
    tail = lambda: table1 + table2
    out, cases = [], 0
    cyc = ec_ref.Cycle(code, 2)
    prog = ft_ref.Rewritten(code, "")
    for tag, gadget, head in ((1, cyc, [cyc.rounds]), (2, prog, [prog.nsteps, prog.measure_mask])):
        eff = ger.effect_words(gadget)
        L = gadget.locations
        site_loc, n1, n2, _ = gate_ref.sites(gadget.gates)
        sites = np.array(site_loc, dtype=np.int64)
        total = lambda w, b: math.comb(n1, w - b) * math.comb(n2, b)
        windows = [(0, 0, 0, 1), (1, 0, 0, n1), (1, 1, n2 - 5, 5), (2, 0, 0, 40), (2, 1, 3 * n1 - 3, 7), (2, 2, total(2, 2) - 9, 9),
                   (3, 0, total(3, 0) - 5, 5), (3, 1, 2 * math.comb(n1, 2) - 3, 7), (3, 2, 5 * n1 - 3, 7), (3, 3, total(3, 3) // 2, 2),
                   (4, 2, 7 * math.comb(n1, 2) - 1, 2), (2, 1, 5, 0)]
        for w, b, first, count in windows:
            want = gate_ref.enumerate_range(gadget, eff, w, b, first, count)
            out += [tag, L, gadget.ldr] + head + [code.r_1, entries1, code.r_2, entries2, n1, n2, w, b, first, count, eff, sites] + tail() + [message("")]
            out += [np.array(want.tolist(), dtype=np.uint64)]
            cases += 1
        twice = sites.copy()
        twice[0] = twice[1]
        for w, b, first, count, r1, table_, text in ((5, 0, 0, 1, 3, sites, "weight"), (2, 3, 0, 1, 3, sites, "CNOT picks"),
                                                     (2, 1, total(2, 1), 1, 3, sites, "leave"), (2, 1, -1, 1, 3, sites, "leave"),
                                                     (1, 0, 0, 1, 32, sites, "<= 31"), (1, 0, 0, 1, 3, twice, "partition")):
            out += [tag, L, gadget.ldr] + head + [r1, entries1, code.r_2, entries2, n1, n2, w, b, first, count, eff, table_] + tail() + [message(text)]
            cases += 1
        out += [tag, L, gadget.ldr] + head + [3, entries1, code.r_2, entries2, n1 + 2, n2 - 1, 1, 0, 0, 1, eff,
                                              np.concatenate((sites, sites[:1]))] + tail() + [message("partition")]
        cases += 1
    return out, cases


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    path = tmp_path_factory.mktemp("gate_enumerate_host") / "cases.bin"
    parts, count = enumerate_cases()
    stream(parts + [0]).tofile(str(path))
    return str(path), count


@pytest.mark.parametrize("kind", ["tsan", "asan"])
def test_gate_enumerate_host_entry_points_under_sanitizer(kind, cases, tmp_path):
    flags, runtimes, marker = SANITIZERS[kind]
    for name in runtimes:                                     # the runtime goes into the program itself
        static = subprocess.run(["g++", "-print-file-name=lib%s.a" % name], capture_output=True, text=True).stdout.strip()
        if not (os.path.isabs(static) and os.path.exists(static)):
            pytest.skip("lib%s.a is not installed" % name)
        flags = flags + ["-static-lib%s" % name]
    program = str(tmp_path / ("gate_enumerate_host_check_%s" % kind))
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include")] + flags +
                   [DRIVER, os.path.join(CSRC, "gf2_host.cpp"), "-o", program], check=True, capture_output=True, text=True)
    path, count = cases
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", TSAN_OPTIONS="exitcode=66 report_signal_unsafe=0",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    run = subprocess.run([program, path], env=env, capture_output=True, text=True, timeout=600, preexec_fn=without_aslr)
    report = run.stdout[-2000:] + run.stderr[-4000:]
    assert run.returncode == 0, report
    assert "gate enumerate host ok: %d cases" % count in run.stdout, report
    assert marker not in run.stderr and "runtime error" not in run.stderr, report
