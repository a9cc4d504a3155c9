"""
gf2_stratum_outcomes_host with gf2_ec_tally_host / gf2_ft_tally_host behind it (csrc/gf2_host.cpp) under ThreadSanitizer and
AddressSanitizer + UBSan on the CPU box.  The test compiles csrc/gf2_host.cpp together with the stand-alone driver
tests/gadget_strata_host_check.cpp with -fsanitize=..., the sanitizer's runtime linked into the program, and runs that program as it
is: no interpreter loads the code, and nothing is preloaded.  The cases are written here, inputs beside the words and counts
tests/gadget_strata_ref.py expects: strata of the Steane cycle and of the gate-free Steane program over the restated gadgets' effect
words (so the driver's input never went through native code), every weight of tests/test_gadget_strata.py, a row pitch wider than
the words, weight 16 on a table of 17 locations, no samples at all, and the refused arguments; the driver holds every array in a
heap block of exactly its size and runs the cases on one thread, then on two at once.
"""
import os
import subprocess

import numpy as np
import pytest

from oracle import cpu_ref
from tests import ec_ref, ft_ref
from tests import gadget_enumerate_ref as ger
from tests import gadget_strata_ref as gsr
from tests.test_ec_sanitizers import SANITIZERS, message, stream
from tests.test_ft_sanitizers import STEANE, table
from tests.test_host_sanitizers import CSRC, ROOT, without_aslr

DRIVER = os.path.join(ROOT, "tests", "gadget_strata_host_check.cpp")


class _Short(object):
    """The first `locations` locations of a restated gadget: its layout and tally, fewer effect rows."""

    def __init__(self, gadget, locations):
        self.gadget, self.locations, self.ldr = gadget, locations, gadget.ldr

    def tally(self, words):
        return self.gadget.tally(words)


def strata_cases():
    code = cpu_ref.CSSCode(STEANE, STEANE)
    (table1, entries1), (table2, entries2) = table(code._c1_syndromes, code.x_operator_matrix()[0]), table(code._c2_syndromes, code.z_operator_matrix()[0])
    tail = lambda: table1 + table2
    out, cases = [], 0
    cyc = ec_ref.Cycle(code, 2)
    prog = ft_ref.Rewritten(code, "")
    for tag, gadget, head in ((1, cyc, [cyc.rounds]), (2, prog, [prog.nsteps, prog.measure_mask])):
        eff = ger.effect_words(gadget)
        L, ldr = gadget.locations, gadget.ldr
        tables = [code.r_1, entries1, code.r_2, entries2]

        def accepted_case(eff, locations, w, seed, first, count, kinds, ldw, judge=gadget):
            words = gsr.stratum_words(eff, seed, first, count, w, kinds)
            want, _ = judge.tally(words)
            return ([tag, locations, ldr] + head + tables + [w, seed, first, count] + list(kinds) + [ldw, eff] + tail() + [message("")] +
                    [words, np.array([int(v) for v in want], dtype=np.uint64)])

        for w, seed, first, count, kinds, ldw in ((0, 1, 0, 64, (1, 1, 1), ldr), (1, 2, 5, 257, (1, 0, 0), ldr), (2, 3, 1000, 300, (2, 1, 3), ldr + 2),
                                                  (3, 4, 1 << 40, 300, (1, 1, 1), ldr), (7, 5, 0, 200, (0, 0, 1), ldr + 1), (16, 6, 77, 200, (2, 1, 3), ldr),
                                                  (3, 7, 9, 0, (1, 1, 1), ldr)):
            out += accepted_case(eff, L, w, seed, first, count, kinds, ldw)
            cases += 1
        short = eff[:17]                                                      # weight 16 of seventeen locations: Floyd's rule takes j almost always
        out += accepted_case(short, 17, 16, 8, 0, 500, (1, 1, 1), ldr, _Short(gadget, 17))
        out += accepted_case(short, 17, 15, 8, 3, 500, (1, 2, 0), ldr, _Short(gadget, 17))
        cases += 2
        refusal = lambda locations, ldr_, w, first, count, kinds, ldw, eff_, text: \
            [tag, locations, ldr_] + head + tables + [w, 1, first, count] + list(kinds) + [ldw, eff_] + tail() + [message(text)]
        for args in ((17, ldr, 17, 0, 4, (1, 1, 1), ldr, short, "min(L = 17, 16)"), (L, ldr, 17, 0, 4, (1, 1, 1), ldr, eff, "16)"),
                     (L, ldr, -1, 0, 4, (1, 1, 1), ldr, eff, "weight"), (5, ldr, 6, 0, 4, (1, 1, 1), ldr, eff[:5], "min(L = 5, 16)"),
                     (L, ldr, 2, -1, 4, (1, 1, 1), ldr, eff, "negative range"), (L, ldr, 2, 0, -1, (1, 1, 1), ldr, eff, "negative range"),
                     (L, ldr, 2, 0, 4, (1, 1, 1), ldr - 1, eff, "ldw"), (L, ldr, 2, 0, 4, (0, 0, 0), ldr, eff, "kind weights"),
                     (L, ldr, 2, 0, 4, (1, -1, 1), ldr, eff, "kind weights"),
                     (4, 17, 2, 0, 4, (1, 1, 1), 17, np.zeros((4, 2, 17), dtype="<u8"), "ldr <= 16")):
            out += refusal(*args)
            cases += 1
    return out, cases


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    path = tmp_path_factory.mktemp("gadget_strata_host") / "cases.bin"
    parts, count = strata_cases()
    stream(parts + [0]).tofile(str(path))
    return str(path), count


@pytest.mark.parametrize("kind", ["tsan", "asan"])
def test_gadget_strata_host_statement_under_sanitizer(kind, cases, tmp_path):
    flags, runtimes, marker = SANITIZERS[kind]
    for name in runtimes:                                     # the runtime goes into the program itself
        static = subprocess.run(["g++", "-print-file-name=lib%s.a" % name], capture_output=True, text=True).stdout.strip()
        if not (os.path.isabs(static) and os.path.exists(static)):
            pytest.skip("lib%s.a is not installed" % name)
        flags = flags + ["-static-lib%s" % name]
    program = str(tmp_path / ("gadget_strata_host_check_%s" % kind))
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include")] + flags +
                   [DRIVER, os.path.join(CSRC, "gf2_host.cpp"), "-o", program], check=True, capture_output=True, text=True)
    path, count = cases
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", TSAN_OPTIONS="exitcode=66 report_signal_unsafe=0",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    run = subprocess.run([program, path], env=env, capture_output=True, text=True, timeout=600, preexec_fn=without_aslr)
    report = run.stdout[-2000:] + run.stderr[-4000:]
    assert run.returncode == 0, report
    assert "gadget strata host ok: %d cases" % count in run.stdout, report
    assert marker not in run.stderr and "runtime error" not in run.stderr, report
