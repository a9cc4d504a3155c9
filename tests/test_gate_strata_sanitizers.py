"""
gf2_gate_stratum_outcomes_host with gf2_ec_tally_host / gf2_ft_tally_host behind it (csrc/gf2_host.cpp) under ThreadSanitizer and
AddressSanitizer + UBSan on the CPU box.  The test compiles csrc/gf2_host.cpp together with the stand-alone driver
tests/gate_strata_host_check.cpp with -fsanitize=..., the sanitizer's runtime linked into the program, and runs that program as it
is: no interpreter loads the code, and nothing is preloaded.  The cases are written here, inputs beside the words, classes and counts
tests/gate_strata_ref.py expects: strata of the Steane cycle and of the gate-free Steane program over the restated gadgets' effect
words and site tables (so the driver's input never went through native code), the strata of tests/test_gate_strata.py, a row pitch
wider than the words, Floyd's fallback at its limit on (n1, n2) = (9, 8) and (16, 1), no samples at all, and the refused arguments;
the driver holds every array in a heap block of exactly its size and runs the cases on one thread, then on two at once.
"""
import os
import subprocess

import numpy as np
import pytest

from oracle import cpu_ref
from tests import ec_ref, ft_ref
from tests import gadget_enumerate_ref as ger
from tests import gate_enumerate_ref as gate_ref
from tests import gate_strata_ref as gsr
from tests.test_ec_sanitizers import SANITIZERS, message, stream
from tests.test_ft_sanitizers import STEANE, table
from tests.test_host_sanitizers import CSRC, ROOT, without_aslr

DRIVER = os.path.join(ROOT, "tests", "gate_strata_host_check.cpp")
SEED = 20261019


class _Short(object):
    """A restated gadget's layout and tally over another effect table."""

    def __init__(self, gadget):
        self.gadget, self.ldr = gadget, gadget.ldr

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
        site_loc, n1, n2, _ = gate_ref.sites(gadget.gates)
        sites = np.array(site_loc, dtype=np.int64)
        tables = [code.r_1, entries1, code.r_2, entries2]

        def accepted_case(eff, sites, n1, n2, a, b, seed, first, count, ldw, judge=gadget):
            words, c = gsr.gate_stratum_words(eff, sites, n1, n2, seed, first, count, a, b)
            want = gsr.gate_stratum_counts(judge, eff, sites, n1, n2, seed, first, count, a, b)
            return ([tag, len(eff), ldr] + head + tables + [n1, n2, a, b, seed, first, count, ldw, eff, sites] + tail() + [message("")] +
                    [words, c.astype(np.int64), want])

        for case, (a, b, first, count, ldw) in enumerate(((0, 0, 0, 64, ldr), (1, 0, 5, 257, ldr), (0, 1, 1000, 300, ldr + 2), (2, 1, 1 << 40, 300, ldr),
                                                          (3, 5, 0, 200, ldr + 1), (8, 8, 77, 200, ldr), (16, 0, 3, 200, ldr), (0, 16, 4, 200, ldr),
                                                          (2, 2, 9, 0, ldr))):
            out += accepted_case(eff, sites, n1, n2, a, b, SEED + case, first, count, ldw)
            cases += 1
        # Floyd's rule takes j almost always: every site of (9, 8) but one CNOT, and all sixteen one-operand sites of (16, 1)
        rng = np.random.default_rng(SEED + tag)
        for (m1, m2), (a, b) in (((9, 8), (9, 7)), ((16, 1), (16, 0))):
            short_sites = gsr.synthetic_sites(m1, m2, rng).astype(np.int64)
            short = eff[:m1 + 2 * m2]
            out += accepted_case(short, short_sites, m1, m2, a, b, SEED, 0, 500, ldr, _Short(gadget))
            cases += 1
        refusal = lambda eff_, ldr_, sites_, n1_, n2_, a, b, first, count, ldw, text: \
            [tag, len(eff_), ldr_] + head + tables + [n1_, n2_, a, b, 1, first, count, ldw, eff_, sites_] + tail() + [message(text)]
        overlap = sites.copy()
        overlap[1] = overlap[0]
        mixed = np.array([0, 1, 2, 3, 5, 7, 9, 11, 13, 15], dtype=np.int64)      # n1 = 3, n2 = 7 over 17 locations
        for args in ((eff, ldr, sites, n1, n2, 9, 8, 0, 4, ldr, "a + b <= 16"), (eff, ldr, sites, n1, n2, 17, 0, 0, 4, ldr, "a + b <= 16"),
                     (eff, ldr, sites, n1, n2, -1, 2, 0, 4, ldr, "a, b >= 0"), (eff[:17], ldr, mixed, 3, 7, 4, 0, 0, 4, ldr, "a <= n_1 = 3"),
                     (eff[:17], ldr, np.arange(17), 17, 0, 3, 1, 0, 4, ldr, "b <= n_2 = 0"), (eff, ldr, overlap, n1, n2, 1, 1, 0, 4, ldr, "no partition"),
                     (eff, ldr, sites[1:], n1 - 1, n2, 1, 1, 0, 4, ldr, "no partition"), (eff, ldr, sites, n1, n2, 1, 1, -1, 4, ldr, "first_sample >= 0"),
                     (eff, ldr, sites, n1, n2, 1, 1, 0, -1, ldr, "count >= 0"), (eff, ldr, sites, n1, n2, 1, 1, 0, 4, ldr - 1, "ldw"),
                     (np.zeros((4, 2, 17), dtype="<u8"), 17, np.arange(4), 4, 0, 1, 0, 0, 4, 17, "ldr <= 16")):
            out += refusal(*args)
            cases += 1
    return out, cases


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    path = tmp_path_factory.mktemp("gate_strata_host") / "cases.bin"
    parts, count = strata_cases()
    stream(parts + [0]).tofile(str(path))
    return str(path), count


@pytest.mark.parametrize("kind", ["tsan", "asan"])
def test_gate_strata_host_statement_under_sanitizer(kind, cases, tmp_path):
    flags, runtimes, marker = SANITIZERS[kind]
    for name in runtimes:                                     # the runtime goes into the program itself
        static = subprocess.run(["g++", "-print-file-name=lib%s.a" % name], capture_output=True, text=True).stdout.strip()
        if not (os.path.isabs(static) and os.path.exists(static)):
            pytest.skip("lib%s.a is not installed" % name)
        flags = flags + ["-static-lib%s" % name]
    program = str(tmp_path / ("gate_strata_host_check_%s" % kind))
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include")] + flags +
                   [DRIVER, os.path.join(CSRC, "gf2_host.cpp"), "-o", program], check=True, capture_output=True, text=True)
    path, count = cases
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", TSAN_OPTIONS="exitcode=66 report_signal_unsafe=0",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    run = subprocess.run([program, path], env=env, capture_output=True, text=True, timeout=600, preexec_fn=without_aslr)
    report = run.stdout[-2000:] + run.stderr[-4000:]
    assert run.returncode == 0, report
    assert "gate strata host ok: %d cases" % count in run.stdout, report
    assert marker not in run.stderr and "runtime error" not in run.stderr, report
