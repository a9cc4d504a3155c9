"""
gf2_gate_outcomes_host with gf2_ec_tally_host / gf2_ft_tally_host behind it (csrc/gf2_host.cpp) under ThreadSanitizer and
AddressSanitizer + UBSan on the CPU box.  The test compiles csrc/gf2_host.cpp together with the stand-alone driver
tests/gate_mc_host_check.cpp with -fsanitize=..., the sanitizer's runtime linked into the program, and runs that program as it is:
no interpreter loads the code, and nothing is preloaded.  The cases are written here, inputs beside the words, fault counts and
tally tests/gate_mc_ref.py expects: the Steane cycle and the gate-free Steane program over the restated gadgets' effect words and
site tables (so the driver's input never went through native code) at p in {0, 1e-3, 0.5, 1}, a range past 2^40, a row pitch wider
than the words, no faults_out, no samples at all, the synthetic site tables of tests/test_gate_mc.py with picks on both sides of a
segment boundary, and the refused arguments; the driver holds every array in a heap block of exactly its size and runs the cases on
one thread, then on two at once.
"""
import os
import subprocess

import numpy as np
import pytest

from oracle import cpu_ref
from tests import ec_ref, ft_ref
from tests import gadget_enumerate_ref as ger
from tests import gate_enumerate_ref as gate_ref
from tests import gate_mc_ref as gmr
from tests import gate_strata_ref as gsr
from tests.test_ec_sanitizers import SANITIZERS, message, stream
from tests.test_ft_sanitizers import STEANE, table
from tests.test_host_sanitizers import CSRC, ROOT, without_aslr

DRIVER = os.path.join(ROOT, "tests", "gate_mc_host_check.cpp")
SEED = 20261020
SITE_TABLES = ((512, 1), (513, 0), (0, 513), (1024, 1025), (1, 1))


def bits(p):
    return np.array([p], dtype="<f8").view("<i8")


def mc_cases():
    code = cpu_ref.CSSCode(STEANE, STEANE)
    (table1, entries1), (table2, entries2) = table(code._c1_syndromes, code.x_operator_matrix()[0]), table(code._c2_syndromes, code.z_operator_matrix()[0])
    tail = lambda: table1 + table2
    out, cases = [], 0
    cyc = ec_ref.Cycle(code, 1)
    prog = ft_ref.Rewritten(code, "")
    for tag, gadget, head in ((1, cyc, [cyc.rounds]), (2, prog, [prog.nsteps, prog.measure_mask])):
        eff = ger.effect_words(gadget)
        ldr = gadget.ldr
        site_loc, n1, n2, _ = gate_ref.sites(gadget.gates)
        sites = np.array(site_loc, dtype=np.int64)
        tables = [code.r_1, entries1, code.r_2, entries2]

        def accepted_case(eff, sites, n1, n2, p1, p2, seed, first, count, ldw, with_faults):
            words, faults = gmr.gate_mc_words(eff, sites, n1, n2, seed, first, count, p1, p2)
            want = np.array([int(v) for v in gadget.tally(words)[0]], dtype=np.uint64)
            return ([tag, len(eff), ldr] + head + tables + [n1, n2, bits(p1), bits(p2), seed, first, count, ldw, with_faults, eff, sites] + tail() +
                    [message("")] + [words, faults.astype(np.int64), want])

        for case, (p1, p2, first, count, ldw, with_faults) in enumerate(((0.0, 0.0, 0, 64, ldr, 1), (1e-3, 1e-3, 5, 257, ldr, 1),
                                                                         (1e-3, 2e-3, 1 << 40, 300, ldr + 2, 1), (0.5, 0.5, 1000, 40, ldr, 1),
                                                                         (1.0, 1.0, 0, 12, ldr + 1, 1), (0.05, 0.0, 77, 200, ldr, 0),
                                                                         (0.0, 0.05, 3, 200, ldr, 1), (0.01, 0.01, 9, 0, ldr, 1))):
            out += accepted_case(eff, sites, n1, n2, p1, p2, SEED + case, first, count, ldw, with_faults)
            cases += 1
        # synthetic site tables over the gadget's effect table, repeated until it reaches: picks on both sides of a segment boundary
        rng = np.random.default_rng(SEED + tag)
        for m1, m2 in SITE_TABLES:
            long = np.tile(eff, (-(-(m1 + 2 * m2) // len(eff)), 1, 1))[:m1 + 2 * m2]
            for p in (1e-3, 0.5, 1.0):
                out += accepted_case(long, gsr.synthetic_sites(m1, m2, rng).astype(np.int64), m1, m2, p, p, SEED, 0, 24, ldr, 1)
                cases += 1
        refusal = lambda eff_, ldr_, sites_, n1_, n2_, p1, p2, first, count, ldw, text: \
            [tag, len(eff_), ldr_] + head + tables + [n1_, n2_, bits(p1), bits(p2), 1, first, count, ldw, 1, eff_, sites_] + tail() + [message(text)]
        overlap = sites.copy()
        overlap[1] = overlap[0]
        nan = float("nan")
        for args in ((eff, ldr, sites, n1, n2, -1e-9, 0.1, 0, 4, ldr, "0 <= p_1, p_2 <= 1"), (eff, ldr, sites, n1, n2, 1.0 + 1e-9, 0.1, 0, 4, ldr, "0 <= p_1, p_2 <= 1"),
                     (eff, ldr, sites, n1, n2, nan, 0.1, 0, 4, ldr, "0 <= p_1, p_2 <= 1"), (eff, ldr, sites, n1, n2, 0.1, -0.5, 0, 4, ldr, "0 <= p_1, p_2 <= 1"),
                     (eff, ldr, sites, n1, n2, 0.1, 2.0, 0, 4, ldr, "0 <= p_1, p_2 <= 1"), (eff, ldr, sites, n1, n2, 0.1, nan, 0, 4, ldr, "0 <= p_1, p_2 <= 1"),
                     (eff, ldr, overlap, n1, n2, 0.1, 0.1, 0, 4, ldr, "no partition"), (eff, ldr, sites[1:], n1 - 1, n2, 0.1, 0.1, 0, 4, ldr, "no partition"),
                     (eff, ldr, sites, n1, n2, 0.1, 0.1, -1, 4, ldr, "first_sample >= 0"), (eff, ldr, sites, n1, n2, 0.1, 0.1, 0, -1, ldr, "count >= 0"),
                     (eff, ldr, sites, n1, n2, 0.1, 0.1, 0, 4, ldr - 1, "ldw"),
                     (np.zeros((4, 2, 17), dtype="<u8"), 17, np.arange(4), 4, 0, 0.1, 0.1, 0, 4, 17, "ldr <= 16")):
            out += refusal(*args)
            cases += 1
    return out, cases


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    path = tmp_path_factory.mktemp("gate_mc_host") / "cases.bin"
    parts, count = mc_cases()
    stream(parts + [0]).tofile(str(path))
    return str(path), count


@pytest.mark.parametrize("kind", ["tsan", "asan"])
def test_gate_mc_host_statement_under_sanitizer(kind, cases, tmp_path):
    flags, runtimes, marker = SANITIZERS[kind]
    for name in runtimes:                                     # the runtime goes into the program itself
        static = subprocess.run(["g++", "-print-file-name=lib%s.a" % name], capture_output=True, text=True).stdout.strip()
        if not (os.path.isabs(static) and os.path.exists(static)):
            pytest.skip("lib%s.a is not installed" % name)
        flags = flags + ["-static-lib%s" % name]
    program = str(tmp_path / ("gate_mc_host_check_%s" % kind))
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include")] + flags +
                   [DRIVER, os.path.join(CSRC, "gf2_host.cpp"), "-o", program], check=True, capture_output=True, text=True)
    path, count = cases
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", TSAN_OPTIONS="exitcode=66 report_signal_unsafe=0",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    run = subprocess.run([program, path], env=env, capture_output=True, text=True, timeout=600, preexec_fn=without_aslr)
    report = run.stdout[-2000:] + run.stderr[-4000:]
    assert run.returncode == 0, report
    assert "gate mc host ok: %d cases" % count in run.stdout, report
    assert marker not in run.stderr and "runtime error" not in run.stderr, report
