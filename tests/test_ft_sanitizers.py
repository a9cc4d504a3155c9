"""
gf2_ft_tally_host (csrc/gf2_host.cpp) under ThreadSanitizer and AddressSanitizer + UBSan on the CPU box.  The test compiles
csrc/gf2_host.cpp together with the stand-alone driver tests/ft_host_check.cpp with -fsanitize=..., the sanitizer's runtime linked
into the program, and runs that program as it is: no interpreter loads the code, and nothing is preloaded.  The cases are written
here, inputs beside the results tests/ft_ref.py expects: tallies of random outcome words of Steane and Reed-Muller programs (every
LDR from 8 to 16 that they have, exact-fit and padded rows) and the refused arguments; the driver holds every array in a heap block
of exactly its size and runs the cases on one thread, then on two at once.
"""
import os
import subprocess

import numpy as np
import pytest

from oracle import cpu_ref
from tests import ft_ref
from tests.test_ec_sanitizers import SANITIZERS, message, stream
from tests.test_host_sanitizers import CSRC, ROOT, without_aslr

DRIVER = os.path.join(ROOT, "tests", "ft_host_check.cpp")
STEANE = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])


def table(entries, operator):
    keys = np.array([int(k) for k in entries], dtype="<u8")
    return [keys, [int(np.dot(operator, e)) & 1 for e in entries.values()]], len(keys)


def tally_cases(rng):
    cols = np.arange(1, 16)
    h1 = np.array([(cols >> b) & 1 for b in range(4)])
    rm15 = cpu_ref.CSSCode(h1, np.vstack([h1] + [h1[a] & h1[b] for a in range(4) for b in range(a + 1, 4)]))
    steane = cpu_ref.CSSCode(STEANE, STEANE)
    out, cases = [], 0
    #   code, logical gates, flag words, extra words per row
    for code, k, flag_words, pad in ((steane, 0, 2, 0), (steane, 3, 2, 0), (steane, 5, 3, 2), (steane, 7, 3, 0), (rm15, 0, 3, 1)):
        steps = [ft_ref.EC] * k + [ft_ref.MEASURE, ft_ref.EC] * 3
        nsteps, mask = len(steps), sum(1 << s for s, kind in enumerate(steps) if kind == ft_ref.MEASURE)
        ldr, count = nsteps + flag_words, 600
        (table1, entries1), (table2, entries2) = table(code._c1_syndromes, code.x_operator_matrix()[0]), table(code._c2_syndromes, code.z_operator_matrix()[0])
        words = np.zeros((count, ldr + pad), dtype="<u8")
        for s, kind in enumerate(steps):
            key_x = rng.integers(0, 1 << code.r_2, count, dtype=np.uint64)
            high = (rng.integers(0, 1 << code.r_1, count, dtype=np.uint64) << np.uint64(32) if kind == ft_ref.EC
                    else (rng.random(count) < 0.2).astype(np.uint64) << np.uint64(31))
            quiet = rng.random(count) < 0.7
            words[:, s] = np.where(quiet, 0, key_x | high)
        words[rng.random(count) < 0.1, ldr - 1] = 1 << 40
        words[:, ldr:] = 0xffff                                                   # beyond ldr: never read
        want, classes = ft_ref.tally(code, steps, words[:, :ldr])
        assert 100 < want[0] < count and 10 < want[1] < want[0] and want[4] > 10    # accepted, rejected, wrong, right and split words all occur
        out += [1, count, ldr + pad, ldr, nsteps, mask, code.r_1, entries1, code.r_2, entries2, words] + table1 + table2 + [message(""), want, classes]
        cases += 1
    words = np.zeros(17, dtype="<u8")
    for nsteps, mask, r1, r2, ldr, text in ((9, 0b10101000, 32, 3, 11, "<= 31"), (9, 0b10101000, 3, 3, 17, "ldr <= 16"), (9, 0b101000, 3, 3, 11, "odd number"),
                                            (9, 1 << 9, 3, 3, 11, "at or above nsteps"), (11, 0b10101000, 3, 3, 11, "F >= 1"), (0, 0, 3, 3, 5, "nsteps >= 1")):
        out += [1, 1, 17, ldr, nsteps, mask, r1, entries1, r2, entries2, words] + table1 + table2 + [message(text)]
        cases += 1
    return out, cases


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    rng = np.random.default_rng(5)
    path = tmp_path_factory.mktemp("ft_host") / "cases.bin"
    parts, count = tally_cases(rng)
    stream(parts + [0]).tofile(str(path))
    return str(path), count


@pytest.mark.parametrize("kind", ["tsan", "asan"])
def test_ft_host_entry_point_under_sanitizer(kind, cases, tmp_path):
    flags, runtimes, marker = SANITIZERS[kind]
    for name in runtimes:                                     # the runtime goes into the program itself
        static = subprocess.run(["g++", "-print-file-name=lib%s.a" % name], capture_output=True, text=True).stdout.strip()
        if not (os.path.isabs(static) and os.path.exists(static)):
            pytest.skip("lib%s.a is not installed" % name)
        flags = flags + ["-static-lib%s" % name]
    program = str(tmp_path / ("ft_host_check_%s" % kind))
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include")] + flags +
                   [DRIVER, os.path.join(CSRC, "gf2_host.cpp"), "-o", program], check=True, capture_output=True, text=True)
    path, count = cases
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", TSAN_OPTIONS="exitcode=66 report_signal_unsafe=0",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    run = subprocess.run([program, path], env=env, capture_output=True, text=True, timeout=600, preexec_fn=without_aslr)
    report = run.stdout[-2000:] + run.stderr[-4000:]
    assert run.returncode == 0, report
    assert "ft host ok: %d cases" % count in run.stdout, report
    assert marker not in run.stderr and "runtime error" not in run.stderr, report
