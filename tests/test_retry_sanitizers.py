"""
gf2_retry_words_host (csrc/gf2_host.cpp) under ThreadSanitizer and AddressSanitizer + UBSan on the CPU box.  The test compiles
csrc/gf2_host.cpp together with the stand-alone driver tests/retry_host_check.cpp with -fsanitize=..., the sanitizer's runtime linked
into the program, and runs that program as it is: no interpreter loads the code, and nothing is preloaded.  The cases are written
here, inputs beside the words and attempts tests/retry_ref.py expects: two Steane rounds with and without exhausted samples (three
attempts at p = 3e-3), a row pitch wider than the words, no attempts array; the Steane program XY (a NONE block, seven block types);
one Reed-Muller round (segments of 369 and 330 locations); no samples at all; and the refused arguments.  The driver holds every
array in a heap block of exactly its size and runs the cases on one thread, then on two at once.
"""
import os
import subprocess

import numpy as np
import pytest

from tests import retry_ref
from tests.test_ec_sanitizers import SANITIZERS, message, stream
from tests.test_host_sanitizers import CSRC, ROOT, without_aslr
from tests.test_stream import streamed

DRIVER = os.path.join(ROOT, "tests", "retry_host_check.cpp")


def retry_cases():
    out, cases = [], 0

    def case(gadget, seed, first, count, p, max_attempts, pad=0, with_attempts=1, text="", regions=None):
        type_eff, type_locations, type_flags, block_type, block_kind = gadget._sequence()
        regions = gadget.type_regions if regions is None else np.asarray(regions, dtype=np.int64)
        ldw = gadget.ldw + 1 + pad
        parts = [1, len(type_locations), len(block_type), len(type_eff), type_locations, type_flags, block_type, block_kind, type_eff,
                 len(regions), gadget.type_nregions, regions, np.uint64(seed), first, count, np.array(p, dtype=np.float64).view(np.int64),
                 max_attempts, ldw, gadget.preparations, with_attempts, message(text)]
        if not text:
            words, attempts = retry_ref.retry_words(gadget, seed, first, count, p, max_attempts)
            padded = np.full((count, ldw), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
            padded[:, :gadget.ldw + 1] = words
            parts.append(padded)
            if with_attempts:
                parts.append(attempts)
        return parts

    steane2, p = streamed("steane", "cycle", (2, False)), (3e-3, 3e-3, 3e-3)
    out += case(steane2, 5, 1 << 40, 1500, p, 256)
    out += case(steane2, 6, 0, 1500, p, 3, pad=2)
    out += case(steane2, 7, 9, 500, p, 1, with_attempts=0)
    out += case(steane2, 7, 9, 0, p, 256)
    out += case(streamed("steane", "program", "XY"), 8, 3, 800, (2e-3, 2e-3, 2e-3), 256)
    out += case(streamed("rm15", "cycle", (1, False)), 9, 0, 500, (1e-3, 1e-3, 1e-3), 256, pad=1)
    cases += 6
    for kwargs, text in ((dict(regions=[(0, 148, 1), (148, 21, 0), (169, 133, 0), (302, 28, 0)]), "is not retried but its locations set a flag bit"),
                         (dict(regions=[(0, 148, 1), (148, 20, 0), (169, 133, 1), (302, 28, 0)]), "do not partition its 330 locations in order"),
                         (dict(regions=[(0, 100, 1), (100, 69, 1), (169, 133, 1), (302, 28, 0)]), "the flag masks of regions 0 and 1"),
                         (dict(max_attempts=0), "needs 1 <= max_attempts <= 65536, got 0"), (dict(pad=-1), "nsteps + F + 1 = 5 words"),
                         (dict(first=-1), "negative range"), (dict(p=(0.6, 0.6, 0.0)), "sum to at most 1")):
        args = dict(gadget=steane2, seed=1, first=0, count=4, p=p, max_attempts=256, text=text)
        args.update(kwargs)
        out += case(**args)
        cases += 1
    return out, cases


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    path = tmp_path_factory.mktemp("retry_host") / "cases.bin"
    parts, count = retry_cases()
    stream(parts + [0]).tofile(str(path))
    return str(path), count


@pytest.mark.parametrize("kind", ["tsan", "asan"])
def test_retry_host_statement_under_sanitizer(kind, cases, tmp_path):
    flags, runtimes, marker = SANITIZERS[kind]
    for name in runtimes:                                     # the runtime goes into the program itself
        static = subprocess.run(["g++", "-print-file-name=lib%s.a" % name], capture_output=True, text=True).stdout.strip()
        if not (os.path.isabs(static) and os.path.exists(static)):
            pytest.skip("lib%s.a is not installed" % name)
        flags = flags + ["-static-lib%s" % name]
    program = str(tmp_path / ("retry_host_check_%s" % kind))
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include")] + flags +
                   [DRIVER, os.path.join(CSRC, "gf2_host.cpp"), "-o", program], check=True, capture_output=True, text=True)
    path, count = cases
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", TSAN_OPTIONS="exitcode=66 report_signal_unsafe=0",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    run = subprocess.run([program, path], env=env, capture_output=True, text=True, timeout=600, preexec_fn=without_aslr)
    report = run.stdout[-2000:] + run.stderr[-4000:]
    assert run.returncode == 0, report
    assert "retry host ok: %d cases" % count in run.stdout, report
    assert marker not in run.stderr and "runtime error" not in run.stderr, report
