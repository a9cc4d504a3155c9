"""
gf2_retry_gate_words_host (csrc/gf2_host.cpp) under ThreadSanitizer and AddressSanitizer + UBSan on the CPU box.  The test compiles
csrc/gf2_host.cpp together with the stand-alone driver tests/retry_gate_host_check.cpp with -fsanitize=..., the sanitizer's runtime
linked into the program, and runs that program as it is: no interpreter loads the code, and nothing is preloaded.  The cases are
written here, inputs beside the words and attempts tests/retry_gate_ref.py expects: two Steane rounds with and without exhausted
samples (three attempts at p = 3e-3), a row pitch wider than the words, no attempts array, either class alone; the Steane program XY
(a NONE block, seven block types); one Reed-Muller round; no samples at all; and the refused arguments.  The driver holds every
array in a heap block of exactly its size and runs the cases on one thread, then on two at once.
"""
import os
import subprocess

import numpy as np
import pytest

from tests import retry_gate_ref
from tests.test_ec_sanitizers import SANITIZERS, message, stream
from tests.test_host_sanitizers import CSRC, ROOT, without_aslr
from tests.test_stream import streamed

DRIVER = os.path.join(ROOT, "tests", "retry_gate_host_check.cpp")


def retry_gate_cases():
    out, cases = [], 0

    def case(gadget, seed, first, count, p1, p2, max_attempts, pad=0, with_attempts=1, text="", site_loc=None, site_regions=None):
        type_eff, type_locations, type_flags, block_type, block_kind = gadget._sequence()
        site_loc = gadget.type_site_loc if site_loc is None else np.asarray(site_loc, dtype=np.int32)
        site_regions = gadget.type_site_regions if site_regions is None else np.asarray(site_regions, dtype=np.int64)
        ldw = gadget.ldw + 1 + pad
        parts = [1, len(type_locations), len(block_type), len(type_eff), type_locations, type_flags, block_type, block_kind, type_eff,
                 len(gadget.type_regions), gadget.type_nregions, gadget.type_regions, site_regions, len(site_loc), site_loc, np.uint64(seed), first,
                 count, np.array([p1, p2], dtype=np.float64).view(np.int64), max_attempts, ldw, gadget.preparations, with_attempts, message(text)]
        if not text:
            words, attempts = retry_gate_ref.retry_gate_words(gadget, seed, first, count, p1, p2, max_attempts)
            padded = np.full((count, ldw), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
            padded[:, :gadget.ldw + 1] = words
            parts.append(padded)
            if with_attempts:
                parts.append(attempts)
        return parts

    steane2, p = streamed("steane", "cycle", (2, False)), 3e-3
    out += case(steane2, 5, 1 << 40, 1500, p, p, 256)
    out += case(steane2, 6, 0, 1500, p, p, 3, pad=2)
    out += case(steane2, 7, 9, 500, p, p, 1, with_attempts=0)
    out += case(steane2, 7, 9, 0, p, p, 256)
    out += case(steane2, 10, 0, 500, 0.0, 6e-3, 256)
    out += case(steane2, 11, 0, 500, 6e-3, 0.0, 256)
    out += case(streamed("steane", "program", "XY"), 8, 3, 800, 2e-3, 2e-3, 256)
    out += case(streamed("rm15", "cycle", (1, False)), 9, 0, 500, 2e-3, 2e-3, 256, pad=1)
    cases += 8
    loc = steane2.type_site_loc
    swapped = loc.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    outside = loc.copy()
    outside[0] = 148
    for kwargs, text in ((dict(site_loc=np.resize(loc, 229), site_regions=[[55, 47], [7, 7], [51, 41], [14, 7]]), "has n_1 + 2 n_2 = 55 + 2 * 47"),
                         (dict(site_loc=outside), "do not partition its locations 0 .. 147"), (dict(site_loc=swapped), "are not ascending"),
                         (dict(max_attempts=0), "needs 1 <= max_attempts <= 65536, got 0"), (dict(pad=-1), "nsteps + F + 1 = 5 words"),
                         (dict(first=-1), "negative range"), (dict(p1=1.5), "needs 0 <= p_1, p_2 <= 1"), (dict(p2=float("nan")), "needs 0 <= p_1, p_2 <= 1")):
        args = dict(gadget=steane2, seed=1, first=0, count=4, p1=p, p2=p, max_attempts=256, text=text)
        args.update(kwargs)
        out += case(**args)
        cases += 1
    return out, cases


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    path = tmp_path_factory.mktemp("retry_gate_host") / "cases.bin"
    parts, count = retry_gate_cases()
    stream(parts + [0]).tofile(str(path))
    return str(path), count


@pytest.mark.parametrize("kind", ["tsan", "asan"])
def test_retry_gate_host_statement_under_sanitizer(kind, cases, tmp_path):
    flags, runtimes, marker = SANITIZERS[kind]
    for name in runtimes:                                     # the runtime goes into the program itself
        static = subprocess.run(["g++", "-print-file-name=lib%s.a" % name], capture_output=True, text=True).stdout.strip()
        if not (os.path.isabs(static) and os.path.exists(static)):
            pytest.skip("lib%s.a is not installed" % name)
        flags = flags + ["-static-lib%s" % name]
    program = str(tmp_path / ("retry_gate_host_check_%s" % kind))
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include")] + flags +
                   [DRIVER, os.path.join(CSRC, "gf2_host.cpp"), "-o", program], check=True, capture_output=True, text=True)
    path, count = cases
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", TSAN_OPTIONS="exitcode=66 report_signal_unsafe=0",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    run = subprocess.run([program, path], env=env, capture_output=True, text=True, timeout=600, preexec_fn=without_aslr)
    report = run.stdout[-2000:] + run.stderr[-4000:]
    assert run.returncode == 0, report
    assert "retry gate host ok: %d cases" % count in run.stdout, report
    assert marker not in run.stderr and "runtime error" not in run.stderr, report
