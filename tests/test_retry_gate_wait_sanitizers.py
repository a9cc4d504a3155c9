"""
gf2_retry_gate_wait_words_host (csrc/gf2_host.cpp) under ThreadSanitizer and AddressSanitizer + UBSan on the CPU box.  The test
compiles csrc/gf2_host.cpp together with the stand-alone driver tests/retry_gate_wait_host_check.cpp with -fsanitize=..., the
sanitizer's runtime linked into the program, and runs that program as it is: no interpreter loads the code, and nothing is preloaded.
The cases are written here, inputs beside the words and attempts tests/retry_gate_wait_ref.py expects: two Steane rounds with and
without exhausted samples (three attempts at p = 3e-3), two wait steps, a row pitch wider than the words, no attempts array, q = 0;
the Steane program XY (a NONE block without wait rows, seven block types); [prepare, FINAL] with no wait row at all (a null wait
table); one Reed-Muller round; the sequence made by hand with a region of 512 wait rows; no samples at all; and the refused arguments.
The driver holds every array in a heap block of exactly its size and runs the cases on one thread, then on two at once.
"""
import os
import subprocess

import numpy as np
import pytest

from tests import retry_gate_wait_ref
from tests.test_ec_sanitizers import SANITIZERS, message, stream
from tests.test_host_sanitizers import CSRC, ROOT, without_aslr
from tests.test_retry_gate import prepare_final
from tests.test_retry_gate_wait import HandMadeGate, many_wait_sizes
from tests.test_stream import streamed

DRIVER = os.path.join(ROOT, "tests", "retry_gate_wait_host_check.cpp")


def retry_gate_wait_cases():
    out, cases = [], 0

    def case(tables, arguments, ldr, preparations, seed, first, count, p, q, max_attempts, pad=0, with_attempts=1, text="", wait_eff=None,
             wait_count=None):
        type_eff, type_locations, type_flags, block_type, block_kind, regions, nregions, site_loc, site_regions, eff, counts = arguments
        eff = np.asarray(eff if wait_eff is None else wait_eff, dtype=np.uint64).reshape(-1, 2, 2)
        counts = np.asarray(counts if wait_count is None else wait_count, dtype=np.int64)
        site_loc = np.asarray(site_loc, dtype=np.int32)
        ldw = ldr + pad
        parts = [1, len(type_locations), len(block_type), len(type_eff), type_locations, type_flags, block_type, block_kind, type_eff,
                 len(regions), nregions, np.asarray(regions, dtype=np.int64), len(site_loc), np.asarray(site_regions, dtype=np.int64), site_loc,
                 len(eff), counts, eff, np.uint64(seed), first, count, np.array(tuple(p) + tuple(q), dtype=np.float64).view(np.int64), max_attempts,
                 ldw, preparations, with_attempts, message(text)]
        if not text:
            words, attempts = retry_gate_wait_ref.retry_gate_wait_words(*tables, seed, first, count, *p, q, max_attempts)
            padded = np.full((count, ldw), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
            padded[:, :ldr] = words
            parts.append(padded)
            if with_attempts:
                parts.append(attempts)
        return parts

    def of(gadget, wait_steps=1):
        return dict(tables=retry_gate_wait_ref.tables_of(gadget, wait_steps), arguments=gadget._retry_gate_wait_sequence(wait_steps),
                    ldr=gadget.ldw + 2, preparations=gadget.preparations)

    steane2, p, q = streamed("steane", "cycle", (2, False)), (3e-3, 3e-3), (3e-3, 3e-3, 3e-3)
    out += case(**of(steane2), seed=5, first=1 << 40, count=1500, p=p, q=q, max_attempts=256)
    out += case(**of(steane2), seed=6, first=0, count=1500, p=p, q=(1e-2, 0.0, 5e-3), max_attempts=3, pad=2)
    out += case(**of(steane2, 2), seed=7, first=9, count=500, p=p, q=q, max_attempts=1, with_attempts=0)
    out += case(**of(steane2), seed=7, first=9, count=0, p=p, q=q, max_attempts=256)
    out += case(**of(steane2), seed=7, first=9, count=300, p=p, q=(0.0, 0.0, 0.0), max_attempts=256)
    out += case(**of(streamed("steane", "program", "XY")), seed=8, first=3, count=800, p=(2e-3, 2e-3), q=(1e-3, 1e-3, 1e-3), max_attempts=256)
    out += case(**of(prepare_final()), seed=8, first=3, count=300, p=(1e-2, 1e-2), q=q, max_attempts=256)
    out += case(**of(streamed("rm15", "cycle", (1, False))), seed=9, first=0, count=500, p=(2e-3, 2e-3), q=(2e-3, 2e-3, 2e-3), max_attempts=256, pad=1)
    cases += 8
    hand = HandMadeGate()
    eff = hand.sequence[0]
    by_hand = dict(tables=([(eff, hand.regions, 5, hand.site_loc, hand.site_regions)], hand.sequence[3], hand.sequence[4],
                           [(hand.wait_eff, hand.wait_count)]), arguments=hand.arguments(), ldr=hand.ldw + 2, preparations=1)
    out += case(**by_hand, seed=10, first=0, count=400, p=(2e-2, 2e-2), q=(1e-2, 1e-2, 1e-2), max_attempts=256)
    cases += 1
    blank = lambda rows: np.zeros((rows, 2, 2), dtype=np.uint64)
    for kwargs, text in ((dict(wait_eff=blank(513), wait_count=[513, 0]), "has 513 wait rows, a region holds 0 <= wait rows <= 512"),
                         (dict(wait_eff=blank(3), wait_count=[0, 3]), "is not retried but has 3 wait rows"),
                         (dict(q=(0.6, 0.6, 0.0)), "the waiting probabilities must be non-negative and sum to at most 1"),
                         (dict(q=(-0.1, 0.0, 0.0)), "the waiting probabilities must be non-negative and sum to at most 1"),
                         (dict(p=(1.5, 0.0)), "needs 0 <= p_1, p_2 <= 1"), (dict(max_attempts=0), "needs 1 <= max_attempts <= 65536, got 0"),
                         (dict(pad=-1), "nsteps + F + 2 = 5 words"), (dict(first=-1), "negative range")):
        args = dict(by_hand, seed=1, first=0, count=4, p=p, q=q, max_attempts=256, text=text)
        args.update(kwargs)
        out += case(**args)
        cases += 1
    out += case(tables=None, arguments=many_wait_sizes([1, 2, 3, 4]), ldr=5, preparations=4, seed=1, first=0, count=4, p=p, q=q, max_attempts=256,
                text="more than GF2_RETRY_GATE_WAIT_MAX_SIZES = 3 distinct wait sizes")
    cases += 1
    return out, cases


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    path = tmp_path_factory.mktemp("retry_gate_wait_host") / "cases.bin"
    parts, count = retry_gate_wait_cases()
    stream(parts + [0]).tofile(str(path))
    return str(path), count


@pytest.mark.parametrize("kind", ["tsan", "asan"])
def test_retry_gate_wait_host_statement_under_sanitizer(kind, cases, tmp_path):
    flags, runtimes, marker = SANITIZERS[kind]
    for name in runtimes:                                     # the runtime goes into the program itself
        static = subprocess.run(["g++", "-print-file-name=lib%s.a" % name], capture_output=True, text=True).stdout.strip()
        if not (os.path.isabs(static) and os.path.exists(static)):
            pytest.skip("lib%s.a is not installed" % name)
        flags = flags + ["-static-lib%s" % name]
    program = str(tmp_path / ("retry_gate_wait_host_check_%s" % kind))
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include")] + flags +
                   [DRIVER, os.path.join(CSRC, "gf2_host.cpp"), "-o", program], check=True, capture_output=True, text=True)
    path, count = cases
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", TSAN_OPTIONS="exitcode=66 report_signal_unsafe=0",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    run = subprocess.run([program, path], env=env, capture_output=True, text=True, timeout=600, preexec_fn=without_aslr)
    report = run.stdout[-2000:] + run.stderr[-4000:]
    assert run.returncode == 0, report
    assert "retry gate wait host ok: %d cases" % count in run.stdout, report
    assert marker not in run.stderr and "runtime error" not in run.stderr, report
