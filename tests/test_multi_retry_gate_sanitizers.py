"""
gf2_mretry_gate_words_host (csrc/gf2_host.cpp) under ThreadSanitizer and AddressSanitizer + UBSan on the CPU box.  The test compiles
csrc/gf2_host.cpp together with the stand-alone driver tests/multi_retry_gate_host_check.cpp with -fsanitize=..., the sanitizer's
runtime linked into the program, and runs that program as it is: no interpreter loads the code, and nothing is preloaded.  The cases
are written here, inputs beside the words and attempts tests/multi_retry_gate_ref.py expects: two Steane programs (two frames with
two measurements and a row pitch wider than the words; three frames with CNOTs in both directions, from sample 2^40, with samples that
run out of attempts), one Reed-Muller program with one attempt per preparation, no samples at all, and the refused arguments.  The
driver holds every array in a heap block of exactly its size and runs the cases on one thread, then on two at once.
"""
import os
import subprocess

import numpy as np
import pytest

from quantum_css_codes_amd import stream_noise
from tests import multi_retry_gate_ref
from tests.test_ec_sanitizers import SANITIZERS, message, stream
from tests.test_host_sanitizers import CSRC, ROOT, without_aslr
from tests.test_multi_stream import CNOT_MEASURE, THREE, X_CNOT_TWO, multi

DRIVER = os.path.join(ROOT, "tests", "multi_retry_gate_host_check.cpp")
RATES = (2e-3, 3e-3)


def mretry_gate_cases():
    out, cases = [], 0

    def case(got, seed, first, count, p, max_attempts, pad=0, text="", **changed):
        names = ("eff", "locs", "flags", "types", "kinds", "a", "b", "nframes", "regions", "nregions", "site_loc", "site_regions")
        seq = dict(zip(names, got._retry_gate_sequence()))
        seq.update(changed)
        ldw = got.ldw + 1 + pad
        parts = [1, len(seq["locs"]), len(seq["types"]), len(seq["eff"]), seq["nframes"], len(seq["regions"]), len(seq["site_loc"]), seq["locs"],
                 seq["flags"], seq["types"], seq["kinds"], seq["a"], seq["b"], seq["eff"], seq["regions"], seq["nregions"], seq["site_loc"],
                 seq["site_regions"], seed, first, count, np.array(p, dtype=np.float64).view(np.int64), max_attempts, ldw, got.preparations,
                 message(text)]
        if not text:
            words, attempts, _ = multi_retry_gate_ref.retry_gate_words(got, seed, first, count, *p, max_attempts)
            padded = np.full((count, ldw), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
            padded[:, :got.ldw + 1] = words
            parts += [padded, attempts]
        return parts

    out += case(multi("steane", X_CNOT_TWO)[0], 1, 0, 1200, RATES, 256, pad=2)
    out += case(multi("steane", THREE)[0], 2, 1 << 40, 1000, RATES, 3)
    out += case(multi("rm15", CNOT_MEASURE)[0], 3, 7, 600, RATES, 1, pad=1)
    got = multi("steane", CNOT_MEASURE)[0]
    out += case(got, 4, 0, 0, RATES, 256)
    cases += 4

    def changed(array, at, value):
        array = array.copy()
        array[at] = value
        return array

    regions, counts, kinds = got.type_regions, got.type_nregions, got.block_kind
    site_loc, site_regions = got.type_site_loc, got.type_site_regions
    cnot_type = next(t for t, kind in enumerate(got.types) if kind.kind == stream_noise.CNOT)
    cnot_region = int(counts[:cnot_type].sum())
    cnot_site = int(site_regions[:cnot_region].sum())
    retried = int(np.flatnonzero(regions[:, 2] == 1)[0])
    for kwargs, text in ((dict(regions=changed(regions, (cnot_region, 2), 1)), "one region that is not retried"),
                         (dict(regions=changed(regions, (retried, 1), regions[retried, 1] + 1)), "do not partition its"),
                         (dict(site_regions=changed(site_regions, (retried, 0), site_regions[retried, 0] + 1)), "sites' locations, not its"),
                         (dict(site_loc=changed(site_loc, cnot_site + 1, 0)), "do not partition its locations 0 .. 13: CNOT site 1 at location 0"),
                         (dict(site_loc=changed(changed(site_loc, cnot_site + 1, 4), cnot_site + 2, 2)), "CNOT sites of region 0 of block type"),
                         (dict(max_attempts=0), "1 <= max_attempts <= 65536, got 0"), (dict(max_attempts=65537), "got 65537"),
                         (dict(pad=-1), "ldw must be at least the sequence's nsteps + F + 1"), (dict(nframes=5), "1 <= nframes <= 4"),
                         (dict(kinds=changed(kinds, 3, 3)), "is a FINAL step"), (dict(first=-1), "negative range"),
                         (dict(p=(0.5, 1.5)), "needs 0 <= p_1, p_2 <= 1")):
        args = dict(seed=5, first=0, count=3, p=RATES, max_attempts=256)
        args.update(kwargs)
        out += case(got, text=text, **args)
        cases += 1
    return out, cases


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    path = tmp_path_factory.mktemp("multi_retry_gate_host") / "cases.bin"
    parts, count = mretry_gate_cases()
    stream(parts + [0]).tofile(str(path))
    return str(path), count


@pytest.mark.parametrize("kind", ["tsan", "asan"])
def test_multi_retry_gate_host_statement_under_sanitizer(kind, cases, tmp_path):
    flags, runtimes, marker = SANITIZERS[kind]
    for name in runtimes:                                     # the runtime goes into the program itself
        static = subprocess.run(["g++", "-print-file-name=lib%s.a" % name], capture_output=True, text=True).stdout.strip()
        if not (os.path.isabs(static) and os.path.exists(static)):
            pytest.skip("lib%s.a is not installed" % name)
        flags = flags + ["-static-lib%s" % name]
    program = str(tmp_path / ("multi_retry_gate_host_check_%s" % kind))
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include")] + flags +
                   [DRIVER, os.path.join(CSRC, "gf2_host.cpp"), "-o", program], check=True, capture_output=True, text=True)
    path, count = cases
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", TSAN_OPTIONS="exitcode=66 report_signal_unsafe=0",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    run = subprocess.run([program, path], env=env, capture_output=True, text=True, timeout=600, preexec_fn=without_aslr)
    report = run.stdout[-2000:] + run.stderr[-4000:]
    assert run.returncode == 0, report
    assert "multi retry gate host ok: %d cases" % count in run.stdout, report
    assert marker not in run.stderr and "runtime error" not in run.stderr, report
