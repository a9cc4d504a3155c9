"""
gf2_mstream_words_host and gf2_mstream_tally_host (csrc/gf2_host.cpp) under ThreadSanitizer and AddressSanitizer + UBSan on the CPU
box.  The test compiles csrc/gf2_host.cpp together with the stand-alone driver tests/multi_stream_host_check.cpp with -fsanitize=...,
the sanitizer's runtime linked into the program, and runs that program as it is: no interpreter loads the code, and nothing is
preloaded.  The cases are written here, inputs beside the words and counts tests/multi_stream_ref.py expects: two Steane programs
under the oracle's sampler (two frames with two measurements, a row pitch wider than the words; three frames with CNOTs in both
directions), the hand-built two-fault sample on which the two settings of `records` differ, one Reed-Muller program, no samples at
all, and the refused arguments of both entry points.  The driver holds every array in a heap block of exactly its size and runs the
cases on one thread, then on two at once.
"""
import os
import subprocess

import numpy as np
import pytest

from quantum_css_codes_amd import stream_noise
from tests import stream_ref
from tests.test_ec_sanitizers import SANITIZERS, message, stream
from tests.test_ft_sanitizers import table
from tests.test_host_sanitizers import CSRC, ROOT, without_aslr
from tests.test_multi_stream import CNOT_MEASURE, THREE, X_CNOT_TWO, multi

DRIVER = os.path.join(ROOT, "tests", "multi_stream_host_check.cpp")


def mstream_cases():
    out, cases = [], 0

    def case(got, faults, want_words=None, want=(), pad=0, text_words="", text_tally="", r1=None, flag_words=None, **changed):
        code = got.code
        (table1, entries1), (table2, entries2) = table(code._c1_syndromes, code.x_operator_matrix()[0]), table(code._c2_syndromes, code.z_operator_matrix()[0])
        names = ("eff", "locs", "flags", "types", "kinds", "a", "b", "nframes")
        seq = dict(zip(names, got._sequence()))
        seq.update(changed)
        first, where, kind = faults
        ldw = got.ldw + pad
        parts = [1, len(seq["locs"]), len(seq["types"]), len(seq["eff"]), seq["nframes"], seq["locs"], seq["flags"], seq["types"], seq["kinds"],
                 seq["a"], seq["b"], seq["eff"], len(first) - 1, len(where), first, where, kind, ldw,
                 got.flag_words if flag_words is None else flag_words, code.r_1 if r1 is None else r1, entries1, code.r_2, entries2] + table1 + table2 + \
                [message(text_words), message(text_tally)]
        if not text_words:
            padded = np.full((len(first) - 1, ldw), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
            padded[:, :got.ldw] = want_words
            parts.append(padded)
            if not text_tally:
                parts += [np.array(counts, dtype=np.uint64) for counts in want]
        return parts

    def sampled(name, instructions, seed, first, count, p, pad=0):
        got, ref = multi(name, instructions)
        faults = stream_ref.sampled_faults(got.num_locations, seed, first, count, p)
        words = ref.outcome_words(*stream_ref.dense_faults(got.num_locations, *faults))
        want = [ref.tally(words, records) for records in ('reference', 'propagated')]
        assert want[0][0] > 50
        return case(got, faults, words, want, pad)

    out += sampled("steane", X_CNOT_TWO, 1, 0, 2500, (3e-4, 2e-4, 3e-4), pad=2)
    out += sampled("steane", THREE, 2, 1 << 40, 2000, (1e-4, 1e-4, 1e-4))
    out += sampled("rm15", CNOT_MEASURE, 3, 7, 1500, (1e-4, 1e-4, 1e-4), pad=1)
    cases += 3
    got, ref = multi("steane", (('I', 0), ('CNOT', 0, 1), ('MEASURE', 1)))          # tests/test_multi_stream.py test_records_matter_with_a_cnot
    where = got.locations()
    cnot = int(np.flatnonzero(got.block_kind == stream_noise.CNOT)[0])
    one = next(l for l in range(int(got.block_start[2]) - 1, -1, -1) if where[l, 1] < 7 and
               not got.words_of_faults([0, 1], [l], [1])[0, got.nsteps:].any())
    two = next(l for l in range(int(got.block_start[cnot]), int(got.block_start[cnot + 1])) if where[l, 1] == 7 + (int(where[one, 1]) + 1) % 7)
    faults = (np.array([0, 2], dtype=np.int64), np.array([one, two], dtype=np.int32), np.array([1, 1], dtype=np.uint8))
    words = ref.outcome_words(*stream_ref.dense_faults(got.num_locations, *faults))
    want = [ref.tally(words, records) for records in ('reference', 'propagated')]
    assert want[0][4] == 1 and want[1][4] == 0
    out += case(got, faults, words, want)
    nothing = (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint8))
    out += case(got, nothing, np.zeros((0, got.ldw), dtype=np.uint64), [[0] * 20, [0] * 20])
    cases += 2

    def changed(array, at, value):
        array = array.copy()
        array[at] = value
        return array

    kinds, frame_b = got.block_kind, got.block_b
    a_fault = (np.array([0, 1]), np.array([5], dtype=np.int32), np.array([1], dtype=np.uint8))
    for change, faults, pad, text in ((dict(nframes=5), a_fault, 0, "1 <= nframes <= 4"), (dict(kinds=changed(kinds, 3, 3)), a_fault, 0, "is a FINAL step"),
                                      (dict(b=changed(frame_b, cnot, 0)), a_fault, 0, "as control and as target"),
                                      (dict(b=changed(frame_b, 0, 1)), a_fault, 0, "its second frame must be -1"),
                                      (dict(kinds=changed(kinds, len(kinds) - 3, 1)), a_fault, 0, "same odd number of MEASURE steps"),
                                      (dict(), (a_fault[0], np.array([got.num_locations], dtype=np.int32), a_fault[2]), 0, "outside [0, L ="),
                                      (dict(), (a_fault[0], a_fault[1], np.array([0], dtype=np.uint8)), 0, "has kind 0"),
                                      (dict(), a_fault, -1, "ldw >= nsteps + F")):
        out += case(got, faults, pad=pad, text_words=text, **change)
        cases += 1
    its_words = got.words_of_faults(*a_fault)
    for kwargs, text in ((dict(r1=32), "<= 31"), (dict(flag_words=0), "F >= 1"), (dict(flag_words=got.flag_words + 1), "ldw >= nsteps + F")):
        out += case(got, a_fault, its_words, text_tally=text, **kwargs)
        cases += 1
    return out, cases


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    path = tmp_path_factory.mktemp("multi_stream_host") / "cases.bin"
    parts, count = mstream_cases()
    stream(parts + [0]).tofile(str(path))
    return str(path), count


@pytest.mark.parametrize("kind", ["tsan", "asan"])
def test_multi_stream_host_statements_under_sanitizer(kind, cases, tmp_path):
    flags, runtimes, marker = SANITIZERS[kind]
    for name in runtimes:                                     # the runtime goes into the program itself
        static = subprocess.run(["g++", "-print-file-name=lib%s.a" % name], capture_output=True, text=True).stdout.strip()
        if not (os.path.isabs(static) and os.path.exists(static)):
            pytest.skip("lib%s.a is not installed" % name)
        flags = flags + ["-static-lib%s" % name]
    program = str(tmp_path / ("multi_stream_host_check_%s" % kind))
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include")] + flags +
                   [DRIVER, os.path.join(CSRC, "gf2_host.cpp"), "-o", program], check=True, capture_output=True, text=True)
    path, count = cases
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", TSAN_OPTIONS="exitcode=66 report_signal_unsafe=0",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    run = subprocess.run([program, path], env=env, capture_output=True, text=True, timeout=600, preexec_fn=without_aslr)
    report = run.stdout[-2000:] + run.stderr[-4000:]
    assert run.returncode == 0, report
    assert "multi stream host ok: %d cases" % count in run.stdout, report
    assert marker not in run.stderr and "runtime error" not in run.stderr, report
