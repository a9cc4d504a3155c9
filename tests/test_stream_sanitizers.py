"""
gf2_stream_words_host and gf2_stream_tally_host (csrc/gf2_host.cpp) under ThreadSanitizer and AddressSanitizer + UBSan on the CPU
box.  The test compiles csrc/gf2_host.cpp together with the stand-alone driver tests/stream_host_check.cpp with -fsanitize=..., the
sanitizer's runtime linked into the program, and runs that program as it is: no interpreter loads the code, and nothing is
preloaded.  The cases are written here, inputs beside the words and counts tests/stream_ref.py expects.  The Steane cycle's one
block table is read off the restated one-round cycle's single-fault outcome words (its round word, its final frame, its flag
word), so those inputs never went through native code: cycles of 3 and 12 rounds (one and three flag words, flag rows that
straddle a word, a row pitch wider than the words) under the oracle's sampler against ec_ref; the gate-free Steane program (a NONE
block, MEASURE steps) against ft_ref; no samples at all; and the refused arguments of both entry points.  The driver holds every
array in a heap block of exactly its size and runs the cases on one thread, then on two at once.
"""
import os
import subprocess

import numpy as np
import pytest

from oracle import cpu_ref
from quantum_css_codes_amd import stream_noise
from tests import gadget_enumerate_ref as ger
from tests import ec_ref, stream_ref
from tests.test_ec_sanitizers import SANITIZERS, message, stream
from tests.test_ft_sanitizers import STEANE, table
from tests.test_host_sanitizers import CSRC, ROOT, without_aslr

DRIVER = os.path.join(ROOT, "tests", "stream_host_check.cpp")
STREAM_OF_EC = (0, 1, 2, 3, 4, 5, 6, 7)                    # ec_ref's eight counts among the twelve
STREAM_OF_FT = (0, 8, 9, 10, 11, 6, 7)


def stream_cases():
    code = cpu_ref.CSSCode(STEANE, STEANE)
    (table1, entries1), (table2, entries2) = table(code._c1_syndromes, code.x_operator_matrix()[0]), table(code._c2_syndromes, code.z_operator_matrix()[0])
    tables = lambda r1=3, r2=3: [r1, entries1, r2, entries2] + table1 + table2
    one = ger.effect_words(ec_ref.Cycle(code, 1))          # (330, 2, 3): [final frame] [round 1] [flag word]
    ec_table = np.ascontiguousarray(one[:, :, [1, 0, 2]])  # (local, tail, flags)
    out, cases = [], 0

    def case(sequence, faults, ldw, flag_words, want_words=None, want=None, text_words="", text_tally="", r1=3, r2=3):
        type_eff, type_locations, type_flags, block_type, block_kind = sequence
        first, where, kind = faults
        parts = [1, len(type_locations), len(block_type), len(type_eff), type_locations, type_flags, block_type, block_kind, type_eff,
                 len(first) - 1, len(where), first, where, kind, ldw, flag_words] + tables(r1, r2) + [message(text_words), message(text_tally)]
        if not text_words:
            parts.append(want_words)
            if not text_tally:
                parts += list(want)
        return parts

    def counts12(ref, words, places):
        got, classes = ref.gadget.tally(ref.from_stream_layout(words))
        counts = np.zeros(12, dtype=np.uint64)
        counts[list(places)] = [int(v) for v in got]
        if ref.cycle:
            return counts, classes                          # the class byte's low five bits are ec_ref's
        return counts, (classes & 1) | ((classes >> 1) & 7) << 5

    for rounds, p, count, seed, first, pad in ((3, (0.001, 0.0005, 0.001), 3000, 1, 0, 0), (12, (0.0004, 0.0002, 0.0004), 2000, 2, 1 << 40, 2)):
        ref = stream_ref.cycle_reference(code, rounds)
        sequence = (ec_table, [330], [14], [0] * rounds + [-1], [1] * rounds + [3])
        faults = stream_ref.sampled_faults(ref.locations, seed, first, count, p)
        words = ref.words(seed, first, count, p)
        want = counts12(ref, words, STREAM_OF_EC)
        assert 100 < want[0][0] < count and want[0][3] >= 5
        padded = np.zeros((count, ref.ldw + pad), dtype=np.uint64)
        padded[:, :ref.ldw] = words
        out += case(sequence, faults, ref.ldw + pad, ref.ldw - ref.nsteps, padded, want)
        cases += 1
    nothing = (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint8))
    out += case(sequence, nothing, 16, 3, np.zeros(0, dtype=np.uint64), (np.zeros(12, dtype=np.uint64), np.zeros(0, dtype=np.uint8)))
    cases += 1

    gadget = stream_noise.StreamedGadget.program(code, "")  # (these tables come from gf2_circuit_effects_timed)
    ref = stream_ref.program_reference(code, "")
    program = gadget._sequence()
    faults = stream_ref.sampled_faults(ref.locations, 3, 5, 2000, (0.001, 0.0005, 0.001))
    words = ref.words(3, 5, 2000, (0.001, 0.0005, 0.001))
    want = counts12(ref, words, STREAM_OF_FT)
    assert 100 < want[0][0] < 2000 and want[0][9] >= 5
    out += case(program, faults, ref.ldw, gadget.flag_words, words, want)
    cases += 1

    a_fault = (np.array([0, 1]), np.array([5], dtype=np.int32), np.array([1], dtype=np.uint8))
    cycle2 = lambda **k: (k.get("eff", ec_table), k.get("locs", [330]), k.get("flags", [14]), k.get("types", [0, 0, -1]), k.get("kinds", [1, 1, 3]))
    its_words = np.concatenate([one[5, 0, [1]], one[5, 0, [0]] & np.uint64(~(1 << 31 | 1 << 63) & (2 ** 64 - 1)), one[5, 0, [0]], one[5, 0, [2]]])
    for sequence, faults, ldw, text in ((cycle2(flags=[65]), a_fault, 4, "at most 64"), (cycle2(flags=[13]), a_fault, 4, "at or above its 13 flag rows"),
                                        (cycle2(types=[0, -1, 0], kinds=[1, 3, 1]), a_fault, 4, "must be the last step"),
                                        (cycle2(types=[0, 0, 0], kinds=[1, 1, 1]), a_fault, 4, "0 MEASURE steps"), (cycle2(types=[0, 1, -1]), a_fault, 4, "type 1 outside"),
                                        (cycle2(), (a_fault[0], np.array([660], dtype=np.int32), a_fault[2]), 4, "outside [0, L = 660)"),
                                        (cycle2(), (a_fault[0], a_fault[1], np.array([0], dtype=np.uint8)), 4, "has kind 0"),
                                        (cycle2(), a_fault, 3, "ldw >= nsteps + F = 4 words")):
        out += case(sequence, faults, ldw, 1, text_words=text)
        cases += 1
    for flag_words, r1, r2, text in ((1, 32, 3, "<= 31"), (0, 3, 3, "F >= 1"), (2, 3, 3, "ldw >= nsteps + F = 5 words")):
        out += case(cycle2(), a_fault, 4, flag_words, its_words, text_tally=text, r1=r1, r2=r2)
        cases += 1
    return out, cases


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    path = tmp_path_factory.mktemp("stream_host") / "cases.bin"
    parts, count = stream_cases()
    stream(parts + [0]).tofile(str(path))
    return str(path), count


@pytest.mark.parametrize("kind", ["tsan", "asan"])
def test_stream_host_statements_under_sanitizer(kind, cases, tmp_path):
    flags, runtimes, marker = SANITIZERS[kind]
    for name in runtimes:                                     # the runtime goes into the program itself
        static = subprocess.run(["g++", "-print-file-name=lib%s.a" % name], capture_output=True, text=True).stdout.strip()
        if not (os.path.isabs(static) and os.path.exists(static)):
            pytest.skip("lib%s.a is not installed" % name)
        flags = flags + ["-static-lib%s" % name]
    program = str(tmp_path / ("stream_host_check_%s" % kind))
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include")] + flags +
                   [DRIVER, os.path.join(CSRC, "gf2_host.cpp"), "-o", program], check=True, capture_output=True, text=True)
    path, count = cases
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", TSAN_OPTIONS="exitcode=66 report_signal_unsafe=0",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    run = subprocess.run([program, path], env=env, capture_output=True, text=True, timeout=600, preexec_fn=without_aslr)
    report = run.stdout[-2000:] + run.stderr[-4000:]
    assert run.returncode == 0, report
    assert "stream host ok: %d cases" % count in run.stdout, report
    assert marker not in run.stderr and "runtime error" not in run.stderr, report
