"""
gf2_circuit_effects_timed and gf2_ec_tally_host (csrc/gf2_host.cpp) under ThreadSanitizer and AddressSanitizer + UBSan on the CPU
box.  The test compiles csrc/gf2_host.cpp together with the stand-alone driver tests/ec_host_check.cpp with -fsanitize=..., the
sanitizer's runtime linked into the program, and runs that program as it is: no interpreter loads the code, and nothing is
preloaded.  The cases are written here, inputs beside the results tests/ec_ref.py expects: timed effect tables of random circuits
with RESET (sizes at the word boundaries, the counting call, refused arguments) and tallies of random outcome words of the Steane
cycle; the driver holds every array in a heap block of exactly its size and runs the cases on one thread, then on two at once.
"""
import os
import subprocess

import numpy as np
import pytest

from oracle import cpu_ref
from tests import ec_ref
from tests.test_host_sanitizers import CSRC, ROOT, without_aslr

DRIVER = os.path.join(ROOT, "tests", "ec_host_check.cpp")
SANITIZERS = {"tsan": (["-fsanitize=thread"], ["tsan"], "ThreadSanitizer"),
              "asan": (["-fsanitize=address,undefined"], ["asan", "ubsan"], "AddressSanitizer")}


def pack(mat):
    m, n = mat.shape
    ld = max(1, (n + 63) // 64)
    bits = np.zeros((m, ld * 64), dtype=np.uint8)
    bits[:, :n] = mat & 1
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little").view("<u8").reshape(m, ld))


def message(text):
    return [len(text)] + list(text.encode())


def stream(parts):
    """The parts (ints, lists, arrays of any integer type) as one run of little-endian int64 words; uint64 keeps its bits."""
    return np.concatenate([np.atleast_1d(np.asarray(p)).reshape(-1).astype("<u8" if np.asarray(p).dtype == np.uint64 else "<i8").view("<i8")
                           for p in parts])


def effects_cases(rng):
    out = []
    for n, ngates, nrows in ((1, 5, 1), (7, 12, 7), (64, 100, 64), (65, 150, 65), (130, 300, 129), (9, 0, 3)):
        gates = np.zeros((ngates, 3), dtype=np.int32)
        for g in range(ngates):
            kind = int(rng.integers(0, 4)) if n > 1 else int(rng.choice((0, 2, 3)))
            a, b = (rng.choice(n, 2, replace=False) if n > 1 else (0, 0))
            gates[g] = (kind, a, b)
        rows_x, rows_z = rng.integers(0, 2, (nrows, n), dtype=np.uint8), rng.integers(0, 2, (nrows, n), dtype=np.uint8)
        times = rng.integers(0, ngates + 1, nrows)
        locations = [(g, q) for g, (kind, a, b) in enumerate(gates.tolist()) for q in ((a, b) if kind == ec_ref.CNOT else (a,))]
        L, ldr = len(locations), (nrows + 63) // 64
        ident, zero = np.identity(L, dtype=np.uint8), np.zeros((L, L), dtype=np.uint8)
        eff = np.zeros((L, 2, ldr), dtype="<u8")
        for c, (f_x, f_z) in enumerate(((ident, zero), (zero, ident))):
            bits = np.zeros((L, 64 * ldr), dtype=np.uint8)
            bits[:, :nrows] = ec_ref.propagate_rows(gates, n, f_x, f_z, rows_x, rows_z, times)
            eff[:, c] = ec_ref.pack_words(bits)
        px, pz = pack(rows_x), pack(rows_z)
        out += [1, n, ngates, nrows, px.shape[1], ldr, L, gates, px, pz, times, message(""), eff, np.array(locations, dtype=np.int64)]
    one = np.ones(1, dtype="<u8")
    for bad, time, text in (((4, 0, 0), 2, "unknown kind"), ((3, 9, 0), 2, "outside"), ((1, 2, 2), 2, "with itself"), ((3, 1, 0), 3, "time 3")):
        out += [1, 4, 2, 1, 1, 1, 0, [(0, 1, 0), bad], one, one, [time], message(text)]
    return out


def tally_cases(rng):
    steane = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 1, 0, 0, 1, 1], [1, 0, 1, 0, 1, 0, 1]])
    code = cpu_ref.CSSCode(steane, steane)

    def table(entries, operator):
        keys = np.array([int(k) for k in entries], dtype="<u8")
        return [keys, [int(np.dot(operator, e)) & 1 for e in entries.values()]], len(keys)

    (table1, entries1), (table2, entries2) = table(code._c1_syndromes, code.x_operator_matrix()[0]), table(code._c2_syndromes, code.z_operator_matrix()[0])
    out = []
    for rounds, ldr in ((1, 3), (3, 5), (5, 8), (6, 8)):
        count = 700
        words = np.zeros((count, ldr), dtype="<u8")
        keys = rng.integers(0, 8, (count, rounds + 1), dtype=np.uint64) | rng.integers(0, 8, (count, rounds + 1), dtype=np.uint64) << np.uint64(32)
        keys[rng.random((count, rounds + 1)) < 0.4] = 0
        words[:, :rounds + 1] = keys
        words[:, 0] |= rng.integers(0, 2, count, dtype=np.uint64) << np.uint64(31) | rng.integers(0, 2, count, dtype=np.uint64) << np.uint64(63)
        words[rng.random(count) < 0.1, ldr - 1] = 1 << 40
        want, classes = ec_ref.tally(code, rounds, words)
        assert 100 < want[0] < count and want[1] > 10 and want[2] > 10          # accepted, rejected and flipped words all occur
        out += [2, count, ldr, ldr, rounds, 3, entries1, 3, entries2, words] + table1 + table2 + [message(""), want, classes]
    words = np.zeros(9, dtype="<u8")
    for rounds, r1, r2, ldr, text in ((1, 32, 3, 3, "<= 31"), (0, 3, 3, 3, "rounds"), (7, 3, 3, 8, "rounds"), (1, 3, 3, 9, "ldr <= 8"),
                                      (3, 3, 3, 4, "F >= 1")):
        out += [2, 1, 9, ldr, rounds, r1, entries1, r2, entries2, words] + table1 + table2 + [message(text)]
    return out


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    rng = np.random.default_rng(4)
    path = tmp_path_factory.mktemp("ec_host") / "cases.bin"
    stream(effects_cases(rng) + tally_cases(rng) + [0]).tofile(str(path))
    return str(path), 6 + 4 + 4 + 5


@pytest.mark.parametrize("kind", ["tsan", "asan"])
def test_ec_host_entry_points_under_sanitizer(kind, cases, tmp_path):
    flags, runtimes, marker = SANITIZERS[kind]
    for name in runtimes:                                     # the runtime goes into the program itself
        static = subprocess.run(["g++", "-print-file-name=lib%s.a" % name], capture_output=True, text=True).stdout.strip()
        if not (os.path.isabs(static) and os.path.exists(static)):
            pytest.skip("lib%s.a is not installed" % name)
        flags = flags + ["-static-lib%s" % name]
    program = str(tmp_path / ("ec_host_check_%s" % kind))
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include")] + flags +
                   [DRIVER, os.path.join(CSRC, "gf2_host.cpp"), "-o", program], check=True, capture_output=True, text=True)
    path, count = cases
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", TSAN_OPTIONS="exitcode=66 report_signal_unsafe=0",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    run = subprocess.run([program, path], env=env, capture_output=True, text=True, timeout=600, preexec_fn=without_aslr)
    report = run.stdout[-2000:] + run.stderr[-4000:]
    assert run.returncode == 0, report
    assert "ec host ok: %d cases" % count in run.stdout, report
    assert marker not in run.stderr and "runtime error" not in run.stderr, report
