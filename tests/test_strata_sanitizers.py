"""
gf2_stratum_errors (csrc/gf2_host.cpp) under AddressSanitizer + UBSan on the CPU box: the `make asan` build of that translation
unit, loaded by a child interpreter beside the sanitizer's runtime as tests/test_host_sanitizers.py does, writes the strata of
sizes at the word boundaries into exact-fit buffers (any overrun is ASan's) and checks the weight of every row; refused
arguments come back as GF2_E_ARG.
"""
import os
import subprocess
import sys

import pytest

from tests.test_host_sanitizers import CSRC, runtime_of, without_aslr

CHILD = r"""
import ctypes, sys
import numpy as np
lib = ctypes.CDLL(sys.argv[1])
i64, u64, p, dbl = ctypes.c_int64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_double
lib.gf2_stratum_errors.argtypes = [i64, i64, u64, i64, i64, dbl, dbl, dbl, p, p, i64]
lib.gf2_last_error.restype = ctypes.c_char_p

def weight(words):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=1).sum(axis=1)

for nb in (1, 7, 63, 64, 65, 128, 129, 513, 1030, 1 << 20):
    ld = (nb + 63) // 64
    for w in sorted(w for w in {0, 1, 2, min(nb, 16), nb if nb <= 129 else 3} if w <= nb):
        for first in (0, (1 << 40) + 777):
            count = 5 if nb > 4096 else 64
            ex = np.full((count, ld), 0xFFFFFFFFFFFFFFFF, dtype="<u8"); ez = ex.copy()                  # exact fit, and overwritten
            assert lib.gf2_stratum_errors(nb, w, 20261017, first, count, 2.0, 0.0, 5.0, ex.ctypes.data, ez.ctypes.data, ld) == 0
            assert np.all(weight(ex | ez) == w) and not np.any(ex & ez), (nb, w)
            if nb & 63:
                assert not np.any((ex | ez)[:, -1] >> np.uint64(nb & 63))                                 # pad bits zero
one = np.zeros((1, 1), dtype="<u8")
for args, text in (((7, 8, 0, 0, 1, 1.0, 1.0, 1.0), b"outside"), ((7, 1, 0, 0, -1, 1.0, 1.0, 1.0), b"negative"),
                   ((7, 1, 0, 0, 1, 0.0, 0.0, 0.0), b"kind weights"), ((65, 1, 0, 0, 1, 1.0, 1.0, 1.0), b"lde")):
    assert lib.gf2_stratum_errors(*args, one.ctypes.data, one.ctypes.data, 1) == -1
    assert text in lib.gf2_last_error()
print("stratum errors ok")
"""


def test_stratum_errors_under_asan_ubsan(tmp_path):
    runtime = runtime_of("asan")
    if runtime is None:
        pytest.skip("libasan is not installed")
    subprocess.run(["make", "-C", CSRC, "asan"], check=True, capture_output=True)
    lib = os.path.join(CSRC, "build", "libgf2host_asan.so")
    stdcxx = subprocess.run(["g++", "-print-file-name=libstdc++.so.6"], capture_output=True, text=True).stdout.strip()
    preload = runtime + (" " + os.path.realpath(stdcxx) if os.path.isabs(stdcxx) and os.path.exists(stdcxx) else "")
    env = dict(os.environ, LD_PRELOAD=preload, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", ASAN_OPTIONS="detect_leaks=0",
               UBSAN_OPTIONS="halt_on_error=1 print_stacktrace=1")
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    run = subprocess.run([sys.executable, str(script), lib], env=env, capture_output=True, text=True, timeout=600,
                         preexec_fn=without_aslr)
    report = run.stdout[-2000:] + run.stderr[-4000:]
    assert run.returncode == 0, report
    assert "stratum errors ok" in run.stdout
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, report
