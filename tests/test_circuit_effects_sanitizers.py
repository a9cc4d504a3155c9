"""
gf2_circuit_effects (csrc/gf2_host.cpp) under AddressSanitizer + UBSan on the CPU box: the `make asan` build of that translation
unit, loaded by a child interpreter beside the sanitizer's runtime as tests/test_host_sanitizers.py does, makes effect tables of
random circuits (sizes at the word boundaries, exact-fit and counting calls, refused gates) and compares them with a forward
NumPy propagation of every single fault.
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
i64, p = ctypes.c_int64, ctypes.c_void_p
lib.gf2_circuit_effects.argtypes = [p, i64, i64, p, p, i64, i64, p, i64, i64, p, ctypes.POINTER(i64)]
lib.gf2_last_error.restype = ctypes.c_char_p

def pack(mat):
    m, n = mat.shape
    ld = max(1, (n + 63) // 64)
    bits = np.zeros((m, ld * 64), dtype=np.uint8)
    bits[:, :n] = mat & 1
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little").view("<u8").reshape(m, ld))

def unpack(words, n):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=-1, bitorder="little")[..., :n]

def propagate(gates, n, f_x, f_z):
    e_x = np.zeros((f_x.shape[0], n), dtype=np.uint8); e_z = np.zeros_like(e_x); loc = 0
    for kind, a, b in gates.tolist():
        if kind == 0:
            e_x[:, a], e_z[:, a] = e_z[:, a].copy(), e_x[:, a].copy()
        elif kind == 1:
            e_x[:, b] ^= e_x[:, a]; e_z[:, a] ^= e_z[:, b]
        for q in ((a, b) if kind == 1 else (a,)):
            e_x[:, q] ^= f_x[:, loc]; e_z[:, q] ^= f_z[:, loc]; loc += 1
    return e_x, e_z

rng = np.random.default_rng(3)
for n, ngates, nrows in ((1, 5, 1), (7, 12, 7), (64, 100, 64), (65, 150, 65), (130, 300, 129), (256, 400, 512), (9, 0, 3)):
    gates = np.zeros((ngates, 3), dtype=np.int32)
    for g in range(ngates):
        kind = int(rng.integers(0, 3)) if n > 1 else int(rng.choice((0, 2)))
        a, b = (rng.choice(n, 2, replace=False) if n > 1 else (0, 0))
        gates[g] = (kind, a, b)
    rows_x = rng.integers(0, 2, (nrows, n), dtype=np.uint8); rows_z = rng.integers(0, 2, (nrows, n), dtype=np.uint8)
    px, pz = pack(rows_x), pack(rows_z)
    total = i64(-1)
    args = (gates.ctypes.data if ngates else None, ngates, n, px.ctypes.data, pz.ctypes.data, nrows, px.shape[1])
    assert lib.gf2_circuit_effects(*args, None, 1, 0, None, ctypes.byref(total)) == 0          # counting call
    L = int(total.value)
    assert L == ngates + int((gates[:, 0] == 1).sum())
    ldr = (nrows + 63) // 64
    eff = np.zeros((max(1, L), 2, ldr), dtype="<u8"); locs = np.zeros((max(1, L), 2), dtype=np.int64)   # exact fit: any overrun is ASan's
    assert lib.gf2_circuit_effects(*args, eff.ctypes.data, ldr, L, locs.ctypes.data, ctypes.byref(total)) == 0
    bits = unpack(eff[:L], nrows)
    ident, zero = np.identity(L, dtype=np.uint8), np.zeros((L, L), dtype=np.uint8)
    for c, (f_x, f_z) in enumerate(((ident, zero), (zero, ident))):
        e_x, e_z = propagate(gates, n, f_x, f_z)
        want = (e_x.astype(np.int64) @ rows_x.T + e_z.astype(np.int64) @ rows_z.T) & 1
        assert np.array_equal(bits[:, c], want), (n, ngates, c)
for bad, text in (((3, 0, 0), b"unknown kind"), ((1, 0, 9), b"outside"), ((1, 2, 2), b"with itself")):
    gates = np.array([(0, 1, 0), bad], dtype=np.int32)
    one = np.ones((1, 1), dtype="<u8")
    assert lib.gf2_circuit_effects(gates.ctypes.data, 2, 4, one.ctypes.data, one.ctypes.data, 1, 1, None, 1, 0, None, ctypes.byref(total)) == -1
    assert text in lib.gf2_last_error()
print("circuit effects ok")
"""


def test_circuit_effects_under_asan_ubsan(tmp_path):
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
    assert "circuit effects ok" in run.stdout
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, report
