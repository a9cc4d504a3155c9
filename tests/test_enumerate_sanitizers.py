"""
gf2_subset_unrank and gf2_circuit_enumerate_host (csrc/gf2_host.cpp) under AddressSanitizer + UBSan on the CPU box: the
`make asan` build of that translation unit, loaded by a child interpreter beside the sanitizer's runtime as
tests/test_host_sanitizers.py does.  Positions and counts go into exact-fit buffers (any overrun is ASan's), the unranked subsets
are ranked back with Python integers, the counts of every stratum add up to 3^w subsets per field at most and are additive over
rank ranges; refused arguments come back as GF2_E_ARG.  Host code only.
"""
import os
import subprocess
import sys

import pytest

from tests.test_host_sanitizers import CSRC, runtime_of, without_aslr

CHILD = r"""
import ctypes, math, sys
import numpy as np
lib = ctypes.CDLL(sys.argv[1])
i64, p = ctypes.c_int64, ctypes.c_void_p
lib.gf2_subset_unrank.argtypes = [i64, i64, i64, p]
lib.gf2_circuit_enumerate_host.argtypes = [p, i64, i64, i64, p, p, i64, i64, p, p, i64, i64, i64, i64, p]
lib.gf2_last_error.restype = ctypes.c_char_p

for nb in (1, 7, 21, 64, 65, 1025, 1 << 20):
    for w in range(min(nb, 8) + 1):
        top = min(math.comb(nb, w), 1 << 63)
        for rank in sorted({0, top // 3, top - 1}):
            pos = np.full(max(1, w), -7, dtype=np.int32)[:w]                                        # exact fit
            assert lib.gf2_subset_unrank(nb, w, rank, pos.ctypes.data if w else None) == 0, (nb, w, rank)
            assert sum(math.comb(int(s), k + 1) for k, s in enumerate(pos)) == rank and np.all(np.diff(pos) > 0)
            assert w == 0 or (0 <= pos[0] and pos[-1] < nb)
for args, text in (((7, 3, 35), b"rank"), ((7, 8, 0), b"weight"), ((0, 0, 0), b"positions"), ((1 << 20, 8, -1), b"rank")):
    assert lib.gf2_subset_unrank(*args, None) == -1 and text in lib.gf2_last_error()

rng = np.random.default_rng(20261017)
for r1, r2 in ((3, 3), (64, 63), (40, 70), (70, 70)):                                             # ldr = 3, 4, 4, 5
    kwx, kwz = (1 if r2 <= 63 else 2), (1 if r1 <= 63 else 2)
    ldr = kwx + kwz + 1
    for locations in (1, 9, 40):
        eff = np.zeros((locations, 2, ldr), dtype="<u8")
        for first, kw, r in ((0, kwx, r2), (kwx, kwz, r1)):
            bits = rng.integers(0, 2, (locations, 2, 64 * kw), dtype=np.uint8)
            bits[:, :, r:] = 0
            eff[:, :, first:first + kw] = np.packbits(bits, axis=2, bitorder="little").view("<u8")
        eff[:, :, ldr - 1] = rng.integers(0, 4, (locations, 2))
        keys = []
        for first, kw in ((kwx, kwz), (0, kwx)):                                                     # tables 1 (key_z) and 2 (key_x)
            seen = np.unique(eff[:, :, first:first + kw].reshape(-1, kw), axis=0)[::2]
            keys.append((np.ascontiguousarray(seen), rng.integers(0, 2, len(seen), dtype=np.uint8)))
        (k1, f1), (k2, f2) = keys
        for w in range(min(locations, 3) + 1):
            total = math.comb(locations, w)
            def run(first, count):
                out = np.full((w + 1, w + 1, 5), 0xFFFFFFFFFFFFFFFF, dtype="<u8")                  # exact fit, and overwritten
                rc = lib.gf2_circuit_enumerate_host(eff.ctypes.data, locations, ldr, r1, k1.ctypes.data, f1.ctypes.data, len(k1), r2,
                                                    k2.ctypes.data, f2.ctypes.data, len(k2), w, first, count, out.ctypes.data)
                assert rc == 0, lib.gf2_last_error()
                return out
            whole = run(0, total)
            assert int(whole.max()) <= total * 3**w and int(whole[:, :, 2].sum()) <= total * 3**w
            assert all(not whole[a, b].any() for a in range(w + 1) for b in range(w + 1) if a + b > w)
            cut = total // 3
            assert np.array_equal(run(0, cut) + run(cut, total - cut), whole)
        one = np.zeros(5, dtype="<u8")
        for w, first, count, text in ((locations + 1, 0, 1, b"weight"), (9, 0, 1, b"weight"), (1, locations, 1, b"leave"), (1, 0, -1, b"leave")):
            rc = lib.gf2_circuit_enumerate_host(eff.ctypes.data, locations, ldr, r1, k1.ctypes.data, f1.ctypes.data, len(k1), r2,
                                                k2.ctypes.data, f2.ctypes.data, len(k2), w, first, count, one.ctypes.data)
            assert rc == -1 and text in lib.gf2_last_error(), (w, first, count, lib.gf2_last_error())
print("enumerate ok")
"""


def test_enumerate_host_under_asan_ubsan(tmp_path):
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
    assert "enumerate ok" in run.stdout
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, report
