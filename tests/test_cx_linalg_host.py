"""The one copy of the per-item complex Cholesky factor and triangular substitutions (csrc/cx_linalg.h) held to the
specification WITHOUT a GPU.

The header compiles as plain host C++; a small driver (tests/cx_linalg) runs ``chol``, ``fwd`` and ``bwd`` for float and
double, with the run-time size (NT = 0) and, for n = 2 and n = 4, with the compile-time size (NT = n).  Every output must be
``array_equal`` to ``oracle/mimo_f32.py::cholesky`` and to the substitution steps of ``tests/precoding_f32.py`` - in float32,
and in float64 through the ``precision`` switch of ``tests/precoded_channel_f32.py`` - and NT = n must give the bits of
NT = 0.  (The kernels that use the header are held to the same specification on the GPU: tests/test_gpu_precoding.py,
tests/test_gpu_precoded_channel.py.)
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle.mimo_f32 import C, cholesky                                   # noqa: E402
from precoding_f32 import _forward, _backward                             # noqa: E402
from precoded_channel_f32 import precision                                # noqa: E402

SIZES = (1, 2, 3, 4, 16)        # 1, 2, 4: compiled sizes of the kernels; 3: the run-time path; 16: the cap kD
COLS = (1, 5)
ALPHAS = (0.1, 0.0)
ITEMS = 6
CASES = [(n, cols, alpha) for n in SIZES for cols in COLS for alpha in ALPHAS]


def _inputs(dtype):
    """A = H H^H + alpha I [items, n, n] and right-hand sides X [items, n, cols] per case, from a fixed seed"""
    cd = np.complex64 if dtype is np.float32 else np.complex128
    rng = np.random.default_rng(20260)
    out = []
    for n, cols, alpha in CASES:
        m = 2 * n                                                        # alpha = 0 needs at least n columns for A > 0
        h = (rng.normal(size=(ITEMS, n, m)) + 1j * rng.normal(size=(ITEMS, n, m))) / np.sqrt(2 * m)
        a = h @ np.conj(np.swapaxes(h, 1, 2)) + alpha * np.eye(n)
        x = rng.normal(size=(ITEMS, n, cols)) + 1j * rng.normal(size=(ITEMS, n, cols))
        out.append((np.ascontiguousarray(a.astype(cd)), np.ascontiguousarray(x.astype(cd))))
    return out


def _spec(a, x, dtype):
    """(L lower triangle, L^-1 X, L^-H L^-1 X) of the specification, vectorised over the items"""
    n, cols = a.shape[1], x.shape[2]
    with np.errstate(all="ignore"), precision(dtype):
        A = [[C(a[:, i, j].real, a[:, i, j].imag) for j in range(n)] for i in range(n)]
        X = [[C(x[:, i, c].real, x[:, i, c].imag) for c in range(cols)] for i in range(n)]
        cholesky(A, n)
        L = np.zeros_like(a)
        for i in range(n):
            for j in range(i + 1):
                L[:, i, j].real, L[:, i, j].imag = A[i][j].re, A[i][j].im
        for c in range(cols):
            _forward(A, X, n, c)
        Y = np.zeros_like(x)
        for i in range(n):
            for c in range(cols):
                Y[:, i, c].real, Y[:, i, c].imag = X[i][c].re, X[i][c].im
        for c in range(cols):
            _backward(A, X, n, c)
        Z = np.zeros_like(x)
        for i in range(n):
            for c in range(cols):
                Z[:, i, c].real, Z[:, i, c].imag = X[i][c].re, X[i][c].im
    return L, Y, Z


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cx_linalg") / "cx_linalg_main"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas",
                           "-I", os.path.join(ROOT, "sionna_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "cx_linalg", "cx_linalg_main.cpp")])
    return exe


def _run(driver, tmp_path, dtype):
    """per case: {0: (L, Y, Z) of NT = 0, n: (L, Y, Z) of NT = n where the driver has one}"""
    cd = np.complex64 if dtype is np.float32 else np.complex128
    cases = _inputs(dtype)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for a, x in cases:
            f.write(np.array([a.shape[1], x.shape[2], a.shape[0]], np.int32).tobytes())
            f.write(a.tobytes())
            f.write(x.tobytes())
    subprocess.check_call([str(driver), "f32" if dtype is np.float32 else "f64", str(fin), str(fout)])
    flat = np.fromfile(fout, cd)
    got, pos = [], 0
    for a, x in cases:
        n = a.shape[1]
        res = {}
        for nt in (0, n) if n in (2, 4) else (0,):
            arrs = []
            for shape in (a.shape, x.shape, x.shape):
                arrs.append(flat[pos:pos + int(np.prod(shape))].reshape(shape))
                pos += int(np.prod(shape))
            res[nt] = tuple(arrs)
        got.append(res)
    assert pos == flat.size
    return cases, got


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_header_matches_specification_bit_for_bit(driver, tmp_path, dtype):
    cases, got = _run(driver, tmp_path, dtype)
    for (n, cols, alpha), (a, x), res in zip(CASES, cases, got):
        ref = _spec(a, x, dtype)
        assert all(np.isfinite(r).all() for r in ref), f"the specification is not finite at n={n} alpha={alpha}"
        for nt, out in res.items():
            for name, g, r in zip(("L", "L^-1 X", "L^-H L^-1 X"), out, ref):
                assert g.dtype == r.dtype and np.array_equal(g, r), \
                    f"{name} n={n} cols={cols} alpha={alpha} NT={nt}: {np.mean(g != r):.3e} of the entries differ"


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_compile_time_size_gives_the_bits_of_the_run_time_size(driver, tmp_path, dtype):
    _, got = _run(driver, tmp_path, dtype)
    seen = set()
    for (n, cols, alpha), res in zip(CASES, got):
        if n in res and n != 0:
            seen.add(n)
            for g0, gn in zip(res[0], res[n]):
                assert np.array_equal(g0.view(g0.real.dtype), gn.view(gn.real.dtype)), f"n={n} cols={cols} alpha={alpha}"
    assert seen == {2, 4}
