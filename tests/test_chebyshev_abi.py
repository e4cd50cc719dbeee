"""CPU-side checks of the Chebyshev preconditioner and the Lanczos estimate (spmv_chebyshev_*, spmv_lanczos; SPMV_PRECOND_CHEBYSHEV):
the library exports the six entry points, the coefficient table equals the NumPy twin's bit for bit, and every refusal that is made
before the device is touched - return code and the complete message - on host structs with addresses that are never dereferenced, in
the manner of tests/test_gmres_abi.py."""
import ctypes as C
import inspect
import math
import re
from pathlib import Path

import numpy as np
import pytest

import chebyshev_ref as cr

FUNCTIONS = ("spmv_chebyshev_coefficients", "spmv_lanczos", "spmv_chebyshev_setup", "spmv_chebyshev_info", "spmv_chebyshev_solve", "spmv_chebyshev")
INVALID, UNSUPPORTED = -1, -5
COO, CSR, ELL = 0, 1, 3
CHEBYSHEV = 4


class _Vec(C.Structure):  # struct spmv_vec's leading fields (csrc/common.hpp): ctx, n, d, owned
    _fields_ = [("ctx", C.c_void_p), ("n", C.c_int64), ("d", C.c_void_p), ("owned", C.c_bool)]


class _Mat(C.Structure):  # struct spmv_mat's leading fields: ctx, format, nrow, ncol, k, nnz, row_begin, a, b, v
    _fields_ = [("ctx", C.c_void_p), ("format", C.c_int32), ("nrow", C.c_int32), ("ncol", C.c_int32), ("k", C.c_int32),
                ("nnz", C.c_int64), ("row_begin", C.c_int64), ("a", C.c_void_p), ("b", C.c_void_p), ("v", C.c_void_p)]


def _mat(fmt=CSR, nrow=7, ncol=7, k=0, nnz=12, row_begin=0, arrays=True):
    return _Mat(ctx=None, format=fmt, nrow=nrow, ncol=ncol, k=k, nnz=nnz, row_begin=row_begin, a=16, b=16 if arrays else 0, v=16 if arrays else 0)


SQUARE, TALL, GONE, ELL7, SHARD = _mat(), _mat(ncol=5), _mat(arrays=False), _mat(fmt=ELL, k=2), _mat(row_begin=3)
R_AT, Z_AT = 0x10000, 0x20000  # never dereferenced
_CTX = C.c_int64(0)            # any non-null context: the checks fail before it is used


@pytest.mark.parametrize("name", FUNCTIONS)
def test_library_exports_the_entry_point(pkg, name):
    lib = pkg.capi.load()
    assert hasattr(lib, name), f"libspmv_hip.so does not export {name}"
    assert name in pkg.capi.SIGNATURES


def test_header_and_ctypes_table_agree(pkg):
    header = (Path(__file__).resolve().parent.parent / "include" / "spmv_abi.h").read_text()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(spmv_[a-z0-9_]+)\s*\(", body))) == sorted(pkg.capi.SIGNATURES)
    assert re.search(r"SPMV_PRECOND_CHEBYSHEV\s*=\s*4\b", header) and pkg.capi.PRECOND_CHEBYSHEV == 4
    for name, nargs in zip(FUNCTIONS, (6, 10, 6, 5, 4, 4)):
        assert len(pkg.capi.SIGNATURES[name][1]) == nargs, name
        decl = re.search(name + r"\s*\((.*?)\);", body, re.S).group(1)
        assert decl.count(",") + 1 == nargs, name


@pytest.mark.parametrize("degree, lmin, lmax", [(1, 1.0, 3.0), (4, 2.0 / 30.0, 2.0), (16, 0.05, 1.97), (64, 1e-3, 1.0)])
def test_the_coefficient_table_equals_the_twins_bit_for_bit(pkg, degree, lmin, lmax):
    c0, c1, c2 = pkg.capi.chebyshev_coefficients(degree, lmin, lmax)
    t0, t1, t2 = cr.coefficients(degree, lmin, lmax)
    assert np.float64(c0).tobytes() == np.float64(t0).tobytes()
    assert c1.tobytes() == t1.tobytes() and c2.tobytes() == t2.tobytes()
    assert len(c1) == degree and np.all(np.isfinite(c1)) and np.all(c2 > 0)


def test_the_coefficient_table_is_refused_on_bad_arguments(pkg):
    lib = pkg.capi.load()
    c0, c1, c2 = C.c_double(0.0), (C.c_double * 64)(), (C.c_double * 64)()
    who = "spmv_chebyshev_coefficients"
    cases = [
        ((0, 1.0, 2.0), f"{who}: degree=0, must be 1 .. 64"),
        ((65, 1.0, 2.0), f"{who}: degree=65, must be 1 .. 64"),
        ((4, 2.0, 2.0), f"{who}: lmin=2 lmax=2, must be finite with 0 < lmin < lmax"),
        ((4, 3.0, 2.0), f"{who}: lmin=3 lmax=2, must be finite with 0 < lmin < lmax"),
        ((4, math.nan, 2.0), f"{who}: lmin=nan lmax=2, must be finite with 0 < lmin < lmax"),
        ((4, 1.0, math.inf), f"{who}: lmin=1 lmax=inf, must be finite with 0 < lmin < lmax"),
        ((4, -1.0, 2.0), f"{who}: lmin=-1 lmax=2, must be finite with 0 < lmin < lmax"),
        ((4, 0.0, 2.0), f"{who}: lmin=0 lmax=2, must be finite with 0 < lmin < lmax"),
    ]
    for (degree, lmin, lmax), message in cases:
        assert lib.spmv_chebyshev_coefficients(degree, lmin, lmax, C.byref(c0), c1, c2) == INVALID, message
        assert lib.spmv_last_error().decode() == message
    assert lib.spmv_chebyshev_coefficients(4, 1.0, 2.0, None, c1, c2) == INVALID
    assert lib.spmv_last_error().decode() == f"{who}: null argument"


def test_null_arguments_are_refused_without_a_device(pkg):
    lib = pkg.capi.load()
    calls = {
        "spmv_lanczos": lambda: lib.spmv_lanczos(None, None, 0, 8, 1, None, None, None, None, None),
        "spmv_chebyshev_setup": lambda: lib.spmv_chebyshev_setup(None, None, 4, 1, 0.0, 0.0),
        "spmv_chebyshev_info": lambda: lib.spmv_chebyshev_info(None, None, None, None, None),
        "spmv_chebyshev_solve": lambda: lib.spmv_chebyshev_solve(None, None, None, None),
        "spmv_chebyshev": lambda: lib.spmv_chebyshev(None, None, None, None),
    }
    for name, call in calls.items():
        assert call() == INVALID, name
        assert lib.spmv_last_error().decode() == f"{name}: null argument"


def test_setup_refusals_without_a_device(pkg):
    lib = pkg.capi.load()
    who = "spmv_chebyshev_setup"

    def call(M=SQUARE, degree=4, scaled=1, lmin=0.0, lmax=0.0):
        return lib.spmv_chebyshev_setup(C.byref(_CTX), C.byref(M), degree, scaled, lmin, lmax), lib.spmv_last_error().decode()

    cases = [
        ("degree 0", call(degree=0), f"{who}: degree=0, must be 1 .. 64"),
        ("degree 65", call(degree=65), f"{who}: degree=65, must be 1 .. 64"),
        ("negative lmin", call(lmin=-1.0, lmax=2.0), f"{who}: lmin=-1 lmax=2, must be finite and not negative (0: estimated)"),
        ("lmax nan", call(lmax=math.nan), f"{who}: lmin=0 lmax=nan, must be finite and not negative (0: estimated)"),
        ("lmax inf", call(lmax=math.inf), f"{who}: lmin=0 lmax=inf, must be finite and not negative (0: estimated)"),
        ("lmin = lmax", call(lmin=2.0, lmax=2.0), f"{who}: lmin=2 lmax=2, must be lmin < lmax"),
        ("lmin > lmax", call(lmin=3.0, lmax=2.0), f"{who}: lmin=3 lmax=2, must be lmin < lmax"),
        ("not square", call(M=TALL), f"{who}: Chebyshev needs the whole square matrix (7 x 5, first row 0)"),
        ("a shard", call(M=SHARD), f"{who}: Chebyshev needs the whole square matrix (7 x 7, first row 3)"),
        ("scaled on ELL", call(M=ELL7), f"{who}: the Jacobi scaling reads the diagonal of a CSR handle (format 3)"),
        ("scaled, arrays gone", call(M=GONE), f"{who}: the CSR arrays are gone (panel_keep_csr = 0 released them): no diagonal for the Jacobi scaling"),
    ]
    for what, (rc, err), message in cases:
        assert (rc, err) == (INVALID, message), what


def test_solve_smoother_and_lanczos_refusals_without_a_device(pkg):
    lib = pkg.capi.load()
    for name in ("spmv_chebyshev_solve", "spmv_chebyshev"):
        first, second = ("r", "z") if name.endswith("solve") else ("b", "x")

        def call(M=SQUARE, r=(7, R_AT), z=(7, Z_AT)):
            rv, zv = _Vec(n=r[0], d=r[1]), _Vec(n=z[0], d=z[1])
            return getattr(lib, name)(C.byref(_CTX), C.byref(M), C.byref(rv), C.byref(zv)), lib.spmv_last_error().decode()

        cases = [
            ("not square", call(M=TALL), f"{name}: Chebyshev needs the whole square matrix (7 x 5, first row 0)"),
            ("a shard", call(M=SHARD), f"{name}: Chebyshev needs the whole square matrix (7 x 7, first row 3)"),
            ("length", call(r=(6, R_AT)), f"{name}: {first} has 6 and {second} 7 entries, the matrix 7 rows"),
            ("length", call(z=(8, Z_AT)), f"{name}: {first} has 7 and {second} 8 entries, the matrix 7 rows"),
            ("overlap", call(z=(7, R_AT + 8 * 3)), f"{name}: {first} and {second} must not overlap"),
            ("the same address", call(z=(7, R_AT)), f"{name}: {first} and {second} must not overlap"),
        ]
        for what, (rc, err), message in cases:
            assert (rc, err) == (INVALID, message), (name, what)
    lo, hi, done = C.c_double(0.0), C.c_double(0.0), C.c_int32(0)

    def lanczos(M=SQUARE, scaled=0, steps=8):
        rc = lib.spmv_lanczos(C.byref(_CTX), C.byref(M), scaled, steps, 1, C.byref(lo), C.byref(hi), None, None, C.byref(done))
        return rc, lib.spmv_last_error().decode()

    who = "spmv_lanczos"
    cases = [
        ("steps 0", lanczos(steps=0), f"{who}: steps=0, must be 1 .. 64"),
        ("steps 65", lanczos(steps=65), f"{who}: steps=65, must be 1 .. 64"),
        ("not square", lanczos(M=TALL), f"{who}: needs the whole square matrix (7 x 5, first row 0)"),
        ("a shard", lanczos(M=SHARD), f"{who}: needs the whole square matrix (7 x 7, first row 3)"),
        ("scaled on ELL", lanczos(M=ELL7, scaled=1), f"{who}: the Jacobi scaling reads the diagonal of a CSR handle (format 3)"),
        ("scaled, arrays gone", lanczos(M=GONE, scaled=1), f"{who}: the CSR arrays are gone (panel_keep_csr = 0 released them): no diagonal for the Jacobi scaling"),
    ]
    for what, (rc, err), message in cases:
        assert (rc, err) == (INVALID, message), what


@pytest.mark.parametrize("name, extra", [("spmv_cg", ()), ("spmv_bicgstab", ()), ("spmv_gmres", (30,))])
def test_the_solvers_take_the_preconditioner_and_refuse_on_the_host(pkg, name, extra):
    """4 is a known value: what refuses these calls is the shape, the shard, the lengths - before any device use, on structs that
    hold the leading fields alone"""
    lib = pkg.capi.load()
    iters, res = C.c_int32(0), C.c_double(0.0)
    matrix = "the matrix" if name == "spmv_cg" else "the matrix (shard)"

    def call(M=SQUARE, b=(7, R_AT), x=(7, Z_AT), null=False):
        bv, xv = _Vec(n=b[0], d=b[1]), _Vec(n=x[0], d=x[1])
        rc = getattr(lib, name)(None if null else C.byref(_CTX), C.byref(M), C.byref(bv), C.byref(xv), *extra, 10, 1e-8, 1, CHEBYSHEV, C.byref(iters),
                                C.byref(res))
        return rc, lib.spmv_last_error().decode()

    cases = [
        ("null argument", call(null=True), f"{name}: null argument"),
        ("not square", call(M=TALL), f"{name}: {matrix} is 7 x 5, not square"),
        ("length of b", call(b=(6, R_AT)), f"{name}: b has 6 and x 7 entries, the matrix 7 rows"),
        ("a shard", call(M=SHARD), f"{name}: Chebyshev needs the whole square matrix (7 x 7, first row 3)"),
    ]
    for what, (rc, err), message in cases:
        assert (rc, err) == (INVALID, message), what


def test_cg_multi_refuses_the_preconditioner(pkg):
    lib = pkg.capi.load()
    iters, res = (C.c_int32 * 4)(), (C.c_double * 4)()
    for M in (SQUARE, ELL7, SHARD):
        bv, xv = _Vec(n=21, d=R_AT), _Vec(n=21, d=Z_AT)
        rc = lib.spmv_cg_multi(C.byref(_CTX), C.byref(M), 3, C.byref(bv), C.byref(xv), 10, 1e-8, 1, CHEBYSHEV, iters, res)
        assert (rc, lib.spmv_last_error().decode()) == (UNSUPPORTED, "spmv_cg_multi: the Chebyshev preconditioner is not built for k columns")


def test_context_has_the_methods(pkg):
    for name in ("lanczos", "chebyshev_setup", "chebyshev_info", "chebyshev_solve", "chebyshev"):
        assert callable(getattr(pkg.capi.Context, name, None)), name
    sig = inspect.signature(pkg.capi.Context.chebyshev_setup)
    assert [p for p in sig.parameters][1:] == ["A", "degree", "scaled", "lmin", "lmax"]
    assert (sig.parameters["degree"].default, sig.parameters["scaled"].default, sig.parameters["lmin"].default, sig.parameters["lmax"].default) == (4, True, 0.0, 0.0)
    assert callable(pkg.capi.chebyshev_coefficients)
