"""Every refusal of the five solves' ABI entries (spmv_cg, spmv_cg_multi, spmv_cgls, spmv_bicgstab, spmv_gmres) that is made before the
device is touched: return code and the complete message.  Host structs with addresses that are never dereferenced, as
tests/test_gmres_abi.py.  The messages were recorded from the library before the entries came to share their checks
(csrc/solver_host.hpp) and are spelled out here; two of spmv_cg's (Jacobi on a handle that is not CSR, or without its arrays) were
made behind the device's set-up then and are taken from that source."""
import ctypes as C

import pytest

INVALID, UNSUPPORTED = -1, -5


class _Vec(C.Structure):  # struct spmv_vec's leading fields (csrc/common.hpp): ctx, n, d, owned
    _fields_ = [("ctx", C.c_void_p), ("n", C.c_int64), ("d", C.c_void_p), ("owned", C.c_bool)]


class _Mat(C.Structure):  # struct spmv_mat's leading fields: ctx, format, nrow, ncol, k, nnz, row_begin, a, b, v
    _fields_ = [("ctx", C.c_void_p), ("format", C.c_int32), ("nrow", C.c_int32), ("ncol", C.c_int32), ("k", C.c_int32),
                ("nnz", C.c_int64), ("row_begin", C.c_int64), ("a", C.c_void_p), ("b", C.c_void_p), ("v", C.c_void_p)]


COO, CSR, ELL = 0, 1, 3
NONE, JACOBI, SYMGS, ILU0 = 0, 1, 2, 3


def _mat(fmt=CSR, nrow=7, ncol=7, k=0, nnz=12, row_begin=0, arrays=True):
    return _Mat(ctx=None, format=fmt, nrow=nrow, ncol=ncol, k=k, nnz=nnz, row_begin=row_begin, a=16, b=16 if arrays else 0, v=16 if arrays else 0)


SQUARE = _mat()                       # 7 x 7 CSR
TALL = _mat(ncol=5)                   # 7 x 5 CSR
GONE = _mat(arrays=False)             # a CSR handle that released its arrays (panel_keep_csr = 0)
ELL7 = _mat(fmt=ELL, k=2)             # 7 x 7 ELL, two slots per row
COO7 = _mat(fmt=COO)
SHARD = _mat(row_begin=3)             # rows 3 .. 9 of a larger matrix
B_AT, X_AT = 0x10000, 0x20000         # never dereferenced
_CTX = C.c_int64(0)                   # any non-null context: the checks fail before it is used


def _vec(n, d):
    return _Vec(n=n, d=d)


def _square_call(lib, name, extra=()):
    """a call of spmv_cg / spmv_bicgstab / spmv_gmres (extra: gmres's restart, in front of max_iter) with one thing wrong"""
    iters, res = C.c_int32(0), C.c_double(0.0)

    def call(M=SQUARE, b=(7, B_AT), x=(7, X_AT), max_iter=10, rel_tol=1e-8, precond=NONE, extra=extra, null=False):
        bv, xv = _vec(*b), _vec(*x)
        rc = getattr(lib, name)(None if null else C.byref(_CTX), C.byref(M), C.byref(bv), C.byref(xv), *extra, max_iter, rel_tol, 1, precond,
                                C.byref(iters), C.byref(res))
        return rc, lib.spmv_last_error().decode()

    return call


def _square_cases(call, who, matrix, symgs_built):
    """(what, result, return code, message) of the refusals the three square single-vector solves share"""
    cases = [
        ("null argument", call(null=True), INVALID, f"{who}: null argument"),
        ("not square", call(M=TALL), INVALID, f"{who}: {matrix} is 7 x 5, not square"),
        ("length of b", call(b=(6, B_AT)), INVALID, f"{who}: b has 6 and x 7 entries, the matrix 7 rows"),
        ("length of x", call(x=(8, X_AT)), INVALID, f"{who}: b has 7 and x 8 entries, the matrix 7 rows"),
        ("max_iter < 0", call(max_iter=-1), INVALID, f"{who}: max_iter=-1 rel_tol=1e-08"),
        ("rel_tol < 0", call(rel_tol=-1e-8), INVALID, f"{who}: max_iter=10 rel_tol=-1e-08"),
        ("preconditioner 7", call(precond=7), INVALID, f"{who}: unknown preconditioner 7"),
        ("ILU(0) on ELL", call(M=ELL7, precond=ILU0), UNSUPPORTED, f"{who}: ILU(0) needs a CSR handle (format 3)"),
        ("ILU(0) on a shard", call(M=SHARD, precond=ILU0), INVALID, f"{who}: ILU(0) needs the whole square matrix (7 x 7, first row 3)"),
        ("ILU(0), arrays gone", call(M=GONE, precond=ILU0), INVALID, f"{who}: the CSR arrays are gone (panel_keep_csr = 0 released them)"),
        ("Jacobi on ELL", call(M=ELL7, precond=JACOBI), UNSUPPORTED, f"{who}: the Jacobi preconditioner reads the diagonal of a CSR handle"),
    ]
    if not symgs_built:
        cases.append(("symmetric Gauss-Seidel", call(precond=SYMGS), UNSUPPORTED,
                      f"{who}: the symmetric Gauss-Seidel preconditioner is not built for this solver"))
    return cases


def _check(cases):
    for what, (rc, err), code, message in cases:
        assert (rc, err) == (code, message), what


def test_cg_refusals(pkg):
    lib = pkg.capi.load()
    call = _square_call(lib, "spmv_cg")
    _check(_square_cases(call, "spmv_cg", "the matrix", symgs_built=True) + [
        ("alias", call(x=(7, B_AT)), INVALID, "spmv_cg: b and x must not alias"),
        # UNSUPPORTED with the words of a handle that is not CSR: spmv_cg's own rule (the other solves say INVALID, "gave up")
        ("Jacobi, arrays gone", call(M=GONE, precond=JACOBI), UNSUPPORTED, "spmv_cg: the Jacobi preconditioner reads the diagonal of a CSR handle"),
    ])


@pytest.mark.parametrize("name, extra", [("spmv_bicgstab", ()), ("spmv_gmres", (30,))])
def test_bicgstab_and_gmres_refusals(pkg, name, extra):
    lib = pkg.capi.load()
    call = _square_call(lib, name, extra)
    cases = _square_cases(call, name, "the matrix (shard)", symgs_built=False) + [
        ("overlap", call(x=(7, B_AT + 8 * 3)), INVALID, f"{name}: b and x must not overlap"),
        ("the same address", call(x=(7, B_AT)), INVALID, f"{name}: b and x must not overlap"),
        ("Jacobi, arrays gone", call(M=GONE, precond=JACOBI), INVALID,
         f"{name}: this handle gave up its CSR arrays (panel_keep_csr = 0): no diagonal for the Jacobi preconditioner"),
    ]
    if name == "spmv_gmres":
        cases += [
            ("restart -1", call(extra=(-1,)), INVALID, "spmv_gmres: restart=-1, must be 1 .. 64 (0: 30)"),
            ("restart 65", call(extra=(65,)), INVALID, "spmv_gmres: restart=65, must be 1 .. 64 (0: 30)"),
        ]
    _check(cases)


def test_cg_multi_refusals(pkg):
    lib = pkg.capi.load()
    iters, res = (C.c_int32 * 65)(), (C.c_double * 65)()
    who = "spmv_cg_multi"

    def call(M=SQUARE, k=3, B=(21, B_AT), X=(21, X_AT), max_iter=10, rel_tol=1e-8, precond=NONE, null=False):
        bv, xv = _vec(*B), _vec(*X)
        rc = lib.spmv_cg_multi(None if null else C.byref(_CTX), C.byref(M), k, C.byref(bv), C.byref(xv), max_iter, rel_tol, 1, precond, iters, res)
        return rc, lib.spmv_last_error().decode()

    _check([
        ("null argument", call(null=True), INVALID, f"{who}: null argument"),
        ("k = 0", call(k=0, B=(0, B_AT), X=(0, X_AT)), INVALID, f"{who}: k = 0, must be in [1, 64]"),
        ("k = 65", call(k=65, B=(455, B_AT), X=(455, X_AT)), INVALID, f"{who}: k = 65, must be in [1, 64]"),
        ("not square", call(M=TALL), INVALID, f"{who}: the matrix is 7 x 5, not square"),
        ("length of B", call(B=(20, B_AT)), INVALID, f"{who}: B has 20 and X 21 entries, nrow * k = 7 * 3"),
        ("length of X", call(X=(24, X_AT)), INVALID, f"{who}: B has 21 and X 24 entries, nrow * k = 7 * 3"),
        ("overlap", call(X=(21, B_AT + 8 * 20)), INVALID, f"{who}: B and X must not overlap"),
        ("max_iter < 0", call(max_iter=-1), INVALID, f"{who}: max_iter=-1 rel_tol=1e-08"),
        ("rel_tol < 0", call(rel_tol=-1e-8), INVALID, f"{who}: max_iter=10 rel_tol=-1e-08"),
        ("preconditioner 7", call(precond=7), INVALID, f"{who}: unknown preconditioner 7"),
        ("a COO handle", call(M=COO7), UNSUPPORTED, f"{who}: CSR and ELL handles only (format 0), as spmv_apply_multi"),
        ("symmetric Gauss-Seidel", call(precond=SYMGS), UNSUPPORTED, f"{who}: the symmetric Gauss-Seidel preconditioner is not built for k columns"),
        ("ILU(0)", call(precond=ILU0), UNSUPPORTED, f"{who}: the ILU(0) preconditioner is not built for k columns"),
        ("ILU(0) on ELL", call(M=ELL7, precond=ILU0), UNSUPPORTED, f"{who}: the ILU(0) preconditioner is not built for k columns"),
        ("ILU(0) on a shard", call(M=SHARD, precond=ILU0), UNSUPPORTED, f"{who}: the ILU(0) preconditioner is not built for k columns"),
        ("Jacobi on ELL", call(M=ELL7, precond=JACOBI), UNSUPPORTED, f"{who}: the Jacobi preconditioner reads the diagonal of a CSR handle"),
        ("the product, arrays gone", call(M=GONE), INVALID, f"{who}: this handle gave up its CSR arrays (panel_keep_csr = 0)"),
        ("Jacobi, arrays gone", call(M=GONE, precond=JACOBI), INVALID, f"{who}: this handle gave up its CSR arrays (panel_keep_csr = 0)"),
    ])


def test_cgls_refusals(pkg):
    lib = pkg.capi.load()
    iters, normal, res = C.c_int32(0), C.c_double(0.0), C.c_double(0.0)
    who = "spmv_cgls"

    def call(M=TALL, b=(7, B_AT), x=(5, X_AT), max_iter=10, rel_tol=1e-8, damp=0.0, null=False):
        bv, xv = _vec(*b), _vec(*x)
        rc = lib.spmv_cgls(None if null else C.byref(_CTX), C.byref(M), C.byref(bv), C.byref(xv), max_iter, rel_tol, 1, damp, C.byref(iters),
                           C.byref(normal), C.byref(res))
        return rc, lib.spmv_last_error().decode()

    _check([
        ("null argument", call(null=True), INVALID, f"{who}: null argument"),
        ("length of b", call(b=(6, B_AT)), INVALID, f"{who}: b has 6 entries, the matrix (shard) 7 rows"),
        ("length of x", call(x=(8, X_AT)), INVALID, f"{who}: x has 8 entries, the matrix 5 columns"),
        ("overlap", call(x=(5, B_AT + 8 * 6)), INVALID, f"{who}: b and x must not overlap"),
        ("max_iter < 0", call(max_iter=-1), INVALID, f"{who}: max_iter=-1 rel_tol=1e-08"),
        ("rel_tol < 0", call(rel_tol=-1e-8), INVALID, f"{who}: max_iter=10 rel_tol=-1e-08"),
        ("damp < 0", call(damp=-0.5), INVALID, f"{who}: damp=-0.5, must be finite and not negative"),
        ("damp = inf", call(damp=float("inf")), INVALID, f"{who}: damp=inf, must be finite and not negative"),
        ("damp = nan", call(damp=float("nan")), INVALID, f"{who}: damp=nan, must be finite and not negative"),
        ("the transposed product, arrays gone", call(M=_mat(ncol=5, arrays=False)), INVALID, f"{who}: this handle gave up its CSR arrays (panel_keep_csr = 0)"),
    ])
