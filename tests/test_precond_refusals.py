"""Which solver takes which preconditioner on which handle, and what the preconditioners' parameters answer: every refusal that is
made before the device is touched, return code and the complete message.  Host structs with addresses that are never dereferenced,
as tests/test_solver_refusals.py.  The (code, message) pairs were recorded from the library before the preconditioners' host side
went through one table (csrc/precond.hpp) and are spelled out here, not computed.

The first table is the cross product of the entries {spmv_cg, spmv_cg_multi, spmv_bicgstab, spmv_gmres, spmv_lobpcg, spmv_refine over
CG, spmv_refine over BiCGSTAB} x the preconditioners 2 .. 6 x the handles {ELL, COO, a shard, arrays gone, not square}.  A
combination that the library ACCEPTS goes on to the device and would read the fake context, so it is not called: ACCEPTED names each
of them, and test_every_combination_is_listed holds the two tables to the whole product."""
import ctypes as C

import pytest

OK, INVALID, UNSUPPORTED = 0, -1, -5


class _Vec(C.Structure):  # struct spmv_vec's leading fields (csrc/common.hpp): ctx, n, d, owned
    _fields_ = [("ctx", C.c_void_p), ("n", C.c_int64), ("d", C.c_void_p), ("owned", C.c_bool)]


class _Mat(C.Structure):  # struct spmv_mat's leading fields: ctx, format, nrow, ncol, k, nnz, row_begin, a, b, v
    _fields_ = [("ctx", C.c_void_p), ("format", C.c_int32), ("nrow", C.c_int32), ("ncol", C.c_int32), ("k", C.c_int32),
                ("nnz", C.c_int64), ("row_begin", C.c_int64), ("a", C.c_void_p), ("b", C.c_void_p), ("v", C.c_void_p)]


COO, CSR, ELL = 0, 1, 3
PRECONDS = {"SYMGS": 2, "ILU0": 3, "CHEBYSHEV": 4, "AMG": 5, "FSAI": 6}
_CTX = C.c_int64(0)  # any non-null context: the checks fail before it is used (spmv_refine compares the handles' with it)


def _mat(fmt=CSR, nrow=7, ncol=7, k=0, nnz=12, row_begin=0, arrays=True):
    return _Mat(ctx=C.addressof(_CTX), format=fmt, nrow=nrow, ncol=ncol, k=k, nnz=nnz, row_begin=row_begin, a=16, b=16 if arrays else 0,
                v=16 if arrays else 0)


HANDLES = {
    "ELL": _mat(fmt=ELL, k=2),        # 7 x 7, two slots per row
    "COO": _mat(fmt=COO),
    "shard": _mat(row_begin=3),       # rows 3 .. 9 of a larger matrix
    "gone": _mat(arrays=False),       # a CSR handle that released its arrays (panel_keep_csr = 0)
    "not square": _mat(ncol=5),       # 7 x 5 CSR
}
B_AT, X_AT = 0x10000, 0x20000  # never dereferenced


def _call(lib, entry, M, precond):
    """one call of `entry` that is in order but for the preconditioner on this handle"""
    ctx, A = C.byref(_CTX), C.byref(M)
    iters, inner, res, resid = (C.c_int32 * 2)(), C.c_int32(0), (C.c_double * 2)(), (C.c_double * 2)()
    b, x = _Vec(n=7, d=B_AT), _Vec(n=7, d=X_AT)
    B, X = _Vec(n=14, d=B_AT), _Vec(n=14, d=X_AT)  # two columns
    if entry == "spmv_cg":
        rc = lib.spmv_cg(ctx, A, C.byref(b), C.byref(x), 10, 1e-8, 1, precond, iters, res)
    elif entry == "spmv_cg_multi":
        rc = lib.spmv_cg_multi(ctx, A, 2, C.byref(B), C.byref(X), 10, 1e-8, 1, precond, iters, res)
    elif entry == "spmv_bicgstab":
        rc = lib.spmv_bicgstab(ctx, A, C.byref(b), C.byref(x), 10, 1e-8, 1, precond, iters, res)
    elif entry == "spmv_gmres":
        rc = lib.spmv_gmres(ctx, A, C.byref(b), C.byref(x), 30, 10, 1e-8, 1, precond, iters, res)
    elif entry == "spmv_lobpcg":
        rc = lib.spmv_lobpcg(ctx, A, 2, 2, 0, C.byref(X), 10, 1e-8, precond, res, resid, iters)
    else:  # the handle is both A and A_lo: the inner solver's refusals are about A_lo
        solver = {"spmv_refine/cg": 0, "spmv_refine/bicgstab": 1}[entry]
        rc = lib.spmv_refine(ctx, A, A, C.byref(b), C.byref(x), solver, precond, 5, 10, 1e-4, 1e-10, iters, C.byref(inner), res)
    return rc, lib.spmv_last_error().decode()


ENTRIES = ("spmv_cg", "spmv_cg_multi", "spmv_bicgstab", "spmv_gmres", "spmv_lobpcg", "spmv_refine/cg", "spmv_refine/bicgstab")

# Not called: the library takes these and goes on to the device.  Symmetric Gauss-Seidel looks at the handle in its set-up, behind the
# device (conjugate gradients alone take it); the Chebyshev polynomial runs through the forward product of any whole square handle,
# and whether it can be set up with the Jacobi scaling is looked at there too.
ACCEPTED = {
    (entry, "SYMGS", handle) for entry in ("spmv_cg", "spmv_refine/cg") for handle in ("ELL", "COO", "shard", "gone")
} | {
    (entry, "CHEBYSHEV", handle)
    for entry in ("spmv_cg", "spmv_bicgstab", "spmv_gmres", "spmv_lobpcg", "spmv_refine/cg", "spmv_refine/bicgstab")
    for handle in ("ELL", "COO", "gone")
}

# (entry, preconditioner, handle): (return code, message)
REFUSALS = {
    ("spmv_cg", "SYMGS", "not square"): (INVALID, "spmv_cg: the matrix is 7 x 5, not square"),
    ("spmv_cg", "ILU0", "ELL"): (UNSUPPORTED, "spmv_cg: ILU(0) needs a CSR handle (format 3)"),
    ("spmv_cg", "ILU0", "COO"): (UNSUPPORTED, "spmv_cg: ILU(0) needs a CSR handle (format 0)"),
    ("spmv_cg", "ILU0", "shard"): (INVALID, "spmv_cg: ILU(0) needs the whole square matrix (7 x 7, first row 3)"),
    ("spmv_cg", "ILU0", "gone"): (INVALID, "spmv_cg: the CSR arrays are gone (panel_keep_csr = 0 released them)"),
    ("spmv_cg", "ILU0", "not square"): (INVALID, "spmv_cg: the matrix is 7 x 5, not square"),
    ("spmv_cg", "CHEBYSHEV", "shard"): (INVALID, "spmv_cg: Chebyshev needs the whole square matrix (7 x 7, first row 3)"),
    ("spmv_cg", "CHEBYSHEV", "not square"): (INVALID, "spmv_cg: the matrix is 7 x 5, not square"),
    ("spmv_cg", "AMG", "ELL"): (UNSUPPORTED, "spmv_cg: AMG needs a CSR handle (format 3)"),
    ("spmv_cg", "AMG", "COO"): (UNSUPPORTED, "spmv_cg: AMG needs a CSR handle (format 0)"),
    ("spmv_cg", "AMG", "shard"): (INVALID, "spmv_cg: AMG needs the whole square matrix (7 x 7, first row 3)"),
    ("spmv_cg", "AMG", "gone"): (INVALID, "spmv_cg: the CSR arrays are gone (panel_keep_csr = 0 released them)"),
    ("spmv_cg", "AMG", "not square"): (INVALID, "spmv_cg: the matrix is 7 x 5, not square"),
    ("spmv_cg", "FSAI", "ELL"): (UNSUPPORTED, "spmv_cg: FSAI needs a CSR handle (format 3)"),
    ("spmv_cg", "FSAI", "COO"): (UNSUPPORTED, "spmv_cg: FSAI needs a CSR handle (format 0)"),
    ("spmv_cg", "FSAI", "shard"): (INVALID, "spmv_cg: FSAI needs the whole square matrix (7 x 7, first row 3)"),
    ("spmv_cg", "FSAI", "gone"): (INVALID, "spmv_cg: the CSR arrays are gone (panel_keep_csr = 0 released them)"),
    ("spmv_cg", "FSAI", "not square"): (INVALID, "spmv_cg: the matrix is 7 x 5, not square"),
    ("spmv_cg_multi", "SYMGS", "ELL"): (UNSUPPORTED, "spmv_cg_multi: the symmetric Gauss-Seidel preconditioner is not built for k columns"),
    ("spmv_cg_multi", "SYMGS", "COO"): (UNSUPPORTED, "spmv_cg_multi: CSR and ELL handles only (format 0), as spmv_apply_multi"),
    ("spmv_cg_multi", "SYMGS", "shard"): (UNSUPPORTED, "spmv_cg_multi: the symmetric Gauss-Seidel preconditioner is not built for k columns"),
    ("spmv_cg_multi", "SYMGS", "gone"): (UNSUPPORTED, "spmv_cg_multi: the symmetric Gauss-Seidel preconditioner is not built for k columns"),
    ("spmv_cg_multi", "SYMGS", "not square"): (INVALID, "spmv_cg_multi: the matrix is 7 x 5, not square"),
    ("spmv_cg_multi", "ILU0", "ELL"): (UNSUPPORTED, "spmv_cg_multi: the ILU(0) preconditioner is not built for k columns"),
    ("spmv_cg_multi", "ILU0", "COO"): (UNSUPPORTED, "spmv_cg_multi: CSR and ELL handles only (format 0), as spmv_apply_multi"),
    ("spmv_cg_multi", "ILU0", "shard"): (UNSUPPORTED, "spmv_cg_multi: the ILU(0) preconditioner is not built for k columns"),
    ("spmv_cg_multi", "ILU0", "gone"): (UNSUPPORTED, "spmv_cg_multi: the ILU(0) preconditioner is not built for k columns"),
    ("spmv_cg_multi", "ILU0", "not square"): (INVALID, "spmv_cg_multi: the matrix is 7 x 5, not square"),
    ("spmv_cg_multi", "CHEBYSHEV", "ELL"): (UNSUPPORTED, "spmv_cg_multi: the Chebyshev preconditioner is not built for k columns"),
    ("spmv_cg_multi", "CHEBYSHEV", "COO"): (UNSUPPORTED, "spmv_cg_multi: CSR and ELL handles only (format 0), as spmv_apply_multi"),
    ("spmv_cg_multi", "CHEBYSHEV", "shard"): (UNSUPPORTED, "spmv_cg_multi: the Chebyshev preconditioner is not built for k columns"),
    ("spmv_cg_multi", "CHEBYSHEV", "gone"): (UNSUPPORTED, "spmv_cg_multi: the Chebyshev preconditioner is not built for k columns"),
    ("spmv_cg_multi", "CHEBYSHEV", "not square"): (INVALID, "spmv_cg_multi: the matrix is 7 x 5, not square"),
    ("spmv_cg_multi", "AMG", "ELL"): (UNSUPPORTED, "spmv_cg_multi: the AMG preconditioner is not built for k columns"),
    ("spmv_cg_multi", "AMG", "COO"): (UNSUPPORTED, "spmv_cg_multi: CSR and ELL handles only (format 0), as spmv_apply_multi"),
    ("spmv_cg_multi", "AMG", "shard"): (UNSUPPORTED, "spmv_cg_multi: the AMG preconditioner is not built for k columns"),
    ("spmv_cg_multi", "AMG", "gone"): (UNSUPPORTED, "spmv_cg_multi: the AMG preconditioner is not built for k columns"),
    ("spmv_cg_multi", "AMG", "not square"): (INVALID, "spmv_cg_multi: the matrix is 7 x 5, not square"),
    ("spmv_cg_multi", "FSAI", "ELL"): (UNSUPPORTED, "spmv_cg_multi: the FSAI preconditioner is not built for k columns"),
    ("spmv_cg_multi", "FSAI", "COO"): (UNSUPPORTED, "spmv_cg_multi: CSR and ELL handles only (format 0), as spmv_apply_multi"),
    ("spmv_cg_multi", "FSAI", "shard"): (UNSUPPORTED, "spmv_cg_multi: the FSAI preconditioner is not built for k columns"),
    ("spmv_cg_multi", "FSAI", "gone"): (UNSUPPORTED, "spmv_cg_multi: the FSAI preconditioner is not built for k columns"),
    ("spmv_cg_multi", "FSAI", "not square"): (INVALID, "spmv_cg_multi: the matrix is 7 x 5, not square"),
    ("spmv_bicgstab", "SYMGS", "ELL"): (UNSUPPORTED, "spmv_bicgstab: the symmetric Gauss-Seidel preconditioner is not built for this solver"),
    ("spmv_bicgstab", "SYMGS", "COO"): (UNSUPPORTED, "spmv_bicgstab: the symmetric Gauss-Seidel preconditioner is not built for this solver"),
    ("spmv_bicgstab", "SYMGS", "shard"): (UNSUPPORTED, "spmv_bicgstab: the symmetric Gauss-Seidel preconditioner is not built for this solver"),
    ("spmv_bicgstab", "SYMGS", "gone"): (UNSUPPORTED, "spmv_bicgstab: the symmetric Gauss-Seidel preconditioner is not built for this solver"),
    ("spmv_bicgstab", "SYMGS", "not square"): (INVALID, "spmv_bicgstab: the matrix (shard) is 7 x 5, not square"),
    ("spmv_bicgstab", "ILU0", "ELL"): (UNSUPPORTED, "spmv_bicgstab: ILU(0) needs a CSR handle (format 3)"),
    ("spmv_bicgstab", "ILU0", "COO"): (UNSUPPORTED, "spmv_bicgstab: ILU(0) needs a CSR handle (format 0)"),
    ("spmv_bicgstab", "ILU0", "shard"): (INVALID, "spmv_bicgstab: ILU(0) needs the whole square matrix (7 x 7, first row 3)"),
    ("spmv_bicgstab", "ILU0", "gone"): (INVALID, "spmv_bicgstab: the CSR arrays are gone (panel_keep_csr = 0 released them)"),
    ("spmv_bicgstab", "ILU0", "not square"): (INVALID, "spmv_bicgstab: the matrix (shard) is 7 x 5, not square"),
    ("spmv_bicgstab", "CHEBYSHEV", "shard"): (INVALID, "spmv_bicgstab: Chebyshev needs the whole square matrix (7 x 7, first row 3)"),
    ("spmv_bicgstab", "CHEBYSHEV", "not square"): (INVALID, "spmv_bicgstab: the matrix (shard) is 7 x 5, not square"),
    ("spmv_bicgstab", "AMG", "ELL"): (UNSUPPORTED, "spmv_bicgstab: AMG needs a CSR handle (format 3)"),
    ("spmv_bicgstab", "AMG", "COO"): (UNSUPPORTED, "spmv_bicgstab: AMG needs a CSR handle (format 0)"),
    ("spmv_bicgstab", "AMG", "shard"): (INVALID, "spmv_bicgstab: AMG needs the whole square matrix (7 x 7, first row 3)"),
    ("spmv_bicgstab", "AMG", "gone"): (INVALID, "spmv_bicgstab: the CSR arrays are gone (panel_keep_csr = 0 released them)"),
    ("spmv_bicgstab", "AMG", "not square"): (INVALID, "spmv_bicgstab: the matrix (shard) is 7 x 5, not square"),
    ("spmv_bicgstab", "FSAI", "ELL"): (UNSUPPORTED, "spmv_bicgstab: FSAI needs a CSR handle (format 3)"),
    ("spmv_bicgstab", "FSAI", "COO"): (UNSUPPORTED, "spmv_bicgstab: FSAI needs a CSR handle (format 0)"),
    ("spmv_bicgstab", "FSAI", "shard"): (INVALID, "spmv_bicgstab: FSAI needs the whole square matrix (7 x 7, first row 3)"),
    ("spmv_bicgstab", "FSAI", "gone"): (INVALID, "spmv_bicgstab: the CSR arrays are gone (panel_keep_csr = 0 released them)"),
    ("spmv_bicgstab", "FSAI", "not square"): (INVALID, "spmv_bicgstab: the matrix (shard) is 7 x 5, not square"),
    ("spmv_gmres", "SYMGS", "ELL"): (UNSUPPORTED, "spmv_gmres: the symmetric Gauss-Seidel preconditioner is not built for this solver"),
    ("spmv_gmres", "SYMGS", "COO"): (UNSUPPORTED, "spmv_gmres: the symmetric Gauss-Seidel preconditioner is not built for this solver"),
    ("spmv_gmres", "SYMGS", "shard"): (UNSUPPORTED, "spmv_gmres: the symmetric Gauss-Seidel preconditioner is not built for this solver"),
    ("spmv_gmres", "SYMGS", "gone"): (UNSUPPORTED, "spmv_gmres: the symmetric Gauss-Seidel preconditioner is not built for this solver"),
    ("spmv_gmres", "SYMGS", "not square"): (INVALID, "spmv_gmres: the matrix (shard) is 7 x 5, not square"),
    ("spmv_gmres", "ILU0", "ELL"): (UNSUPPORTED, "spmv_gmres: ILU(0) needs a CSR handle (format 3)"),
    ("spmv_gmres", "ILU0", "COO"): (UNSUPPORTED, "spmv_gmres: ILU(0) needs a CSR handle (format 0)"),
    ("spmv_gmres", "ILU0", "shard"): (INVALID, "spmv_gmres: ILU(0) needs the whole square matrix (7 x 7, first row 3)"),
    ("spmv_gmres", "ILU0", "gone"): (INVALID, "spmv_gmres: the CSR arrays are gone (panel_keep_csr = 0 released them)"),
    ("spmv_gmres", "ILU0", "not square"): (INVALID, "spmv_gmres: the matrix (shard) is 7 x 5, not square"),
    ("spmv_gmres", "CHEBYSHEV", "shard"): (INVALID, "spmv_gmres: Chebyshev needs the whole square matrix (7 x 7, first row 3)"),
    ("spmv_gmres", "CHEBYSHEV", "not square"): (INVALID, "spmv_gmres: the matrix (shard) is 7 x 5, not square"),
    ("spmv_gmres", "AMG", "ELL"): (UNSUPPORTED, "spmv_gmres: AMG needs a CSR handle (format 3)"),
    ("spmv_gmres", "AMG", "COO"): (UNSUPPORTED, "spmv_gmres: AMG needs a CSR handle (format 0)"),
    ("spmv_gmres", "AMG", "shard"): (INVALID, "spmv_gmres: AMG needs the whole square matrix (7 x 7, first row 3)"),
    ("spmv_gmres", "AMG", "gone"): (INVALID, "spmv_gmres: the CSR arrays are gone (panel_keep_csr = 0 released them)"),
    ("spmv_gmres", "AMG", "not square"): (INVALID, "spmv_gmres: the matrix (shard) is 7 x 5, not square"),
    ("spmv_gmres", "FSAI", "ELL"): (UNSUPPORTED, "spmv_gmres: FSAI needs a CSR handle (format 3)"),
    ("spmv_gmres", "FSAI", "COO"): (UNSUPPORTED, "spmv_gmres: FSAI needs a CSR handle (format 0)"),
    ("spmv_gmres", "FSAI", "shard"): (INVALID, "spmv_gmres: FSAI needs the whole square matrix (7 x 7, first row 3)"),
    ("spmv_gmres", "FSAI", "gone"): (INVALID, "spmv_gmres: the CSR arrays are gone (panel_keep_csr = 0 released them)"),
    ("spmv_gmres", "FSAI", "not square"): (INVALID, "spmv_gmres: the matrix (shard) is 7 x 5, not square"),
    ("spmv_lobpcg", "SYMGS", "ELL"): (UNSUPPORTED, "spmv_lobpcg: the symmetric Gauss-Seidel preconditioner is not built for this solver"),
    ("spmv_lobpcg", "SYMGS", "COO"): (UNSUPPORTED, "spmv_lobpcg: the symmetric Gauss-Seidel preconditioner is not built for this solver"),
    ("spmv_lobpcg", "SYMGS", "shard"): (UNSUPPORTED, "spmv_lobpcg: the symmetric Gauss-Seidel preconditioner is not built for this solver"),
    ("spmv_lobpcg", "SYMGS", "gone"): (UNSUPPORTED, "spmv_lobpcg: the symmetric Gauss-Seidel preconditioner is not built for this solver"),
    ("spmv_lobpcg", "SYMGS", "not square"): (INVALID, "spmv_lobpcg: the matrix (shard) is 7 x 5, not square"),
    ("spmv_lobpcg", "ILU0", "ELL"): (UNSUPPORTED, "spmv_lobpcg: ILU(0) needs a CSR handle (format 3)"),
    ("spmv_lobpcg", "ILU0", "COO"): (UNSUPPORTED, "spmv_lobpcg: ILU(0) needs a CSR handle (format 0)"),
    ("spmv_lobpcg", "ILU0", "shard"): (INVALID, "spmv_lobpcg: ILU(0) needs the whole square matrix (7 x 7, first row 3)"),
    ("spmv_lobpcg", "ILU0", "gone"): (INVALID, "spmv_lobpcg: the CSR arrays are gone (panel_keep_csr = 0 released them)"),
    ("spmv_lobpcg", "ILU0", "not square"): (INVALID, "spmv_lobpcg: the matrix (shard) is 7 x 5, not square"),
    ("spmv_lobpcg", "CHEBYSHEV", "shard"): (INVALID, "spmv_lobpcg: Chebyshev needs the whole square matrix (7 x 7, first row 3)"),
    ("spmv_lobpcg", "CHEBYSHEV", "not square"): (INVALID, "spmv_lobpcg: the matrix (shard) is 7 x 5, not square"),
    ("spmv_lobpcg", "AMG", "ELL"): (UNSUPPORTED, "spmv_lobpcg: AMG needs a CSR handle (format 3)"),
    ("spmv_lobpcg", "AMG", "COO"): (UNSUPPORTED, "spmv_lobpcg: AMG needs a CSR handle (format 0)"),
    ("spmv_lobpcg", "AMG", "shard"): (INVALID, "spmv_lobpcg: AMG needs the whole square matrix (7 x 7, first row 3)"),
    ("spmv_lobpcg", "AMG", "gone"): (INVALID, "spmv_lobpcg: the CSR arrays are gone (panel_keep_csr = 0 released them)"),
    ("spmv_lobpcg", "AMG", "not square"): (INVALID, "spmv_lobpcg: the matrix (shard) is 7 x 5, not square"),
    ("spmv_lobpcg", "FSAI", "ELL"): (UNSUPPORTED, "spmv_lobpcg: FSAI needs a CSR handle (format 3)"),
    ("spmv_lobpcg", "FSAI", "COO"): (UNSUPPORTED, "spmv_lobpcg: FSAI needs a CSR handle (format 0)"),
    ("spmv_lobpcg", "FSAI", "shard"): (INVALID, "spmv_lobpcg: FSAI needs the whole square matrix (7 x 7, first row 3)"),
    ("spmv_lobpcg", "FSAI", "gone"): (INVALID, "spmv_lobpcg: the CSR arrays are gone (panel_keep_csr = 0 released them)"),
    ("spmv_lobpcg", "FSAI", "not square"): (INVALID, "spmv_lobpcg: the matrix (shard) is 7 x 5, not square"),
    ("spmv_refine/cg", "SYMGS", "not square"): (INVALID, "spmv_refine: the matrix is 7 x 5, not square"),
    ("spmv_refine/cg", "ILU0", "ELL"): (UNSUPPORTED, "spmv_cg: ILU(0) needs a CSR handle (format 3)"),
    ("spmv_refine/cg", "ILU0", "COO"): (UNSUPPORTED, "spmv_cg: ILU(0) needs a CSR handle (format 0)"),
    ("spmv_refine/cg", "ILU0", "shard"): (INVALID, "spmv_cg: ILU(0) needs the whole square matrix (7 x 7, first row 3)"),
    ("spmv_refine/cg", "ILU0", "gone"): (INVALID, "spmv_cg: the CSR arrays are gone (panel_keep_csr = 0 released them)"),
    ("spmv_refine/cg", "ILU0", "not square"): (INVALID, "spmv_refine: the matrix is 7 x 5, not square"),
    ("spmv_refine/cg", "CHEBYSHEV", "shard"): (INVALID, "spmv_cg: Chebyshev needs the whole square matrix (7 x 7, first row 3)"),
    ("spmv_refine/cg", "CHEBYSHEV", "not square"): (INVALID, "spmv_refine: the matrix is 7 x 5, not square"),
    ("spmv_refine/cg", "AMG", "ELL"): (UNSUPPORTED, "spmv_cg: AMG needs a CSR handle (format 3)"),
    ("spmv_refine/cg", "AMG", "COO"): (UNSUPPORTED, "spmv_cg: AMG needs a CSR handle (format 0)"),
    ("spmv_refine/cg", "AMG", "shard"): (INVALID, "spmv_cg: AMG needs the whole square matrix (7 x 7, first row 3)"),
    ("spmv_refine/cg", "AMG", "gone"): (INVALID, "spmv_cg: the CSR arrays are gone (panel_keep_csr = 0 released them)"),
    ("spmv_refine/cg", "AMG", "not square"): (INVALID, "spmv_refine: the matrix is 7 x 5, not square"),
    ("spmv_refine/cg", "FSAI", "ELL"): (UNSUPPORTED, "spmv_cg: FSAI needs a CSR handle (format 3)"),
    ("spmv_refine/cg", "FSAI", "COO"): (UNSUPPORTED, "spmv_cg: FSAI needs a CSR handle (format 0)"),
    ("spmv_refine/cg", "FSAI", "shard"): (INVALID, "spmv_cg: FSAI needs the whole square matrix (7 x 7, first row 3)"),
    ("spmv_refine/cg", "FSAI", "gone"): (INVALID, "spmv_cg: the CSR arrays are gone (panel_keep_csr = 0 released them)"),
    ("spmv_refine/cg", "FSAI", "not square"): (INVALID, "spmv_refine: the matrix is 7 x 5, not square"),
    ("spmv_refine/bicgstab", "SYMGS", "ELL"): (UNSUPPORTED, "spmv_bicgstab: the symmetric Gauss-Seidel preconditioner is not built for this solver"),
    ("spmv_refine/bicgstab", "SYMGS", "COO"): (UNSUPPORTED, "spmv_bicgstab: the symmetric Gauss-Seidel preconditioner is not built for this solver"),
    ("spmv_refine/bicgstab", "SYMGS", "shard"): (UNSUPPORTED, "spmv_bicgstab: the symmetric Gauss-Seidel preconditioner is not built for this solver"),
    ("spmv_refine/bicgstab", "SYMGS", "gone"): (UNSUPPORTED, "spmv_bicgstab: the symmetric Gauss-Seidel preconditioner is not built for this solver"),
    ("spmv_refine/bicgstab", "SYMGS", "not square"): (INVALID, "spmv_refine: the matrix is 7 x 5, not square"),
    ("spmv_refine/bicgstab", "ILU0", "ELL"): (UNSUPPORTED, "spmv_bicgstab: ILU(0) needs a CSR handle (format 3)"),
    ("spmv_refine/bicgstab", "ILU0", "COO"): (UNSUPPORTED, "spmv_bicgstab: ILU(0) needs a CSR handle (format 0)"),
    ("spmv_refine/bicgstab", "ILU0", "shard"): (INVALID, "spmv_bicgstab: ILU(0) needs the whole square matrix (7 x 7, first row 3)"),
    ("spmv_refine/bicgstab", "ILU0", "gone"): (INVALID, "spmv_bicgstab: the CSR arrays are gone (panel_keep_csr = 0 released them)"),
    ("spmv_refine/bicgstab", "ILU0", "not square"): (INVALID, "spmv_refine: the matrix is 7 x 5, not square"),
    ("spmv_refine/bicgstab", "CHEBYSHEV", "shard"): (INVALID, "spmv_bicgstab: Chebyshev needs the whole square matrix (7 x 7, first row 3)"),
    ("spmv_refine/bicgstab", "CHEBYSHEV", "not square"): (INVALID, "spmv_refine: the matrix is 7 x 5, not square"),
    ("spmv_refine/bicgstab", "AMG", "ELL"): (UNSUPPORTED, "spmv_bicgstab: AMG needs a CSR handle (format 3)"),
    ("spmv_refine/bicgstab", "AMG", "COO"): (UNSUPPORTED, "spmv_bicgstab: AMG needs a CSR handle (format 0)"),
    ("spmv_refine/bicgstab", "AMG", "shard"): (INVALID, "spmv_bicgstab: AMG needs the whole square matrix (7 x 7, first row 3)"),
    ("spmv_refine/bicgstab", "AMG", "gone"): (INVALID, "spmv_bicgstab: the CSR arrays are gone (panel_keep_csr = 0 released them)"),
    ("spmv_refine/bicgstab", "AMG", "not square"): (INVALID, "spmv_refine: the matrix is 7 x 5, not square"),
    ("spmv_refine/bicgstab", "FSAI", "ELL"): (UNSUPPORTED, "spmv_bicgstab: FSAI needs a CSR handle (format 3)"),
    ("spmv_refine/bicgstab", "FSAI", "COO"): (UNSUPPORTED, "spmv_bicgstab: FSAI needs a CSR handle (format 0)"),
    ("spmv_refine/bicgstab", "FSAI", "shard"): (INVALID, "spmv_bicgstab: FSAI needs the whole square matrix (7 x 7, first row 3)"),
    ("spmv_refine/bicgstab", "FSAI", "gone"): (INVALID, "spmv_bicgstab: the CSR arrays are gone (panel_keep_csr = 0 released them)"),
    ("spmv_refine/bicgstab", "FSAI", "not square"): (INVALID, "spmv_refine: the matrix is 7 x 5, not square"),
}


def test_every_combination_is_listed():
    product = {(e, p, h) for e in ENTRIES for p in PRECONDS for h in HANDLES}
    assert not (set(REFUSALS) & ACCEPTED)
    assert set(REFUSALS) | ACCEPTED == product
    assert len(REFUSALS) == 7 * 5 * 5 - 26


@pytest.mark.parametrize("entry, precond, handle", sorted(REFUSALS))
def test_preconditioner_refusals(pkg, entry, precond, handle):
    lib = pkg.capi.load()
    assert _call(lib, entry, HANDLES[handle], PRECONDS[precond]) == REFUSALS[(entry, precond, handle)]


# ---- the parameters: spmv_mat_set_param / spmv_mat_get_param on a handle of zeros ----------------------------------------------------
class _Handle(C.Structure):  # room for the whole struct spmv_mat behind its leading fields; only integers in it are read and written
    _fields_ = [("lead", _Mat), ("rest", C.c_byte * 65536)]


# (name, value): (return code, message) of spmv_mat_set_param
SET_PARAM = {
    ("symgs_order", 0): (OK, ""),
    ("symgs_order", 1): (OK, ""),
    ("symgs_order", 2): (INVALID, "symgs_order: 0 (row order) or 1 (multicolour), got 2"),
    ("ilu0_order", 0): (OK, ""),
    ("ilu0_order", 1): (OK, ""),
    ("ilu0_order", 2): (INVALID, "ilu0_order: 0 (row order) or 1 (multicolour), got 2"),
    ("fsai_level", 0): (INVALID, "fsai_level: 1 .. 3, got 0"),
    ("fsai_level", 2): (OK, ""),
    ("fsai_level", 4): (INVALID, "fsai_level: 1 .. 3, got 4"),
    ("cheby_degree", 0): (INVALID, "cheby_degree: 1 .. 64, got 0"),
    ("cheby_degree", 8): (OK, ""),
    ("cheby_degree", 65): (INVALID, "cheby_degree: 1 .. 64, got 65"),
    ("amg_level_kernel", -1): (INVALID, "amg_level_kernel: a CSR kernel id 1 .. 8 for every coarse handle of the next set-up, or 0 (AUTO), got -1"),
    ("amg_level_kernel", 3): (OK, ""),
    ("amg_level_kernel", 9): (INVALID, "amg_level_kernel: a CSR kernel id 1 .. 8 for every coarse handle of the next set-up, or 0 (AUTO), got 9"),
    ("symgs_nope", 1): (INVALID, "unknown parameter 'symgs_nope'"),
    ("ilu0_nope", 1): (INVALID, "unknown parameter 'ilu0_nope'"),
    ("cheby_nope", 1): (INVALID, "unknown parameter 'cheby_nope'"),
    ("amg_nope", 1): (INVALID, "unknown parameter 'amg_nope'"),
    ("fsai_nope", 1): (INVALID, "unknown parameter 'fsai_nope'"),
}

# name: (return code, message) of spmv_mat_get_param on a handle of zeros
GET_UNKNOWN = {
    "symgs_nope": (INVALID, "unknown parameter 'symgs_nope'"),
    "ilu0_nope": (INVALID, "unknown parameter 'ilu0_nope'"),
    "cheby_nope": (INVALID, "unknown parameter 'cheby_nope'"),
    "amg_nope": (INVALID, "unknown parameter 'amg_nope'"),
    "fsai_nope": (INVALID, "unknown parameter 'fsai_nope'"),
}


@pytest.mark.parametrize("name, value", sorted(SET_PARAM))
def test_set_param(pkg, name, value):
    lib = pkg.capi.load()
    h = _Handle(lead=_mat())
    rc = lib.spmv_mat_set_param(C.byref(h), name.encode(), value)
    assert (rc, lib.spmv_last_error().decode() if rc else "") == SET_PARAM[(name, value)]
    if name in ("symgs_order", "ilu0_order", "fsai_level", "cheby_degree", "amg_level_kernel") and rc == OK:  # what was set is what is read
        got = C.c_int64(-7)
        assert lib.spmv_mat_get_param(C.byref(h), name.encode(), C.byref(got)) == OK
        assert got.value == value


@pytest.mark.parametrize("name", sorted(GET_UNKNOWN))
def test_get_param_unknown_name(pkg, name):
    lib = pkg.capi.load()
    h = _Handle(lead=_mat())
    got = C.c_int64(-7)
    rc = lib.spmv_mat_get_param(C.byref(h), name.encode(), C.byref(got))
    assert (rc, lib.spmv_last_error().decode()) == GET_UNKNOWN[name]
    assert got.value == -7
