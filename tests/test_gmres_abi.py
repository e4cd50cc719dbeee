"""CPU-side checks of restarted GMRES (spmv_gmres): the library exports it, its argument checks run before any device use - the
restart among them, on host structs with addresses that are never dereferenced - and the Python bindings have the methods."""
import ctypes as C
import inspect


def test_library_exports_gmres(pkg):
    lib = pkg.capi.load()
    assert hasattr(lib, "spmv_gmres"), "libspmv_hip.so does not export spmv_gmres"
    assert "spmv_gmres" in pkg.capi.SIGNATURES
    assert len(pkg.capi.SIGNATURES["spmv_gmres"][1]) == 11  # ctx, A, b, x, restart, max_iter, rel_tol, check_every, precond, iters, rel_resid


def test_null_arguments_are_refused_without_a_device(pkg):
    lib = pkg.capi.load()
    iters, res = C.c_int32(0), C.c_double(0.0)
    assert lib.spmv_gmres(None, None, None, None, 30, 10, 1e-8, 1, 0, C.byref(iters), C.byref(res)) == -1
    assert b"spmv_gmres" in lib.spmv_last_error()
    assert lib.spmv_gmres(None, None, None, None, 30, 10, 1e-8, 1, 1, None, None) == -1
    assert b"spmv_gmres" in lib.spmv_last_error()


class _Vec(C.Structure):  # struct spmv_vec's leading fields (csrc/common.hpp): ctx, n, d, owned
    _fields_ = [("ctx", C.c_void_p), ("n", C.c_int64), ("d", C.c_void_p), ("owned", C.c_bool)]


class _Mat(C.Structure):  # struct spmv_mat's leading fields: ctx, format, nrow, ncol, k, nnz, row_begin, a, b, v
    _fields_ = [("ctx", C.c_void_p), ("format", C.c_int32), ("nrow", C.c_int32), ("ncol", C.c_int32), ("k", C.c_int32),
                ("nnz", C.c_int64), ("row_begin", C.c_int64), ("a", C.c_void_p), ("b", C.c_void_p), ("v", C.c_void_p)]


def test_sizes_restart_and_preconditioner_are_refused_without_a_device(pkg):
    capi = pkg.capi
    lib = capi.load()
    ctx = C.c_int64(0)  # any non-null context: the checks fail before it is used
    A = _Mat(ctx=None, format=capi.FMT_CSR, nrow=7, ncol=7, k=0, nnz=12, row_begin=0, a=16, b=16, v=16)
    R = _Mat(ctx=None, format=capi.FMT_CSR, nrow=7, ncol=5, k=0, nnz=12, row_begin=0, a=16, b=16, v=16)
    G = _Mat(ctx=None, format=capi.FMT_CSR, nrow=7, ncol=7, k=0, nnz=12, row_begin=0, a=16, b=0, v=0)
    L = _Mat(ctx=None, format=capi.FMT_ELL, nrow=7, ncol=7, k=2, nnz=12, row_begin=0, a=16, b=16, v=16)
    b, x = _Vec(n=7, d=0x10000), _Vec(n=7, d=0x20000)
    iters, res = C.c_int32(0), C.c_double(0.0)

    def call(M=A, bv=b, xv=x, restart=30, max_iter=10, rel_tol=1e-8, precond=0):
        rc = lib.spmv_gmres(C.byref(ctx), C.byref(M), C.byref(bv), C.byref(xv), restart, max_iter, rel_tol, 1, precond, C.byref(iters), C.byref(res))
        return rc, lib.spmv_last_error()

    cases = {
        "restart 65": (call(restart=65), -1, b"restart"),
        "restart -1": (call(restart=-1), -1, b"restart"),
        "not square": (call(M=R), -1, b"square"),
        "b length": (call(bv=_Vec(n=6, d=0x10000)), -1, b"entries"),
        "x length": (call(xv=_Vec(n=8, d=0x20000)), -1, b"entries"),
        "overlap": (call(xv=_Vec(n=7, d=0x10000 + 8 * 3)), -1, b"overlap"),
        "max_iter": (call(max_iter=-1), -1, b"max_iter"),
        "rel_tol": (call(rel_tol=-1e-8), -1, b"rel_tol"),
        "precond": (call(precond=7), -1, b"unknown preconditioner"),
        "symgs": (call(precond=capi.PRECOND_SYMGS), -5, b"Gauss-Seidel"),
        "jacobi on ell": (call(M=L, precond=capi.PRECOND_JACOBI), -5, b"Jacobi"),
        "jacobi, arrays released": (call(M=G, precond=capi.PRECOND_JACOBI), -1, b"gave up"),
    }
    for what, ((rc, err), code, needle) in cases.items():
        assert rc == code and b"spmv_gmres" in err and needle in err, (what, rc, err)


def test_context_and_operator_have_gmres(pkg):
    assert callable(getattr(pkg.capi.Context, "gmres", None))
    sig = inspect.signature(pkg.capi.Context.gmres)
    assert [p for p in sig.parameters][1:] == ["A", "b", "x", "restart", "max_iter", "rel_tol", "check_every", "precond"]
    assert (sig.parameters["restart"].default, sig.parameters["max_iter"].default, sig.parameters["rel_tol"].default) == (30, 1000, 1e-8)
    import importlib

    tops = importlib.import_module("arm_spmv_amd.torch_ops")
    solve = inspect.signature(tops.SparseOperator.solve)
    assert "method" in solve.parameters and solve.parameters["method"].default == "bicgstab"
