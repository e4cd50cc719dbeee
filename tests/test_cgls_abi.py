"""CPU-side checks of the least-squares solver (spmv_cgls): the library exports it, its argument checks run before any device use,
and the Python bindings have the methods."""
import ctypes as C


def test_library_exports_the_least_squares_solver(pkg):
    lib = pkg.capi.load()
    assert hasattr(lib, "spmv_cgls"), "libspmv_hip.so does not export spmv_cgls"
    assert "spmv_cgls" in pkg.capi.SIGNATURES


def test_null_arguments_are_refused_without_a_device(pkg):
    lib = pkg.capi.load()
    iters, nres, res = C.c_int32(0), C.c_double(0.0), C.c_double(0.0)
    assert lib.spmv_cgls(None, None, None, None, 10, 1e-8, 1, 0.0, C.byref(iters), C.byref(nres), C.byref(res)) == -1
    assert b"spmv_cgls" in lib.spmv_last_error()
    assert lib.spmv_cgls(None, None, None, None, 10, 1e-8, 1, 0.0, None, None, None) == -1
    assert b"spmv_cgls" in lib.spmv_last_error()


def test_context_and_operator_have_the_least_squares_solver(pkg):
    assert callable(getattr(pkg.capi.Context, "cgls", None))
    import importlib

    tops = importlib.import_module("arm_spmv_amd.torch_ops")
    assert callable(getattr(tops.SparseOperator, "lstsq", None))
