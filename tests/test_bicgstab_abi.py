"""CPU-side checks of the nonsymmetric solver (spmv_bicgstab): the library exports it, its argument checks run before any device
use, and the Python bindings have the methods."""
import ctypes as C


def test_library_exports_the_nonsymmetric_solver(pkg):
    lib = pkg.capi.load()
    assert hasattr(lib, "spmv_bicgstab"), "libspmv_hip.so does not export spmv_bicgstab"
    assert "spmv_bicgstab" in pkg.capi.SIGNATURES


def test_null_arguments_are_refused_without_a_device(pkg):
    lib = pkg.capi.load()
    iters, res = C.c_int32(0), C.c_double(0.0)
    assert lib.spmv_bicgstab(None, None, None, None, 10, 1e-8, 1, 0, C.byref(iters), C.byref(res)) == -1
    assert b"spmv_bicgstab" in lib.spmv_last_error()
    assert lib.spmv_bicgstab(None, None, None, None, 10, 1e-8, 1, 1, None, None) == -1
    assert b"spmv_bicgstab" in lib.spmv_last_error()


def test_context_and_operator_have_the_nonsymmetric_solver(pkg):
    assert callable(getattr(pkg.capi.Context, "bicgstab", None))
    import importlib

    tops = importlib.import_module("arm_spmv_amd.torch_ops")
    assert callable(getattr(tops.SparseOperator, "solve", None))
