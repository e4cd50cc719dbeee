"""CPU-side checks of the k-column solver (spmv_cg_multi): the library exports it, its argument checks run before any device use,
and the Python binding has the method."""
import ctypes as C


def test_library_exports_the_multi_column_solver(pkg):
    lib = pkg.capi.load()
    assert hasattr(lib, "spmv_cg_multi"), "libspmv_hip.so does not export spmv_cg_multi"
    assert "spmv_cg_multi" in pkg.capi.SIGNATURES


def test_null_arguments_are_refused_without_a_device(pkg):
    lib = pkg.capi.load()
    iters, res = (C.c_int32 * 4)(), (C.c_double * 4)()
    assert lib.spmv_cg_multi(None, None, 4, None, None, 10, 1e-8, 1, 0, iters, res) == -1
    assert b"spmv_cg_multi" in lib.spmv_last_error()
    assert lib.spmv_cg_multi(None, None, 4, None, None, 10, 1e-8, 1, 0, None, None) == -1
    assert b"spmv_cg_multi" in lib.spmv_last_error()


def test_context_has_the_multi_column_solver(pkg):
    assert callable(getattr(pkg.capi.Context, "cg_multi", None))
