"""CPU-side checks of the multi-vector product Y += A*X (spmv_apply_multi): the library exports it, its argument checks run
before any device use, and the Python binding has the methods."""
import ctypes as C


def test_library_exports_the_multi_vector_product(pkg):
    lib = pkg.capi.load()
    for name in ("spmv_apply_multi", "spmv_apply_multi_timed"):
        assert hasattr(lib, name), f"libspmv_hip.so does not export {name}"
        assert name in pkg.capi.SIGNATURES


def test_null_arguments_are_refused_without_a_device(pkg):
    lib = pkg.capi.load()
    assert lib.spmv_apply_multi(None, None, 8, None, None, 0) == -1
    assert b"spmv_apply_multi" in lib.spmv_last_error()
    ms = C.c_double(0.0)
    assert lib.spmv_apply_multi_timed(None, None, 8, None, None, 0, 1, C.byref(ms)) == -1
    assert b"spmv_apply_multi" in lib.spmv_last_error()


def test_context_has_the_multi_vector_methods(pkg):
    Context = pkg.capi.Context
    assert callable(getattr(Context, "apply_multi", None))
    assert callable(getattr(Context, "apply_multi_timed", None))
