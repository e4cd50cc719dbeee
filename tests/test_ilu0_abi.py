"""CPU-side checks of ILU(0) (spmv_ilu0_*; SPMV_PRECOND_ILU0): the library exports the four entry points, their argument checks run
before any device use, and the Python bindings have the methods."""
import ctypes as C

import pytest

FUNCTIONS = ("spmv_ilu0_setup", "spmv_ilu0_solve", "spmv_ilu0_factors", "spmv_ilu0_order")


@pytest.mark.parametrize("name", FUNCTIONS)
def test_library_exports_the_entry_point(pkg, name):
    lib = pkg.capi.load()
    assert hasattr(lib, name), f"libspmv_hip.so does not export {name}"
    assert name in pkg.capi.SIGNATURES


def test_null_arguments_are_refused_without_a_device(pkg):
    lib = pkg.capi.load()
    calls = {
        "spmv_ilu0_setup": lambda: lib.spmv_ilu0_setup(None, None),
        "spmv_ilu0_solve": lambda: lib.spmv_ilu0_solve(None, None, None, None),
        "spmv_ilu0_factors": lambda: lib.spmv_ilu0_factors(None, None, None),
        "spmv_ilu0_order": lambda: lib.spmv_ilu0_order(None, None, None),
    }
    for name in FUNCTIONS:
        assert calls[name]() == -1, name
        assert name.encode() in lib.spmv_last_error(), (name, lib.spmv_last_error())


def test_the_solvers_know_the_preconditioner_value_before_any_device_use(pkg):
    """3 is a known value now: what refuses the call is the null argument, as for the other values; 7 stays unknown wherever the
    value is looked at (tests/test_gpu_ilu0.py checks that with real handles)"""
    lib, capi = pkg.capi.load(), pkg.capi
    assert (capi.PRECOND_NONE, capi.PRECOND_JACOBI, capi.PRECOND_SYMGS, capi.PRECOND_ILU0) == (0, 1, 2, 3)
    iters, res = C.c_int32(0), C.c_double(0.0)
    assert lib.spmv_cg(None, None, None, None, 10, 1e-8, 1, capi.PRECOND_ILU0, C.byref(iters), C.byref(res)) == -1
    assert b"spmv_cg" in lib.spmv_last_error()
    assert lib.spmv_bicgstab(None, None, None, None, 10, 1e-8, 1, capi.PRECOND_ILU0, C.byref(iters), C.byref(res)) == -1
    assert b"spmv_bicgstab" in lib.spmv_last_error()


def test_context_has_the_methods(pkg):
    import inspect

    for name in ("ilu0_setup", "ilu0_solve", "ilu0_factors", "ilu0_order"):
        assert callable(getattr(pkg.capi.Context, name, None)), name
    assert "precond" in inspect.signature(pkg.capi.Context.cg).parameters
    assert list(inspect.signature(pkg.capi.Context.cg).parameters)[-1] == "precond"  # trailing: the positional arguments keep their places
