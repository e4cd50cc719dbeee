"""CPU-side checks of FSAI (spmv_fsai_*; SPMV_PRECOND_FSAI): the library exports the four entry points, their argument checks run
before any device use, the solvers know the new preconditioner value, and the Python bindings have the methods."""
import ctypes as C

import pytest

FUNCTIONS = ("spmv_fsai_setup", "spmv_fsai_solve", "spmv_fsai_info", "spmv_fsai_factor")


@pytest.mark.parametrize("name", FUNCTIONS)
def test_library_exports_the_entry_point(pkg, name):
    lib = pkg.capi.load()
    assert hasattr(lib, name), f"libspmv_hip.so does not export {name}"
    assert name in pkg.capi.SIGNATURES


def test_null_arguments_are_refused_without_a_device(pkg):
    lib = pkg.capi.load()
    calls = {
        "spmv_fsai_setup": lambda: lib.spmv_fsai_setup(None, None, 1),
        "spmv_fsai_solve": lambda: lib.spmv_fsai_solve(None, None, None, None),
        "spmv_fsai_info": lambda: lib.spmv_fsai_info(None, None, None, None),
        "spmv_fsai_factor": lambda: lib.spmv_fsai_factor(None, None, None, None, None, None),
    }
    for name in FUNCTIONS:
        assert calls[name]() == -1, name
        assert name.encode() in lib.spmv_last_error(), (name, lib.spmv_last_error())


def test_the_solvers_know_the_preconditioner_value_before_any_device_use(pkg):
    """6 is a known value now: what refuses the call is the null argument, as for the other values; 7 and 9 stay unknown wherever
    the value is looked at (tests/test_gpu_fsai.py checks that with real handles)"""
    lib, capi = pkg.capi.load(), pkg.capi
    assert capi.PRECOND_FSAI == 6 and capi.PRECOND_AMG == 5 and capi.FSAI_MAX_ROW == 64
    iters, res = C.c_int32(0), C.c_double(0.0)
    assert lib.spmv_cg(None, None, None, None, 10, 1e-8, 1, capi.PRECOND_FSAI, C.byref(iters), C.byref(res)) == -1
    assert b"spmv_cg" in lib.spmv_last_error() and b"null" in lib.spmv_last_error()
    assert lib.spmv_bicgstab(None, None, None, None, 10, 1e-8, 1, capi.PRECOND_FSAI, C.byref(iters), C.byref(res)) == -1
    assert b"spmv_bicgstab" in lib.spmv_last_error() and b"null" in lib.spmv_last_error()
    assert lib.spmv_gmres(None, None, None, None, 30, 10, 1e-8, 1, capi.PRECOND_FSAI, C.byref(iters), C.byref(res)) == -1
    assert b"spmv_gmres" in lib.spmv_last_error() and b"null" in lib.spmv_last_error()


def test_the_header_states_the_contract():
    from pathlib import Path

    text = (Path(__file__).resolve().parent.parent / "include" / "spmv_abi.h").read_text()
    assert "SPMV_PRECOND_FSAI = 6" in text and "#define SPMV_FSAI_MAX_ROW 64" in text
    for name in FUNCTIONS:
        assert f"int {name}(" in text, name


def test_context_has_the_methods(pkg):
    import inspect

    for name in ("fsai_setup", "fsai_solve", "fsai_info", "fsai_factor"):
        assert callable(getattr(pkg.capi.Context, name, None)), name
    assert list(inspect.signature(pkg.capi.Context.fsai_setup).parameters) == ["self", "A", "level"]
