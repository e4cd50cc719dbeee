"""CPU-side checks of the symmetric indefinite solver (spmv_minres): the library exports it, its argument checks run before any
device use, the Python bindings have the methods, and the no-scratch gate names its kernels."""
import ctypes as C
import fnmatch
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_library_exports_the_symmetric_indefinite_solver(pkg):
    lib = pkg.capi.load()
    assert hasattr(lib, "spmv_minres"), "libspmv_hip.so does not export spmv_minres"
    assert "spmv_minres" in pkg.capi.SIGNATURES
    restype, argtypes = pkg.capi.SIGNATURES["spmv_minres"]
    # ctx, A, P, b, x, shift, max_iter, rel_tol, check_every, precond, iters, rel_resid
    assert restype is C.c_int and len(argtypes) == 12 and argtypes[5] is C.c_double and argtypes[7] is C.c_double


def test_null_arguments_are_refused_without_a_device(pkg):
    lib = pkg.capi.load()
    iters, res = C.c_int32(0), C.c_double(0.0)
    assert lib.spmv_minres(None, None, None, None, None, 0.0, 10, 1e-8, 1, 0, C.byref(iters), C.byref(res)) == -1
    assert b"spmv_minres" in lib.spmv_last_error() and b"null" in lib.spmv_last_error()
    assert lib.spmv_minres(None, None, None, None, None, 0.5, 10, 1e-8, 1, 1, None, None) == -1
    assert b"spmv_minres" in lib.spmv_last_error()


def test_context_and_operator_have_the_symmetric_indefinite_solver(pkg):
    import importlib
    import inspect

    minres = getattr(pkg.capi.Context, "minres", None)
    assert callable(minres)
    params = inspect.signature(minres).parameters
    assert list(params)[:4] == ["self", "A", "b", "x"]
    assert {k: params[k].default for k in ("shift", "P", "max_iter", "rel_tol", "check_every", "precond")} == {
        "shift": 0.0, "P": None, "max_iter": 1000, "rel_tol": 1e-8, "check_every": 1, "precond": 0}
    tops = importlib.import_module("arm_spmv_amd.torch_ops")
    solve = getattr(tops.SparseOperator, "solve_symmetric", None)
    assert callable(solve)
    params = inspect.signature(solve).parameters
    assert params["x0"].default is None and params["shift"].default == 0.0 and params["M"].default is None


def test_the_no_scratch_gate_names_the_new_kernels():
    """every __global__ kernel of csrc/solver_minres.hip matches a pattern of tools/hot_kernels.txt that names it (not the catch-all)"""
    kernels = re.findall(r"__global__[^;{]*?void\s+(minres_\w+)\s*\(", (ROOT / "arm-spmv_amd" / "csrc" / "solver_minres.hip").read_text())
    assert len(kernels) >= 5, kernels
    patterns = [line.split("#")[0].strip() for line in (ROOT / "tools" / "hot_kernels.txt").read_text().splitlines()]
    patterns = [p for p in patterns if p.startswith("minres_")]
    vector = [k for k in kernels if k != "minres_dinv_sign_kernel"]  # (the set-up's sign check is no hot kernel: the catch-all covers it)
    for k in vector:
        assert any(fnmatch.fnmatch(k, p) or fnmatch.fnmatch(k + "<true>", p) for p in patterns), (k, patterns)
