"""CPU-side checks of the triangular solves (spmv_trsv_*): the library exports them, their argument checks run before any device
use, the Python bindings have the methods and constants, and the no-scratch gate names the new kernels."""
import ctypes as C
import fnmatch
import inspect
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("spmv_trsv_setup", "spmv_trsv_solve", "spmv_trsv_solve_multi", "spmv_trsv_info")


def test_library_exports_the_triangular_solves(pkg):
    lib = pkg.capi.load()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), f"libspmv_hip.so does not export {name}"
        assert name in pkg.capi.SIGNATURES
    sig = pkg.capi.SIGNATURES
    assert sig["spmv_trsv_setup"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32])
    assert sig["spmv_trsv_solve"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p])
    assert sig["spmv_trsv_solve_multi"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p])
    restype, argtypes = sig["spmv_trsv_info"]
    assert restype is C.c_int and len(argtypes) == 6 and argtypes[1] is C.c_uint32
    header = (ROOT / "include" / "spmv_abi.h").read_text()
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint {name}\(", header), name
    for name, value in (("LOWER", 0), ("UPPER", 1), ("UNIT", 2), ("TRANSPOSE", 4)):
        assert getattr(pkg.capi, f"TRSV_{name}") == value
        assert re.search(rf"#define SPMV_TRSV_{name}\s+{value}u", header), name


def test_null_arguments_are_refused_without_a_device(pkg):
    lib = pkg.capi.load()
    calls = {
        "spmv_trsv_setup": lambda: lib.spmv_trsv_setup(None, None, 0),
        "spmv_trsv_solve": lambda: lib.spmv_trsv_solve(None, None, 0, None, None),
        "spmv_trsv_solve_multi": lambda: lib.spmv_trsv_solve_multi(None, None, 0, 4, None, None),
        "spmv_trsv_info": lambda: lib.spmv_trsv_info(None, 0, None, None, None, None),
    }
    for name, call in calls.items():
        assert call() == -1, name
        assert name.encode() in lib.spmv_last_error() and b"null" in lib.spmv_last_error(), (name, lib.spmv_last_error())


def test_context_has_the_methods(pkg):
    ctx = pkg.capi.Context
    for name, head in (("trsv_setup", ["self", "A", "flags"]), ("trsv_solve", ["self", "A", "b", "x", "flags"]),
                       ("trsv_solve_multi", ["self", "A", "B", "X", "k", "flags"]), ("trsv_info", ["self", "A", "flags"])):
        fn = getattr(ctx, name, None)
        assert callable(fn), name
        params = inspect.signature(fn).parameters
        assert list(params) == head and params["flags"].default == pkg.capi.TRSV_LOWER, (name, list(params))


def test_the_no_scratch_gate_names_the_new_kernels():
    """every __global__ kernel that csrc/sptrsv.hip defines matches a pattern of tools/hot_kernels.txt that names it (not the catch-all)"""
    source = (ROOT / "arm-spmv_amd" / "csrc" / "sptrsv.hip").read_text()
    kernels = re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", source)
    assert len(kernels) >= 2 and {"trsv_multi_level_kernel", "trsv_multi_run_kernel"} <= set(kernels), kernels
    patterns = [line.split("#")[0].strip() for line in (ROOT / "tools" / "hot_kernels.txt").read_text().splitlines()]
    patterns = [p for p in patterns if p.startswith("trsv_")]
    assert len(patterns) >= len(kernels), patterns
    for k in kernels:
        assert any(fnmatch.fnmatch(k, p) or fnmatch.fnmatch(k + "<16, true>", p) for p in patterns), (k, patterns)
