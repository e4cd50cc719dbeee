"""CPU-side checks of aggregation AMG (spmv_amg_*; SPMV_PRECOND_AMG): the library exports the entry points, the header and the
ctypes table agree, and every refusal that is made before the device is touched - return code and the message, which names the
entry - on host structs with addresses that are never dereferenced, in the manner of tests/test_chebyshev_abi.py."""
import ctypes as C
import inspect
import math
import re
from pathlib import Path

import pytest

FUNCTIONS = ("spmv_amg_setup", "spmv_amg_info", "spmv_amg_level", "spmv_amg_solve")
INVALID, UNSUPPORTED = -1, -5
COO, CSR, ELL = 0, 1, 3
AMG = 5


class _Vec(C.Structure):  # struct spmv_vec's leading fields (csrc/common.hpp): ctx, n, d, owned
    _fields_ = [("ctx", C.c_void_p), ("n", C.c_int64), ("d", C.c_void_p), ("owned", C.c_bool)]


class _Mat(C.Structure):  # struct spmv_mat's leading fields: ctx, format, nrow, ncol, k, nnz, row_begin, a, b, v
    _fields_ = [("ctx", C.c_void_p), ("format", C.c_int32), ("nrow", C.c_int32), ("ncol", C.c_int32), ("k", C.c_int32),
                ("nnz", C.c_int64), ("row_begin", C.c_int64), ("a", C.c_void_p), ("b", C.c_void_p), ("v", C.c_void_p)]


def _mat(fmt=CSR, nrow=7, ncol=7, k=0, nnz=12, row_begin=0, arrays=True):
    return _Mat(ctx=None, format=fmt, nrow=nrow, ncol=ncol, k=k, nnz=nnz, row_begin=row_begin, a=16, b=16 if arrays else 0, v=16 if arrays else 0)


SQUARE, TALL, GONE, ELL7, SHARD = _mat(), _mat(ncol=5), _mat(arrays=False), _mat(fmt=ELL, k=2), _mat(row_begin=3)
R_AT, Z_AT = 0x10000, 0x20000  # never dereferenced
_CTX = C.c_int64(0)            # any non-null context: the checks fail before it is used


def _handle_refusals(who):
    return [
        ("not CSR", ELL7, UNSUPPORTED, f"{who}: AMG needs a CSR handle (format 3)"),
        ("not square", TALL, INVALID, f"{who}: AMG needs the whole square matrix (7 x 5, first row 0)"),
        ("a shard", SHARD, INVALID, f"{who}: AMG needs the whole square matrix (7 x 7, first row 3)"),
        ("arrays released", GONE, INVALID, f"{who}: the CSR arrays are gone (panel_keep_csr = 0 released them)"),
    ]


@pytest.mark.parametrize("name", FUNCTIONS + ("SPMV_PRECOND_AMG",))
def test_library_exports_the_entry_points_and_the_header_names_them(pkg, name):
    header = (Path(__file__).resolve().parent.parent / "include" / "spmv_abi.h").read_text()
    assert re.search(r"\b" + name + r"\b", header), f"include/spmv_abi.h does not name {name}"
    if name.startswith("spmv_"):
        lib = pkg.capi.load()
        assert hasattr(lib, name), f"libspmv_hip.so does not export {name}"
        assert name in pkg.capi.SIGNATURES


def test_header_and_ctypes_table_agree(pkg):
    header = (Path(__file__).resolve().parent.parent / "include" / "spmv_abi.h").read_text()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"SPMV_PRECOND_AMG\s*=\s*5\b", header) and pkg.capi.PRECOND_AMG == 5 == AMG
    for name, nargs in zip(FUNCTIONS, (7, 4, 7, 4)):
        assert len(pkg.capi.SIGNATURES[name][1]) == nargs, name
        decl = re.search(name + r"\s*\((.*?)\);", body, re.S).group(1)
        assert decl.count(",") + 1 == nargs, name


def test_null_arguments_are_refused_without_a_device(pkg):
    lib = pkg.capi.load()
    calls = {
        "spmv_amg_setup": lambda: lib.spmv_amg_setup(None, None, 0, 0, 0, 0.0, 0.0),
        "spmv_amg_info": lambda: lib.spmv_amg_info(None, None, None, None),
        "spmv_amg_level": lambda: lib.spmv_amg_level(None, None, 0, None, None, None, None),
        "spmv_amg_solve": lambda: lib.spmv_amg_solve(None, None, None, None),
    }
    for name, call in calls.items():
        assert call() == INVALID, name
        assert lib.spmv_last_error().decode() == f"{name}: null argument"


def test_setup_refusals_without_a_device(pkg):
    lib = pkg.capi.load()
    who = "spmv_amg_setup"

    def call(M=SQUARE, max_levels=0, coarse_max=0, smooth_degree=0, strength=0.0, overcorrection=0.0):
        return lib.spmv_amg_setup(C.byref(_CTX), C.byref(M), max_levels, coarse_max, smooth_degree, strength, overcorrection), lib.spmv_last_error().decode()

    cases = [
        ("max_levels -1", call(max_levels=-1), INVALID, f"{who}: max_levels=-1, must be 1 .. 32 (0: 16)"),
        ("max_levels 33", call(max_levels=33), INVALID, f"{who}: max_levels=33, must be 1 .. 32 (0: 16)"),
        ("coarse_max -1", call(coarse_max=-1), INVALID, f"{who}: coarse_max=-1, must be 1 .. 1024 (0: 256)"),
        ("coarse_max 1025", call(coarse_max=1025), INVALID, f"{who}: coarse_max=1025, must be 1 .. 1024 (0: 256)"),
        ("smooth_degree -1", call(smooth_degree=-1), INVALID, f"{who}: smooth_degree=-1, must be 1 .. 64 (0: 2)"),
        ("smooth_degree 65", call(smooth_degree=65), INVALID, f"{who}: smooth_degree=65, must be 1 .. 64 (0: 2)"),
        ("strength nan", call(strength=math.nan), INVALID, f"{who}: strength=nan, must be finite (<= 0: every stored entry)"),
        ("overcorrection 2", call(overcorrection=2.0), INVALID, f"{who}: overcorrection=2, must be inside (0, 2) (0: 1.5)"),
        ("overcorrection -0.5", call(overcorrection=-0.5), INVALID, f"{who}: overcorrection=-0.5, must be inside (0, 2) (0: 1.5)"),
        ("overcorrection nan", call(overcorrection=math.nan), INVALID, f"{who}: overcorrection=nan, must be inside (0, 2) (0: 1.5)"),
    ] + [(what, call(M=M), code, message) for what, M, code, message in _handle_refusals(who)]
    for what, (rc, err), code, message in cases:
        assert (rc, err) == (code, message), what


def test_solve_level_and_info_refusals_without_a_device(pkg):
    lib = pkg.capi.load()
    who = "spmv_amg_solve"

    def solve(M=SQUARE, r=(7, R_AT), z=(7, Z_AT)):
        rv, zv = _Vec(n=r[0], d=r[1]), _Vec(n=z[0], d=z[1])
        return lib.spmv_amg_solve(C.byref(_CTX), C.byref(M), C.byref(rv), C.byref(zv)), lib.spmv_last_error().decode()

    cases = [(what, solve(M=M), code, message) for what, M, code, message in _handle_refusals(who)] + [
        ("length", solve(r=(6, R_AT)), INVALID, f"{who}: r has 6 and z 7 entries, the matrix 7 rows"),
        ("length", solve(z=(8, Z_AT)), INVALID, f"{who}: r has 7 and z 8 entries, the matrix 7 rows"),
        ("overlap", solve(z=(7, R_AT + 8 * 3)), INVALID, f"{who}: r and z must not overlap"),
        ("the same address", solve(z=(7, R_AT)), INVALID, f"{who}: r and z must not overlap"),
    ]
    for what, (rc, err), code, message in cases:
        assert (rc, err) == (code, message), what
    # a handle that was not set up: the whole struct, as the library lays it out, with the state's pointer null
    whole = (C.c_char * 8192)()
    C.memmove(whole, C.byref(SQUARE), C.sizeof(SQUARE))
    rv, zv = _Vec(n=7, d=R_AT), _Vec(n=7, d=Z_AT)
    assert lib.spmv_amg_solve(C.byref(_CTX), whole, C.byref(rv), C.byref(zv)) == INVALID
    assert lib.spmv_last_error().decode() == "spmv_amg_solve: the handle was not set up (spmv_amg_setup)"
    levels = C.c_int32(0)
    assert lib.spmv_amg_info(whole, C.byref(levels), None, None) == INVALID
    assert lib.spmv_last_error().decode() == "spmv_amg_info: the handle was not set up (spmv_amg_setup)"
    assert lib.spmv_amg_level(C.byref(_CTX), whole, 0, None, None, None, None) == INVALID
    assert lib.spmv_last_error().decode() == "spmv_amg_level: the handle was not set up (spmv_amg_setup)"
    for what, M, code, message in _handle_refusals("spmv_amg_level"):
        assert (lib.spmv_amg_level(C.byref(_CTX), C.byref(M), 0, None, None, None, None), lib.spmv_last_error().decode()) == (code, message), what


@pytest.mark.parametrize("name, extra", [("spmv_cg", ()), ("spmv_bicgstab", ()), ("spmv_gmres", (30,))])
def test_the_solvers_take_the_preconditioner_and_refuse_on_the_host(pkg, name, extra):
    """5 is a known value: what refuses these calls is the handle - before any device use, on structs that hold the leading fields"""
    lib = pkg.capi.load()
    iters, res = C.c_int32(0), C.c_double(0.0)

    def call(M):
        bv, xv = _Vec(n=7, d=R_AT), _Vec(n=7, d=Z_AT)
        rc = getattr(lib, name)(C.byref(_CTX), C.byref(M), C.byref(bv), C.byref(xv), *extra, 10, 1e-8, 1, AMG, C.byref(iters), C.byref(res))
        return rc, lib.spmv_last_error().decode()

    for what, M, code, message in _handle_refusals(name):
        if what == "not square":
            continue  # (the solver's own check comes first, with its own words)
        assert call(M) == (code, message), what


def test_cg_multi_refuses_the_preconditioner(pkg):
    lib = pkg.capi.load()
    iters, res = (C.c_int32 * 4)(), (C.c_double * 4)()
    for M in (SQUARE, ELL7, SHARD):
        bv, xv = _Vec(n=21, d=R_AT), _Vec(n=21, d=Z_AT)
        rc = lib.spmv_cg_multi(C.byref(_CTX), C.byref(M), 3, C.byref(bv), C.byref(xv), 10, 1e-8, 1, AMG, iters, res)
        assert (rc, lib.spmv_last_error().decode()) == (UNSUPPORTED, "spmv_cg_multi: the AMG preconditioner is not built for k columns")


def test_context_has_the_methods(pkg):
    for name in ("amg_setup", "amg_info", "amg_level", "amg_solve"):
        assert callable(getattr(pkg.capi.Context, name, None)), name
    sig = inspect.signature(pkg.capi.Context.amg_setup)
    assert [p for p in sig.parameters][1:] == ["A", "max_levels", "coarse_max", "smooth_degree", "strength", "overcorrection"]
    assert [sig.parameters[p].default for p in list(sig.parameters)[2:]] == [0, 0, 0, 0.0, 0.0]
