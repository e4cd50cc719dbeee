"""CPU-side checks of smoothed-aggregation AMG (spmv_amg_setup_smoothed, spmv_amg_prolongator, spmv_amg_transfer_timed): the library
exports the entry points, the header and the ctypes table agree, and every refusal that is made before the device is touched - return
code and the message, which names the entry - on host structs with addresses that are never dereferenced, in the manner of
tests/test_amg_abi.py."""
import ctypes as C
import inspect
import math
import re
from pathlib import Path

import pytest

FUNCTIONS = ("spmv_amg_setup_smoothed", "spmv_amg_prolongator", "spmv_amg_transfer_timed")
NARGS = (8, 7, 8)
INVALID, UNSUPPORTED = -1, -5
CSR, ELL = 1, 3
HEADER = Path(__file__).resolve().parent.parent / "include" / "spmv_abi.h"


class _Vec(C.Structure):  # struct spmv_vec's leading fields (csrc/common.hpp): ctx, n, d, owned
    _fields_ = [("ctx", C.c_void_p), ("n", C.c_int64), ("d", C.c_void_p), ("owned", C.c_bool)]


class _Mat(C.Structure):  # struct spmv_mat's leading fields: ctx, format, nrow, ncol, k, nnz, row_begin, a, b, v
    _fields_ = [("ctx", C.c_void_p), ("format", C.c_int32), ("nrow", C.c_int32), ("ncol", C.c_int32), ("k", C.c_int32),
                ("nnz", C.c_int64), ("row_begin", C.c_int64), ("a", C.c_void_p), ("b", C.c_void_p), ("v", C.c_void_p)]


def _mat(fmt=CSR, nrow=7, ncol=7, k=0, nnz=12, row_begin=0, arrays=True):
    return _Mat(ctx=None, format=fmt, nrow=nrow, ncol=ncol, k=k, nnz=nnz, row_begin=row_begin, a=16, b=16 if arrays else 0, v=16 if arrays else 0)


SQUARE, TALL, GONE, ELL7, SHARD = _mat(), _mat(ncol=5), _mat(arrays=False), _mat(fmt=ELL, k=2), _mat(row_begin=3)
_CTX = C.c_int64(0)  # any non-null context: the checks fail before it is used


def _handle_refusals(who):
    return [
        ("not CSR", ELL7, UNSUPPORTED, f"{who}: AMG needs a CSR handle (format 3)"),
        ("not square", TALL, INVALID, f"{who}: AMG needs the whole square matrix (7 x 5, first row 0)"),
        ("a shard", SHARD, INVALID, f"{who}: AMG needs the whole square matrix (7 x 7, first row 3)"),
        ("arrays released", GONE, INVALID, f"{who}: the CSR arrays are gone (panel_keep_csr = 0 released them)"),
    ]


def _unset():
    """a handle that was not set up: the whole struct, as the library lays it out, with the state's pointer null"""
    whole = (C.c_char * 8192)()
    C.memmove(whole, C.byref(SQUARE), C.sizeof(SQUARE))
    return whole


@pytest.mark.parametrize("name", FUNCTIONS)
def test_library_exports_the_entry_points_and_the_header_names_them(pkg, name):
    assert re.search(r"\b" + name + r"\b", HEADER.read_text()), f"include/spmv_abi.h does not name {name}"
    lib = pkg.capi.load()
    assert hasattr(lib, name), f"libspmv_hip.so does not export {name}"
    assert name in pkg.capi.SIGNATURES


def test_header_and_ctypes_table_agree(pkg):
    header = HEADER.read_text()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, nargs in zip(FUNCTIONS, NARGS):
        assert len(pkg.capi.SIGNATURES[name][1]) == nargs, name
        decl = re.search(name + r"\s*\((.*?)\);", body, re.S).group(1)
        assert decl.count(",") + 1 == nargs, name
    for i, word in enumerate(("RESTRICT_FUSED", "RESTRICT_UNFUSED", "PROLONG_FUSED", "PROLONG_UNFUSED")):
        assert re.search(r"SPMV_AMG_" + word + r"\s*=\s*" + str(i) + r"\b", body) and getattr(pkg.capi, "AMG_" + word) == i
    # the header states the method and the defaults
    for words in ("prolong_damping / lam", "4/3 for prolong_damping", "1.0 for\n *   overcorrection", "spmv_csr_transpose(P)", "\"amg_smoothed\"",
                  "rounded once"):
        assert words in header, words


def test_null_arguments_are_refused_without_a_device(pkg):
    lib = pkg.capi.load()
    nnz, ms = C.c_int64(0), C.c_double(0.0)
    v = _Vec(n=7, d=0x10000)
    calls = {
        "spmv_amg_setup_smoothed": [lambda: lib.spmv_amg_setup_smoothed(None, None, 0, 0, 0, 0.0, 0.0, 0.0),
                                    lambda: lib.spmv_amg_setup_smoothed(C.byref(_CTX), None, 0, 0, 0, 0.0, 0.0, 0.0)],
        "spmv_amg_prolongator": [lambda: lib.spmv_amg_prolongator(None, None, 0, None, None, None, None),
                                 lambda: lib.spmv_amg_prolongator(C.byref(_CTX), C.byref(SQUARE), 0, None, None, None, None),
                                 lambda: lib.spmv_amg_prolongator(None, C.byref(SQUARE), 0, C.byref(nnz), None, None, None)],
        "spmv_amg_transfer_timed": [lambda: lib.spmv_amg_transfer_timed(None, None, 0, 0, 0, None, 1, None),
                                    lambda: lib.spmv_amg_transfer_timed(C.byref(_CTX), C.byref(SQUARE), 0, 0, 0, None, 1, C.byref(ms)),
                                    lambda: lib.spmv_amg_transfer_timed(C.byref(_CTX), C.byref(SQUARE), 0, 0, 0, C.byref(v), 1, None)],
    }
    for name, each in calls.items():
        for call in each:
            assert call() == INVALID, name
            assert lib.spmv_last_error().decode() == f"{name}: null argument"


def test_setup_refusals_without_a_device(pkg):
    lib = pkg.capi.load()
    who = "spmv_amg_setup_smoothed"

    def call(M=SQUARE, max_levels=0, coarse_max=0, smooth_degree=0, strength=0.0, overcorrection=0.0, prolong_damping=0.0):
        rc = lib.spmv_amg_setup_smoothed(C.byref(_CTX), C.byref(M), max_levels, coarse_max, smooth_degree, strength, overcorrection, prolong_damping)
        return rc, lib.spmv_last_error().decode()

    cases = [
        ("max_levels -1", call(max_levels=-1), INVALID, f"{who}: max_levels=-1, must be 1 .. 32 (0: 16)"),
        ("max_levels 33", call(max_levels=33), INVALID, f"{who}: max_levels=33, must be 1 .. 32 (0: 16)"),
        ("coarse_max -1", call(coarse_max=-1), INVALID, f"{who}: coarse_max=-1, must be 1 .. 1024 (0: 256)"),
        ("coarse_max 1025", call(coarse_max=1025), INVALID, f"{who}: coarse_max=1025, must be 1 .. 1024 (0: 256)"),
        ("smooth_degree -1", call(smooth_degree=-1), INVALID, f"{who}: smooth_degree=-1, must be 1 .. 64 (0: 2)"),
        ("smooth_degree 65", call(smooth_degree=65), INVALID, f"{who}: smooth_degree=65, must be 1 .. 64 (0: 2)"),
        ("strength nan", call(strength=math.nan), INVALID, f"{who}: strength=nan, must be finite (<= 0: every stored entry)"),
        ("overcorrection 2", call(overcorrection=2.0), INVALID, f"{who}: overcorrection=2, must be inside (0, 2) (0: 1)"),
        ("overcorrection -0.5", call(overcorrection=-0.5), INVALID, f"{who}: overcorrection=-0.5, must be inside (0, 2) (0: 1)"),
        ("overcorrection nan", call(overcorrection=math.nan), INVALID, f"{who}: overcorrection=nan, must be inside (0, 2) (0: 1)"),
        ("prolong_damping 2", call(prolong_damping=2.0), INVALID, f"{who}: prolong_damping=2, must be inside (0, 2) (0: 4/3)"),
        ("prolong_damping -1", call(prolong_damping=-1.0), INVALID, f"{who}: prolong_damping=-1, must be inside (0, 2) (0: 4/3)"),
        ("prolong_damping nan", call(prolong_damping=math.nan), INVALID, f"{who}: prolong_damping=nan, must be inside (0, 2) (0: 4/3)"),
        ("prolong_damping inf", call(prolong_damping=math.inf), INVALID, f"{who}: prolong_damping=inf, must be inside (0, 2) (0: 4/3)"),
    ] + [(what, call(M=M), code, message) for what, M, code, message in _handle_refusals(who)]
    for what, (rc, err), code, message in cases:
        assert (rc, err) == (code, message), what


def test_prolongator_and_transfer_refusals_without_a_device(pkg):
    lib = pkg.capi.load()
    nnz, ms = C.c_int64(0), C.c_double(0.0)
    v = _Vec(n=7, d=0x10000)
    for what, M, code, message in _handle_refusals("spmv_amg_prolongator"):
        assert (lib.spmv_amg_prolongator(C.byref(_CTX), C.byref(M), 0, C.byref(nnz), None, None, None), lib.spmv_last_error().decode()) == (code, message), what
    for what, M, code, message in _handle_refusals("spmv_amg_transfer_timed"):
        rc = lib.spmv_amg_transfer_timed(C.byref(_CTX), C.byref(M), 0, 0, 0, C.byref(v), 1, C.byref(ms))
        assert (rc, lib.spmv_last_error().decode()) == (code, message), what
    whole = _unset()
    assert lib.spmv_amg_prolongator(C.byref(_CTX), whole, 0, C.byref(nnz), None, None, None) == INVALID
    assert lib.spmv_last_error().decode() == "spmv_amg_prolongator: the handle was not set up (spmv_amg_setup_smoothed)"
    assert lib.spmv_amg_transfer_timed(C.byref(_CTX), whole, 0, 0, 0, C.byref(v), 1, C.byref(ms)) == INVALID
    assert lib.spmv_last_error().decode() == "spmv_amg_transfer_timed: the handle was not set up (spmv_amg_setup_smoothed)"
    assert lib.spmv_amg_transfer_timed(C.byref(_CTX), whole, 0, 0, 0, C.byref(v), 0, C.byref(ms)) == INVALID
    assert lib.spmv_last_error().decode() == "spmv_amg_transfer_timed: reps=0"


def test_context_has_the_methods(pkg):
    for name in ("amg_setup_smoothed", "amg_prolongator", "amg_transfer_timed"):
        assert callable(getattr(pkg.capi.Context, name, None)), name
    sig = inspect.signature(pkg.capi.Context.amg_setup_smoothed)
    assert [p for p in sig.parameters][1:] == ["A", "max_levels", "coarse_max", "smooth_degree", "strength", "overcorrection", "prolong_damping"]
    assert [sig.parameters[p].default for p in list(sig.parameters)[2:]] == [0, 0, 0, 0.0, 0.0, 0.0]
