"""CPU-side checks of the sparse products (spmv_spgemm, spmv_csr_transpose): the library exports the entry points, the header and the
ctypes table agree, and every refusal that is made before the device is touched - return code and the message, which names the
entry - on host structs with addresses that are never dereferenced, in the manner of tests/test_amg_abi.py."""
import ctypes as C
import inspect
import re
from pathlib import Path

import pytest

FUNCTIONS = ("spmv_spgemm", "spmv_csr_transpose")
INVALID, UNSUPPORTED = -1, -5
COO, CSR, ELL = 0, 1, 3


class _Mat(C.Structure):  # struct spmv_mat's leading fields: ctx, format, nrow, ncol, k, nnz, row_begin, a, b, v
    _fields_ = [("ctx", C.c_void_p), ("format", C.c_int32), ("nrow", C.c_int32), ("ncol", C.c_int32), ("k", C.c_int32),
                ("nnz", C.c_int64), ("row_begin", C.c_int64), ("a", C.c_void_p), ("b", C.c_void_p), ("v", C.c_void_p)]


_CTX, _OTHER = C.c_int64(0), C.c_int64(0)  # any two non-null contexts: the checks fail before one is used


def _mat(fmt=CSR, nrow=7, ncol=5, k=0, nnz=12, row_begin=0, arrays=True, ctx=_CTX):
    return _Mat(ctx=C.addressof(ctx), format=fmt, nrow=nrow, ncol=ncol, k=k, nnz=nnz, row_begin=row_begin, a=16, b=16 if arrays else 0,
                v=16 if arrays else 0)


A75, B59 = _mat(), _mat(nrow=5, ncol=9)


@pytest.mark.parametrize("name", FUNCTIONS + ("SPMV_SPGEMM_AUTO", "SPMV_SPGEMM_ROWS", "SPMV_SPGEMM_SORT"))
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
    for name, value in (("AUTO", 0), ("ROWS", 1), ("SORT", 2)):
        assert re.search(rf"SPMV_SPGEMM_{name}\s*=\s*{value}\b", header) and getattr(pkg.capi, f"SPGEMM_{name}") == value
    for name, nargs in zip(FUNCTIONS, (5, 3)):
        assert len(pkg.capi.SIGNATURES[name][1]) == nargs, name
        decl = re.search(name + r"\s*\((.*?)\);", body, re.S).group(1)
        assert decl.count(",") + 1 == nargs, name
    assert pkg.capi.load().spmv_abi_version() == 1


def test_null_arguments_are_refused_without_a_device(pkg):
    lib = pkg.capi.load()
    out = C.c_void_p(0)
    calls = {
        "spmv_spgemm": [lambda: lib.spmv_spgemm(None, C.byref(A75), C.byref(B59), 0, C.byref(out)),
                        lambda: lib.spmv_spgemm(C.byref(_CTX), None, C.byref(B59), 0, C.byref(out)),
                        lambda: lib.spmv_spgemm(C.byref(_CTX), C.byref(A75), None, 0, C.byref(out)),
                        lambda: lib.spmv_spgemm(C.byref(_CTX), C.byref(A75), C.byref(B59), 0, None)],
        "spmv_csr_transpose": [lambda: lib.spmv_csr_transpose(None, C.byref(A75), C.byref(out)),
                               lambda: lib.spmv_csr_transpose(C.byref(_CTX), None, C.byref(out)),
                               lambda: lib.spmv_csr_transpose(C.byref(_CTX), C.byref(A75), None)],
    }
    for name, each in calls.items():
        for call in each:
            assert call() == INVALID, name
            assert lib.spmv_last_error().decode() == f"{name}: null argument"
    assert out.value is None


def test_spgemm_refusals_without_a_device(pkg):
    lib = pkg.capi.load()
    who = "spmv_spgemm"
    out = C.c_void_p(0)

    def call(A=A75, B=B59, method=0):
        return lib.spmv_spgemm(C.byref(_CTX), C.byref(A), C.byref(B), method, C.byref(out)), lib.spmv_last_error().decode()

    gone = "the CSR arrays of {} are gone (panel_keep_csr = 0 released them)"
    cases = [
        ("A not CSR", call(A=_mat(fmt=ELL, k=2)), UNSUPPORTED, f"{who}: both matrices must be CSR handles (A has format 3, B format 1)"),
        ("B not CSR", call(B=_mat(fmt=COO, nrow=5, ncol=9)), UNSUPPORTED, f"{who}: both matrices must be CSR handles (A has format 1, B format 0)"),
        ("A a shard", call(A=_mat(row_begin=3)), INVALID, f"{who}: A must be the whole matrix, not a shard (first row 3)"),
        ("B a shard", call(B=_mat(nrow=5, ncol=9, row_begin=2)), INVALID, f"{who}: B must be the whole matrix, not a shard (first row 2)"),
        ("A released", call(A=_mat(arrays=False)), INVALID, f"{who}: " + gone.format("A")),
        ("B released", call(B=_mat(nrow=5, ncol=9, arrays=False)), INVALID, f"{who}: " + gone.format("B")),
        ("A of another context", call(A=_mat(ctx=_OTHER)), INVALID, f"{who}: A belongs to another context"),
        ("B of another context", call(B=_mat(nrow=5, ncol=9, ctx=_OTHER)), INVALID, f"{who}: B belongs to another context"),
        ("shapes", call(B=_mat(nrow=6, ncol=9)), INVALID, f"{who}: A is 7 x 5 and B is 6 x 9: the columns of A must be the rows of B"),
        ("method -1", call(method=-1), INVALID, f"{who}: method=-1, must be 0 (AUTO), 1 (ROWS) or 2 (SORT)"),
        ("method 3", call(method=3), INVALID, f"{who}: method=3, must be 0 (AUTO), 1 (ROWS) or 2 (SORT)"),
    ]
    for what, (rc, err), code, message in cases:
        assert (rc, err) == (code, message), what
    assert out.value is None, "a refusal leaves *out_C untouched"


def test_transpose_refusals_without_a_device(pkg):
    lib = pkg.capi.load()
    who = "spmv_csr_transpose"
    out = C.c_void_p(0)

    def call(A):
        return lib.spmv_csr_transpose(C.byref(_CTX), C.byref(A), C.byref(out)), lib.spmv_last_error().decode()

    cases = [
        ("not CSR", call(_mat(fmt=ELL, k=2)), UNSUPPORTED, f"{who}: A must be a CSR handle (format 3)"),
        ("a shard", call(_mat(row_begin=3)), INVALID, f"{who}: A must be the whole matrix, not a shard (first row 3)"),
        ("released", call(_mat(arrays=False)), INVALID, f"{who}: the CSR arrays of A are gone (panel_keep_csr = 0 released them)"),
        ("another context", call(_mat(ctx=_OTHER)), INVALID, f"{who}: A belongs to another context"),
    ]
    for what, (rc, err), code, message in cases:
        assert (rc, err) == (code, message), what
    assert out.value is None


def test_context_has_the_methods(pkg):
    sig = inspect.signature(pkg.capi.Context.spgemm)
    assert list(sig.parameters)[1:] == ["A", "B", "method"] and sig.parameters["method"].default == 0
    assert list(inspect.signature(pkg.capi.Context.csr_transpose).parameters)[1:] == ["A"]
