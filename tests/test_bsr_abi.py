"""CPU-side checks of the block CSR entry points (spmv_bsr_upload, spmv_bsr_wrap_device, spmv_csr_to_bsr, spmv_bsr_to_csr) and of
what a BSR handle is refused: every refusal is made before any device use - on host structs with addresses that are never
dereferenced - and names the function."""
import ctypes as C
import inspect
import struct

import numpy as np

ARITY = {"spmv_bsr_upload": 8, "spmv_bsr_wrap_device": 8, "spmv_csr_to_bsr": 4, "spmv_bsr_to_csr": 4}
INVALID, UNSUPPORTED = -1, -5


class _Vec(C.Structure):  # struct spmv_vec's leading fields (csrc/common.hpp): ctx, n, d, owned
    _fields_ = [("ctx", C.c_void_p), ("n", C.c_int64), ("d", C.c_void_p), ("owned", C.c_bool)]


class _Mat(C.Structure):  # struct spmv_mat's leading fields: ctx, format, nrow, ncol, k, nnz, row_begin, a, b, v
    _fields_ = [("ctx", C.c_void_p), ("format", C.c_int32), ("nrow", C.c_int32), ("ncol", C.c_int32), ("k", C.c_int32),
                ("nnz", C.c_int64), ("row_begin", C.c_int64), ("a", C.c_void_p), ("b", C.c_void_p), ("v", C.c_void_p)]


def _handles(capi):
    ctx, other = C.c_int64(0), C.c_int64(0)
    here, there = C.addressof(ctx), C.addressof(other)
    csr = lambda **kw: _Mat(**{**dict(ctx=here, format=capi.FMT_CSR, nrow=30, ncol=30, k=0, nnz=90, row_begin=0, a=16, b=16, v=16), **kw})
    bsr = lambda **kw: _Mat(**{**dict(ctx=here, format=capi.FMT_BSR, nrow=30, ncol=30, k=3, nnz=20 * 9, row_begin=0, a=16, b=16, v=16), **kw})
    return ctx, here, there, csr, bsr


def _refused(cases, who):
    for what, ((rc, err), code, needle) in cases.items():
        assert rc == code and who in err and needle in err, (what, rc, err)


def test_library_header_and_bindings_have_the_entry_points(pkg):
    from pathlib import Path

    capi = pkg.capi
    lib = capi.load()
    text = (Path(__file__).resolve().parent.parent / "include" / "spmv_abi.h").read_text()
    for name, n in ARITY.items():
        assert hasattr(lib, name), f"libspmv_hip.so does not export {name}"
        assert name in capi.SIGNATURES and len(capi.SIGNATURES[name][1]) == n, name
        assert f"int {name}(" in text, name
    assert capi.FMT_BSR == 5 and "SPMV_FMT_BSR = 5" in text
    for name in ("bsr", "wrap_bsr", "csr_to_bsr", "bsr_to_csr"):
        assert callable(getattr(capi.Context, name, None)), name
    assert [p for p in inspect.signature(capi.Context.bsr).parameters][1:] == ["nrow", "ncol", "bs", "brow_ptr", "bcol", "val"]
    assert [p for p in inspect.signature(capi.Context.csr_to_bsr).parameters][1:] == ["A", "bs"]
    assert inspect.signature(capi.Context.bsr_to_csr).parameters["drop_zeros"].default is True


def test_upload_and_wrap_refusals_without_a_device(pkg):
    lib = pkg.capi.load()
    ctx = C.c_int64(0)
    ptr = np.zeros(11, dtype=np.int32).ctypes.data_as(C.c_void_p)
    out = C.c_void_p()
    for name in ("spmv_bsr_upload", "spmv_bsr_wrap_device"):
        fn = getattr(lib, name)

        def call(c=C.byref(ctx), nrow=30, ncol=30, bs=3, p=ptr, o=C.byref(out)):
            return fn(c, nrow, ncol, bs, p, None, None, o), lib.spmv_last_error()

        cases = {"null ctx": (call(c=None), INVALID, b"null"), "null pointer": (call(p=None), INVALID, b"null"), "null out": (call(o=None), INVALID, b"null"),
                 "nrow < 0": (call(nrow=-1), INVALID, b"bad size -1 x 30"), "ncol < 0": (call(ncol=-5), INVALID, b"bad size 30 x -5")}
        for bs in (0, 1, 9, -1):
            cases[f"bs = {bs}"] = (call(bs=bs), UNSUPPORTED, f"bs = {bs}".encode())
        _refused(cases, name.encode())
        assert out.value is None


def test_conversion_refusals_without_a_device(pkg):
    capi = pkg.capi
    lib = capi.load()
    ctx, here, there, csr, bsr = _handles(capi)
    out = C.c_void_p()

    def to_bsr(c=C.byref(ctx), M=csr(), bs=3, o=C.byref(out)):
        return lib.spmv_csr_to_bsr(c, C.byref(M) if M is not None else None, bs, o), lib.spmv_last_error()

    cases = {"null ctx": (to_bsr(c=None), INVALID, b"null"), "null A": (to_bsr(M=None), INVALID, b"null"), "null out": (to_bsr(o=None), INVALID, b"null"),
             "an ELL handle": (to_bsr(M=csr(format=capi.FMT_ELL, k=3)), UNSUPPORTED, b"CSR handle (format 3)"),
             "a BSR handle": (to_bsr(M=bsr()), UNSUPPORTED, b"CSR handle (format 5)"),
             "a shard": (to_bsr(M=csr(row_begin=30)), INVALID, b"shard"),
             "arrays released": (to_bsr(M=csr(b=0, v=0)), INVALID, b"are gone"),
             "another context": (to_bsr(M=csr(ctx=there)), INVALID, b"another context")}
    for bs in (0, 1, 9, -1):
        cases[f"bs = {bs}"] = (to_bsr(bs=bs), UNSUPPORTED, f"bs = {bs}".encode())
    _refused(cases, b"spmv_csr_to_bsr")

    def to_csr(c=C.byref(ctx), M=bsr(), o=C.byref(out)):
        return lib.spmv_bsr_to_csr(c, C.byref(M) if M is not None else None, 1, o), lib.spmv_last_error()

    _refused({"null ctx": (to_csr(c=None), INVALID, b"null"), "null A": (to_csr(M=None), INVALID, b"null"), "null out": (to_csr(o=None), INVALID, b"null"),
              "a CSR handle": (to_csr(M=csr()), UNSUPPORTED, b"BSR handle (format 1)"),
              "a DIA handle": (to_csr(M=csr(format=capi.FMT_DIA, k=3)), UNSUPPORTED, b"BSR handle (format 4)"),
              "another context": (to_csr(M=bsr(ctx=there)), INVALID, b"another context")}, b"spmv_bsr_to_csr")
    assert out.value is None


def test_what_a_bsr_handle_is_refused_without_a_device(pkg):
    capi = pkg.capi
    lib = capi.load()
    ctx, here, there, csr, bsr = _handles(capi)
    A, out = bsr(), C.c_void_p()
    X, Y = _Vec(ctx=here, n=60, d=0x10000), _Vec(ctx=here, n=60, d=0x20000)
    rc = lib.spmv_apply_multi(C.byref(ctx), C.byref(A), 2, C.byref(X), C.byref(Y), 0)
    assert rc == UNSUPPORTED and b"spmv_apply_multi" in lib.spmv_last_error() and b"format 5" in lib.spmv_last_error()
    rc = lib.spmv_ilu0_setup(C.byref(ctx), C.byref(A))
    assert rc == UNSUPPORTED and b"spmv_ilu0_setup" in lib.spmv_last_error() and b"CSR handle (format 5)" in lib.spmv_last_error()
    rc = lib.spmv_spgemm(C.byref(ctx), C.byref(A), C.byref(A), 0, C.byref(out))
    assert rc == UNSUPPORTED and b"spmv_spgemm" in lib.spmv_last_error() and b"format 5" in lib.spmv_last_error()
    B = csr()
    rc = lib.spmv_spgemm(C.byref(ctx), C.byref(B), C.byref(A), 0, C.byref(out))
    assert rc == UNSUPPORTED and b"B format 5" in lib.spmv_last_error()
    rc = lib.spmv_perm_rcm(C.byref(ctx), C.byref(A), C.byref(out))
    assert rc == UNSUPPORTED and b"spmv_perm_rcm" in lib.spmv_last_error() and b"CSR handle" in lib.spmv_last_error()
    assert out.value is None
    bounds = np.zeros(5, dtype=np.int64)
    rc = lib.spmv_mat_partition_rows(C.byref(A), 4, 1, bounds.ctypes.data)
    assert rc == UNSUPPORTED and b"spmv_mat_partition_rows" in lib.spmv_last_error() and b"BSR" in lib.spmv_last_error()
    assert lib.spmv_mat_partition_rows(C.byref(A), 3, 0, bounds.ctypes.data) == 0 and list(bounds[:4]) == [0, 10, 20, 30]  # equal rows: plain arithmetic


def _plan(fmt, kernel=1, lanes=36):
    node = [0] * 32
    node[0], node[1], node[2] = fmt, kernel, lanes
    node[20] = node[21] = node[22] = -1  # no children
    return struct.pack("<4I", 0x4E4C5053, 1, 16 + 128, 1) + struct.pack("<32i", *node)


def test_plan_check_takes_a_format_5_node_and_no_format_6(pkg):
    capi = pkg.capi
    lib = capi.load()
    fmt, kernel, nodes = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    blob = _plan(capi.FMT_BSR)
    assert lib.spmv_plan_check(blob, len(blob), C.byref(fmt), C.byref(kernel), C.byref(nodes)) == 0, lib.spmv_last_error()
    assert (fmt.value, kernel.value, nodes.value) == (5, 1, 1)
    blob = _plan(6)
    assert lib.spmv_plan_check(blob, len(blob), C.byref(fmt), C.byref(kernel), C.byref(nodes)) == INVALID and b"format 6" in lib.spmv_last_error()
    blob = _plan(capi.FMT_CSR, lanes=36)  # 36 lanes per row are a BSR node's alone
    assert lib.spmv_plan_check(blob, len(blob), C.byref(fmt), C.byref(kernel), C.byref(nodes)) == INVALID and b"36 lanes" in lib.spmv_last_error()
