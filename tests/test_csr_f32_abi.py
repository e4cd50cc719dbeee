"""CPU-side checks of single-precision value storage (spmv_csr_to_f32, spmv_csr_f32_upload, spmv_f32_to_csr, spmv_f32_info), of
spmv_refine's argument checks and of what a format-6 handle is refused: every refusal is made before any device use - on host
structs with addresses that are never dereferenced - and names the function."""
import ctypes as C
import inspect
import struct
from pathlib import Path

import numpy as np

ARITY = {"spmv_csr_to_f32": 3, "spmv_csr_f32_upload": 7, "spmv_f32_to_csr": 3, "spmv_f32_info": 4, "spmv_refine": 14}
INVALID, UNSUPPORTED = -1, -5
HEADER = Path(__file__).resolve().parent.parent / "include" / "spmv_abi.h"


class _Vec(C.Structure):  # struct spmv_vec's leading fields (csrc/common.hpp): ctx, n, d, owned
    _fields_ = [("ctx", C.c_void_p), ("n", C.c_int64), ("d", C.c_void_p), ("owned", C.c_bool)]


class _Mat(C.Structure):  # struct spmv_mat's leading fields: ctx, format, nrow, ncol, k, nnz, row_begin, a, b, v
    _fields_ = [("ctx", C.c_void_p), ("format", C.c_int32), ("nrow", C.c_int32), ("ncol", C.c_int32), ("k", C.c_int32),
                ("nnz", C.c_int64), ("row_begin", C.c_int64), ("a", C.c_void_p), ("b", C.c_void_p), ("v", C.c_void_p)]


def _handles(capi):
    ctx, other = C.c_int64(0), C.c_int64(0)
    here, there = C.addressof(ctx), C.addressof(other)
    csr = lambda **kw: _Mat(**{**dict(ctx=here, format=capi.FMT_CSR, nrow=30, ncol=30, k=0, nnz=90, row_begin=0, a=16, b=16, v=16), **kw})
    f32 = lambda **kw: _Mat(**{**dict(ctx=here, format=capi.FMT_CSR_F32, nrow=30, ncol=30, k=0, nnz=90, row_begin=0, a=16, b=16, v=16), **kw})
    return ctx, here, there, csr, f32


def _refused(cases, who):
    for what, ((rc, err), code, needle) in cases.items():
        assert rc == code and who in err and needle in err, (what, rc, err)


def test_library_header_and_bindings_have_the_entry_points(pkg):
    capi = pkg.capi
    lib = capi.load()
    text = HEADER.read_text()
    for name, n in ARITY.items():
        assert hasattr(lib, name), f"libspmv_hip.so does not export {name}"
        assert name in capi.SIGNATURES and len(capi.SIGNATURES[name][1]) == n, name
        assert f"int {name}(" in text, name
    assert capi.FMT_CSR_F32 == 6 and "SPMV_FMT_CSR_F32 = 6" in text
    assert (capi.REFINE_CG, capi.REFINE_BICGSTAB) == (0, 1) and "SPMV_REFINE_CG       = 0" in text and "SPMV_REFINE_BICGSTAB = 1" in text
    assert lib.spmv_abi_version() == 1 and "#define SPMV_ABI_VERSION 1" in text
    assert "spmv_csr_f32_wrap_device" not in capi.SIGNATURES and not hasattr(lib, "spmv_csr_f32_wrap_device")
    assert "NO spmv_csr_f32_wrap_device" in text  # the header says why there is none
    for name in ("csr_f32", "csr_to_f32", "f32_to_csr", "refine"):
        assert callable(getattr(capi.Context, name, None)), name
    assert callable(getattr(capi.Matrix, "f32_info", None))
    assert [p for p in inspect.signature(capi.Context.csr_f32).parameters][1:] == ["nrow", "ncol", "row_ptr", "col", "val"]
    assert [p for p in inspect.signature(capi.Context.refine).parameters][1:5] == ["A", "A_lo", "b", "x"]


def test_upload_refusals_without_a_device(pkg):
    lib = pkg.capi.load()
    ctx = C.c_int64(0)
    ptr = np.zeros(31, dtype=np.int32).ctypes.data_as(C.c_void_p)
    out = C.c_void_p()

    def call(c=C.byref(ctx), nrow=30, ncol=30, p=ptr, o=C.byref(out)):
        return lib.spmv_csr_f32_upload(c, nrow, ncol, p, None, None, o), lib.spmv_last_error()

    _refused({"null ctx": (call(c=None), INVALID, b"null"), "null pointer": (call(p=None), INVALID, b"null"), "null out": (call(o=None), INVALID, b"null"),
              "nrow < 0": (call(nrow=-1), INVALID, b"bad size -1 x 30"), "ncol < 0": (call(ncol=-5), INVALID, b"bad size 30 x -5")}, b"spmv_csr_f32_upload")
    rp = np.arange(31, dtype=np.int32)  # 30 entries and no arrays for them
    assert lib.spmv_csr_f32_upload(C.byref(ctx), 30, 30, rp.ctypes.data_as(C.c_void_p), None, None, C.byref(out)) == INVALID
    assert b"spmv_csr_f32_upload" in lib.spmv_last_error() and b"nnz=30" in lib.spmv_last_error()
    assert out.value is None


def test_conversion_refusals_without_a_device(pkg):
    capi = pkg.capi
    lib = capi.load()
    ctx, here, there, csr, f32 = _handles(capi)
    out = C.c_void_p()

    def to_f32(c=C.byref(ctx), M=csr(), o=C.byref(out)):
        return lib.spmv_csr_to_f32(c, C.byref(M) if M is not None else None, o), lib.spmv_last_error()

    _refused({"null ctx": (to_f32(c=None), INVALID, b"null"), "null A": (to_f32(M=None), INVALID, b"null"), "null out": (to_f32(o=None), INVALID, b"null"),
              "an ELL handle": (to_f32(M=csr(format=capi.FMT_ELL, k=3)), UNSUPPORTED, b"CSR handle (format 3)"),
              "a BSR handle": (to_f32(M=csr(format=capi.FMT_BSR, k=3)), UNSUPPORTED, b"CSR handle (format 5)"),
              "a format-6 handle": (to_f32(M=f32()), UNSUPPORTED, b"CSR handle (format 6)"),
              "a shard": (to_f32(M=csr(row_begin=30)), INVALID, b"shard"),
              "arrays released": (to_f32(M=csr(b=0, v=0)), INVALID, b"are gone"),
              "another context": (to_f32(M=csr(ctx=there)), INVALID, b"another context")}, b"spmv_csr_to_f32")

    def to_csr(c=C.byref(ctx), M=f32(), o=C.byref(out)):
        return lib.spmv_f32_to_csr(c, C.byref(M) if M is not None else None, o), lib.spmv_last_error()

    _refused({"null ctx": (to_csr(c=None), INVALID, b"null"), "null A": (to_csr(M=None), INVALID, b"null"), "null out": (to_csr(o=None), INVALID, b"null"),
              "a CSR handle": (to_csr(M=csr()), UNSUPPORTED, b"format 6 (format 1)"),
              "a DIA handle": (to_csr(M=csr(format=capi.FMT_DIA, k=3)), UNSUPPORTED, b"format 6 (format 4)"),
              "another context": (to_csr(M=f32(ctx=there)), INVALID, b"another context")}, b"spmv_f32_to_csr")
    assert out.value is None
    a, b, r = C.c_int64(-1), C.c_int64(-1), C.c_double(-1.0)
    M = csr()
    assert lib.spmv_f32_info(None, C.byref(a), C.byref(b), C.byref(r)) == INVALID and b"spmv_f32_info" in lib.spmv_last_error()
    assert lib.spmv_f32_info(C.byref(M), C.byref(a), C.byref(b), C.byref(r)) == UNSUPPORTED and b"format 6 (format 1)" in lib.spmv_last_error()
    assert (a.value, b.value, r.value) == (-1, -1, -1.0)


def test_what_a_format_6_handle_is_refused_without_a_device(pkg):
    capi = pkg.capi
    lib = capi.load()
    ctx, here, there, csr, f32 = _handles(capi)
    A, out = f32(), C.c_void_p()
    err = lib.spmv_last_error
    X, Y = _Vec(ctx=here, n=60, d=0x10000), _Vec(ctx=here, n=60, d=0x20000)
    rc = lib.spmv_apply_multi(C.byref(ctx), C.byref(A), 2, C.byref(X), C.byref(Y), 0)
    assert rc == UNSUPPORTED and b"spmv_apply_multi" in err() and b"format 6" in err()
    it, res = np.zeros(2, np.int32), np.zeros(2)
    rc = lib.spmv_cg_multi(C.byref(ctx), C.byref(A), 2, C.byref(X), C.byref(Y), 10, 1e-8, 1, 0, it.ctypes.data_as(C.POINTER(C.c_int32)), res.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == UNSUPPORTED and b"spmv_cg_multi" in err() and b"format 6" in err()
    pa, pb, pv = C.c_void_p(), C.c_void_p(), C.c_void_p()
    rc = lib.spmv_mat_device_ptrs(C.byref(A), C.byref(pa), C.byref(pb), C.byref(pv))
    assert rc == UNSUPPORTED and b"spmv_mat_device_ptrs" in err() and b"format 6" in err() and pa.value is None
    for flags in (1, 2, 3, 0x80000000):
        rc = lib.spmv_mat_set_flags(C.byref(A), flags)
        assert rc == UNSUPPORTED and b"spmv_mat_set_flags" in err() and b"format 6" in err(), flags
    bounds = np.zeros(5, dtype=np.int64)
    rc = lib.spmv_mat_partition_rows(C.byref(A), 4, 1, bounds.ctypes.data)
    assert rc == UNSUPPORTED and b"spmv_mat_partition_rows" in err() and b"format 6" in err()
    assert lib.spmv_mat_partition_rows(C.byref(A), 3, 0, bounds.ctypes.data) == 0 and list(bounds[:4]) == [0, 10, 20, 30]  # equal rows: plain arithmetic
    n = C.c_int64(0)
    rc = lib.spmv_mat_get_plan(C.byref(A), None, C.byref(n))
    assert rc == UNSUPPORTED and b"spmv_mat_get_plan" in err() and b"format 6" in err()
    blob = _plan(capi.FMT_CSR, lanes=8)
    rc = lib.spmv_mat_set_plan(C.byref(A), blob, len(blob))
    assert rc == UNSUPPORTED and b"spmv_mat_set_plan" in err() and b"format 6" in err()
    # one kernel: every other kernel id and every lane count that is no power of two up to 64
    for kernel, lanes in ((2, 0), (3, 0), (4, 0), (5, 0), (6, 0), (7, 0), (8, 0), (1, 3), (1, 128), (0, 48), (1, -1)):
        rc = lib.spmv_mat_set_kernel(C.byref(A), kernel, lanes)
        assert rc == UNSUPPORTED and b"spmv_mat_set_kernel" in err() and b"format 6" in err(), (kernel, lanes)
    # the CSR-only entry points
    rc = lib.spmv_ilu0_setup(C.byref(ctx), C.byref(A))
    assert rc == UNSUPPORTED and b"spmv_ilu0_setup" in err() and b"CSR handle (format 6)" in err()
    rc = lib.spmv_amg_setup(C.byref(ctx), C.byref(A), 0, 0, 0, 0.0, 0.0)
    assert rc == UNSUPPORTED and b"spmv_amg_setup" in err()
    rc = lib.spmv_fsai_setup(C.byref(ctx), C.byref(A), 0)
    assert rc == UNSUPPORTED and b"spmv_fsai_setup" in err()
    rc = lib.spmv_spgemm(C.byref(ctx), C.byref(A), C.byref(A), 0, C.byref(out))
    assert rc == UNSUPPORTED and b"spmv_spgemm" in err() and b"format 6" in err()
    rc = lib.spmv_csr_transpose(C.byref(ctx), C.byref(A), C.byref(out))
    assert rc == UNSUPPORTED and b"spmv_csr_transpose" in err() and b"format 6" in err()
    rc = lib.spmv_perm_rcm(C.byref(ctx), C.byref(A), C.byref(out))
    assert rc == UNSUPPORTED and b"spmv_perm_rcm" in err() and b"CSR handle" in err()
    rc = lib.spmv_csr_to_bsr(C.byref(ctx), C.byref(A), 3, C.byref(out))
    assert rc == UNSUPPORTED and b"CSR handle (format 6)" in err()
    assert out.value is None
    b, x = _Vec(ctx=here, n=30, d=0x10000), _Vec(ctx=here, n=30, d=0x20000)
    iters, rres = C.c_int32(0), C.c_double(0.0)
    for name in ("spmv_cg", "spmv_bicgstab"):
        rc = getattr(lib, name)(C.byref(ctx), C.byref(A), C.byref(b), C.byref(x), 10, 1e-8, 1, capi.PRECOND_JACOBI, C.byref(iters), C.byref(rres))
        assert rc == UNSUPPORTED and name.encode() in err() and b"Jacobi" in err(), name


def _plan(fmt, kernel=1, lanes=8):
    node = [0] * 32
    node[0], node[1], node[2] = fmt, kernel, lanes
    node[20] = node[21] = node[22] = -1  # no children
    return struct.pack("<4I", 0x4E4C5053, 1, 16 + 128, 1) + struct.pack("<32i", *node)


def test_plans_do_not_learn_the_format(pkg):
    capi = pkg.capi
    lib = capi.load()
    fmt, kernel, nodes = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    blob = _plan(6)
    assert lib.spmv_plan_check(blob, len(blob), C.byref(fmt), C.byref(kernel), C.byref(nodes)) == INVALID and b"format 6" in lib.spmv_last_error()
    assert (fmt.value, kernel.value, nodes.value) == (-1, -1, -1)
    blob = _plan(capi.FMT_BSR, lanes=36)
    assert lib.spmv_plan_check(blob, len(blob), C.byref(fmt), C.byref(kernel), C.byref(nodes)) == 0 and fmt.value == 5


def test_refine_refusals_without_a_device(pkg):
    capi = pkg.capi
    lib = capi.load()
    ctx, here, there, csr, f32 = _handles(capi)
    outer, inner, res = C.c_int32(-7), C.c_int32(-7), C.c_double(-7.0)

    def call(c=C.byref(ctx), A=csr(), L=f32(), b=_Vec(ctx=here, n=30, d=0x10000), x=_Vec(ctx=here, n=30, d=0x20000), solver=0, precond=0, max_outer=5,
             inner_max=100, inner_tol=1e-4, rel_tol=1e-12, o=C.byref(outer), i=C.byref(inner), r=C.byref(res)):
        ref = lambda s: C.byref(s) if s is not None else None
        return lib.spmv_refine(c, ref(A), ref(L), ref(b), ref(x), solver, precond, max_outer, inner_max, inner_tol, rel_tol, o, i, r), lib.spmv_last_error()

    cases = {"null ctx": (call(c=None), INVALID, b"null"), "null A": (call(A=None), INVALID, b"null"), "null A_lo": (call(L=None), INVALID, b"null"),
             "null b": (call(b=None), INVALID, b"null"), "null x": (call(x=None), INVALID, b"null"), "null outer": (call(o=None), INVALID, b"null"),
             "null inner": (call(i=None), INVALID, b"null"), "null resid": (call(r=None), INVALID, b"null"),
             "not square": (call(A=csr(ncol=31), L=f32(ncol=31)), INVALID, b"30 x 31, not square"),
             "A_lo of another shape": (call(L=f32(nrow=29, ncol=29)), INVALID, b"A_lo is 29 x 29, A is 30 x 30"),
             "A of another context": (call(A=csr(ctx=there)), INVALID, b"A belongs to another context"),
             "A_lo of another context": (call(L=f32(ctx=there)), INVALID, b"A_lo belongs to another context"),
             "b too short": (call(b=_Vec(ctx=here, n=29, d=0x10000)), INVALID, b"b has 29 and x 30 entries"),
             "x too long": (call(x=_Vec(ctx=here, n=31, d=0x20000)), INVALID, b"b has 30 and x 31 entries"),
             "b and x overlap": (call(x=_Vec(ctx=here, n=30, d=0x10000 + 8 * 29)), INVALID, b"must not overlap"),
             "b is x": (call(x=_Vec(ctx=here, n=30, d=0x10000)), INVALID, b"must not overlap"),
             "max_outer < 0": (call(max_outer=-1), INVALID, b"max_outer=-1"), "inner_max_iter < 0": (call(inner_max=-2), INVALID, b"inner_max_iter=-2"),
             "inner_tol < 0": (call(inner_tol=-1e-4), INVALID, b"inner_tol=-0.0001"), "rel_tol < 0": (call(rel_tol=-1.0), INVALID, b"rel_tol=-1"),
             "rel_tol NaN": (call(rel_tol=float("nan")), INVALID, b"rel_tol="),
             "solver 2": (call(solver=2), INVALID, b"unknown solver 2"), "solver -1": (call(solver=-1), INVALID, b"unknown solver -1"),
             "precond 99": (call(precond=99), INVALID, b"unknown preconditioner 99")}
    _refused(cases, b"spmv_refine")
    # the inner solver's own refusals are the call's: Jacobi reads a CSR handle's diagonal, ILU(0) factors one
    rc, err = call(precond=capi.PRECOND_JACOBI)
    assert rc == UNSUPPORTED and b"Jacobi" in err
    rc, err = call(solver=1, precond=capi.PRECOND_ILU0)
    assert rc == UNSUPPORTED and b"CSR handle (format 6)" in err
    assert (outer.value, inner.value, res.value) == (-7, -7, -7.0)  # nothing is written by a refused call
