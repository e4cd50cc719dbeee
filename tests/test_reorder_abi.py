"""CPU-side checks of the reordering entry points (spmv_perm_*, spmv_csr_permute, spmv_vec_permute, spmv_csr_bandwidth): the library
exports them, every refusal is made before any device use - on host structs with addresses that are never dereferenced - empty
problems return without a device, and the Python bindings have the methods."""
import ctypes as C
import inspect

import numpy as np

ARITY = {"spmv_perm_create": 4, "spmv_perm_rcm": 3, "spmv_perm_download": 3, "spmv_perm_info": 3, "spmv_perm_destroy": 1, "spmv_csr_permute": 5,
         "spmv_vec_permute": 5, "spmv_csr_bandwidth": 4}


def test_library_exports_the_entry_points(pkg):
    lib = pkg.capi.load()
    for name, n in ARITY.items():
        assert hasattr(lib, name), f"libspmv_hip.so does not export {name}"
        assert name in pkg.capi.SIGNATURES and len(pkg.capi.SIGNATURES[name][1]) == n, name
    assert lib.spmv_abi_version() == 1


def test_the_header_declares_them(pkg):
    from pathlib import Path

    text = (Path(__file__).resolve().parent.parent / "include" / "spmv_abi.h").read_text()
    for name in ARITY:
        assert f"int {name}(" in text, name
    assert "typedef struct spmv_perm spmv_perm;" in text


class _Vec(C.Structure):  # struct spmv_vec's leading fields (csrc/common.hpp): ctx, n, d, owned
    _fields_ = [("ctx", C.c_void_p), ("n", C.c_int64), ("d", C.c_void_p), ("owned", C.c_bool)]


class _Mat(C.Structure):  # struct spmv_mat's leading fields: ctx, format, nrow, ncol, k, nnz, row_begin, a, b, v
    _fields_ = [("ctx", C.c_void_p), ("format", C.c_int32), ("nrow", C.c_int32), ("ncol", C.c_int32), ("k", C.c_int32),
                ("nnz", C.c_int64), ("row_begin", C.c_int64), ("a", C.c_void_p), ("b", C.c_void_p), ("v", C.c_void_p)]


class _Perm(C.Structure):  # struct spmv_perm's leading fields (csrc/reorder.hip): ctx, n, order, inverse
    _fields_ = [("ctx", C.c_void_p), ("n", C.c_int64), ("order", C.c_void_p), ("inverse", C.c_void_p)]


def _handles(capi):
    ctx, other = C.c_int64(0), C.c_int64(0)
    here, there = C.addressof(ctx), C.addressof(other)
    mat = lambda **kw: _Mat(**{**dict(ctx=here, format=capi.FMT_CSR, nrow=30, ncol=30, k=0, nnz=90, row_begin=0, a=16, b=16, v=16), **kw})
    return ctx, other, here, there, mat


def _refused(cases, who):
    for what, ((rc, err), code, needle) in cases.items():
        assert rc == code and who in err and needle in err, (what, rc, err)


def test_perm_create_refusals_and_the_empty_permutation(pkg):
    lib = pkg.capi.load()
    ctx = C.c_int64(0)
    order = np.arange(4, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    out = C.c_void_p()

    def call(c=C.byref(ctx), n=4, o=order, p=C.byref(out)):
        return lib.spmv_perm_create(c, n, o, p), lib.spmv_last_error()

    _refused({"null ctx": (call(c=None), -1, b"null"), "null order": (call(o=None), -1, b"null"), "null out": (call(p=None), -1, b"null"),
              "n < 0": (call(n=-1), -1, b"n=-1"), "n beyond int32": (call(n=2**31), -1, b"n=2147483648")}, b"spmv_perm_create")
    rc, err = call(n=0, o=None)  # n = 0: a valid permutation, no device
    assert rc == 0 and out.value, (rc, err)
    n = C.c_int64(7)
    assert lib.spmv_perm_info(out, b"n", C.byref(n)) == 0 and n.value == 0
    for name in (b"rcm_isolated", b"rcm_components", b"rcm_levels", b"rcm_bfs", b"rcm_launches", b"rcm_transient_bytes"):
        n.value = 7
        assert lib.spmv_perm_info(out, name, C.byref(n)) == 0 and n.value == 0, name
    assert lib.spmv_perm_info(out, b"rcm_nothing", C.byref(n)) == -1 and b"unknown name" in lib.spmv_last_error()
    assert lib.spmv_perm_info(None, b"n", C.byref(n)) == -1 and lib.spmv_perm_info(out, None, C.byref(n)) == -1 and lib.spmv_perm_info(out, b"n", None) == -1
    assert lib.spmv_perm_download(out, None, None) == 0 and lib.spmv_perm_download(None, None, None) == -1
    assert lib.spmv_perm_destroy(out) == 0 and lib.spmv_perm_destroy(None) == 0


def test_perm_rcm_refusals_without_a_device(pkg):
    capi = pkg.capi
    lib = capi.load()
    ctx, other, here, there, mat = _handles(capi)
    out = C.c_void_p()

    def call(c=C.byref(ctx), M=mat(), p=C.byref(out)):
        return lib.spmv_perm_rcm(c, C.byref(M) if M is not None else None, p), lib.spmv_last_error()

    _refused({
        "null ctx": (call(c=None), -1, b"null"), "null A": (call(M=None), -1, b"null"), "null out": (call(p=None), -1, b"null"),
        "not CSR": (call(M=mat(format=capi.FMT_ELL, k=3)), -5, b"CSR handle"),
        "a shard": (call(M=mat(row_begin=30)), -1, b"shard"),
        "arrays released": (call(M=mat(b=0, v=0)), -1, b"are gone"),
        "another context": (call(M=mat(ctx=there)), -1, b"another context"),
        "not square": (call(M=mat(ncol=20)), -1, b"not square"),
    }, b"spmv_perm_rcm")
    assert out.value is None
    rc, err = call(M=mat(nrow=0, ncol=0, nnz=0))  # an empty matrix: the empty permutation, no device
    assert rc == 0 and out.value, (rc, err)
    assert lib.spmv_perm_destroy(out) == 0


def test_csr_permute_refusals_without_a_device(pkg):
    capi = pkg.capi
    lib = capi.load()
    ctx, other, here, there, mat = _handles(capi)
    out = C.c_void_p()
    rows, cols = _Perm(ctx=here, n=30, order=16, inverse=16), _Perm(ctx=here, n=20, order=16, inverse=16)
    R = mat(ncol=20)

    def call(c=C.byref(ctx), M=R, r=C.byref(rows), cl=C.byref(cols), p=C.byref(out)):
        return lib.spmv_csr_permute(c, C.byref(M) if M is not None else None, r, cl, p), lib.spmv_last_error()

    _refused({
        "null ctx": (call(c=None), -1, b"null"), "null A": (call(M=None), -1, b"null"), "null out": (call(p=None), -1, b"null"),
        "not CSR": (call(M=mat(format=capi.FMT_COO, ncol=20)), -5, b"CSR handle"),
        "a shard": (call(M=mat(ncol=20, row_begin=7)), -1, b"shard"),
        "arrays released": (call(M=mat(ncol=20, b=0, v=0)), -1, b"are gone"),
        "another context": (call(M=mat(ncol=20, ctx=there)), -1, b"another context"),
        "rows of another size": (call(r=C.byref(cols)), -1, b"20 entries, A has 30 rows"),
        "columns of another size": (call(cl=C.byref(rows)), -1, b"30 entries, A has 20 columns"),
        "rows of another context": (call(r=C.byref(_Perm(ctx=there, n=30, order=16, inverse=16))), -1, b"rows belongs to another context"),
        "columns of another context": (call(cl=C.byref(_Perm(ctx=there, n=20, order=16, inverse=16))), -1, b"columns belongs to another context"),
    }, b"spmv_csr_permute")
    assert out.value is None


def test_vec_permute_refusals_without_a_device(pkg):
    lib = pkg.capi.load()
    ctx, other = C.c_int64(0), C.c_int64(0)
    here, there = C.addressof(ctx), C.addressof(other)
    P = _Perm(ctx=here, n=100, order=16, inverse=16)
    at = lambda addr, n=100: C.byref(_Vec(ctx=here, n=n, d=addr))

    def call(c=C.byref(ctx), p=C.byref(P), back=0, s=at(0x10000), d=at(0x20000)):
        return lib.spmv_vec_permute(c, p, back, s, d), lib.spmv_last_error()

    _refused({
        "null ctx": (call(c=None), -1, b"null"), "null perm": (call(p=None), -1, b"null"), "null src": (call(s=None), -1, b"null"), "null dst": (call(d=None), -1, b"null"),
        "back = 2": (call(back=2), -1, b"back=2"), "back = -1": (call(back=-1), -1, b"back=-1"),
        "another context": (call(p=C.byref(_Perm(ctx=there, n=100, order=16, inverse=16))), -1, b"permutation belongs to another context"),
        "src of another context": (call(s=C.byref(_Vec(ctx=there, n=100, d=0x10000))), -1, b"src belongs to another context"),
        "dst of another context": (call(d=C.byref(_Vec(ctx=there, n=100, d=0x20000))), -1, b"dst belongs to another context"),
        "src short": (call(s=at(0x10000, 99)), -1, b"src has 99"), "dst long": (call(d=at(0x20000, 101)), -1, b"dst 101"),
        "the same vector": (call(d=at(0x10000)), -1, b"overlap"),
        "dst inside src": (call(d=at(0x10000 + 8 * 99)), -1, b"overlap"), "src inside dst": (call(d=at(0x10000 - 8 * 99)), -1, b"overlap"),
    }, b"spmv_vec_permute")
    empty = _Perm(ctx=here, n=0, order=0, inverse=0)
    for back in (0, 1):
        rc, err = call(p=C.byref(empty), back=back, s=at(0, 0), d=at(0, 0))  # n = 0: nothing to do, no device
        assert rc == 0, (rc, err)


def test_csr_bandwidth_refusals_without_a_device(pkg):
    capi = pkg.capi
    lib = capi.load()
    ctx, other, here, there, mat = _handles(capi)
    bw, prof = C.c_int64(5), C.c_int64(5)

    def call(c=C.byref(ctx), M=mat(), b=C.byref(bw), p=C.byref(prof)):
        return lib.spmv_csr_bandwidth(c, C.byref(M) if M is not None else None, b, p), lib.spmv_last_error()

    _refused({
        "null ctx": (call(c=None), -1, b"null"), "null A": (call(M=None), -1, b"null"), "null bandwidth": (call(b=None), -1, b"null"),
        "null profile": (call(p=None), -1, b"null"),
        "not CSR": (call(M=mat(format=capi.FMT_DIA, k=3)), -5, b"CSR handle"), "a shard": (call(M=mat(row_begin=1)), -1, b"shard"),
        "arrays released": (call(M=mat(b=0, v=0)), -1, b"are gone"), "another context": (call(M=mat(ctx=there)), -1, b"another context"),
    }, b"spmv_csr_bandwidth")
    assert (bw.value, prof.value) == (5, 5)
    for M in (mat(nrow=0, ncol=0, nnz=0), mat(nnz=0)):  # no rows, or no entries: zeros, no device
        bw.value = prof.value = 5
        rc, err = call(M=M)
        assert rc == 0 and (bw.value, prof.value) == (0, 0), (rc, err)


def test_python_has_the_methods(pkg):
    Ctx, Perm = pkg.capi.Context, pkg.capi.Perm
    for name in ("perm", "perm_rcm", "csr_permute", "vec_permute", "csr_bandwidth"):
        assert callable(getattr(Ctx, name, None)), name
    assert [p for p in inspect.signature(Ctx.csr_permute).parameters][1:] == ["A", "rows", "cols"]
    assert [p for p in inspect.signature(Ctx.vec_permute).parameters][1:] == ["p", "src", "dst", "back"]
    assert inspect.signature(Ctx.vec_permute).parameters["back"].default is False
    for name in ("download", "info"):
        assert callable(getattr(Perm, name, None)), name


def test_the_twin_reads_the_repeat_limit_from_the_settings_header():
    import rcm_ref

    assert rcm_ref.root_repeats() == 8


def test_the_lane_rule_and_the_constants_of_the_settings_header(tmp_path):
    import shutil
    import subprocess
    from pathlib import Path

    import pytest

    if not shutil.which("g++"):
        pytest.skip("no g++ here")
    root = Path(__file__).resolve().parent.parent
    exe = tmp_path / "reorder_settings_check"
    subprocess.run(["g++", "-O2", "-std=c++17", f"-I{root / 'arm-spmv_amd' / 'csrc'}", str(root / "tests" / "reorder_settings_check.cpp"), "-o", str(exe)],
                   check=True, timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and " 0 violations" in r.stdout, r.stdout + r.stderr
