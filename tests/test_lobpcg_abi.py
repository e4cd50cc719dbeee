"""CPU-side checks of the block operations and the eigensolver (spmv_block_gram, spmv_block_combine, spmv_lobpcg): the library exports
them, every argument check runs before any device use - on host structs with addresses that are never dereferenced - and the Python
bindings have the methods."""
import ctypes as C
import inspect

import numpy as np


def test_library_exports_the_three_entry_points(pkg):
    lib = pkg.capi.load()
    arity = {"spmv_block_gram": 9, "spmv_block_combine": 9, "spmv_lobpcg": 12}
    for name, n in arity.items():
        assert hasattr(lib, name), f"libspmv_hip.so does not export {name}"
        assert name in pkg.capi.SIGNATURES and len(pkg.capi.SIGNATURES[name][1]) == n, name


class _Vec(C.Structure):  # struct spmv_vec's leading fields (csrc/common.hpp): ctx, n, d, owned
    _fields_ = [("ctx", C.c_void_p), ("n", C.c_int64), ("d", C.c_void_p), ("owned", C.c_bool)]


class _Mat(C.Structure):  # struct spmv_mat's leading fields: ctx, format, nrow, ncol, k, nnz, row_begin, a, b, v
    _fields_ = [("ctx", C.c_void_p), ("format", C.c_int32), ("nrow", C.c_int32), ("ncol", C.c_int32), ("k", C.c_int32),
                ("nnz", C.c_int64), ("row_begin", C.c_int64), ("a", C.c_void_p), ("b", C.c_void_p), ("v", C.c_void_p)]


_F64P = C.POINTER(C.c_double)


def test_block_gram_refusals_without_a_device(pkg):
    lib = pkg.capi.load()
    ctx = C.c_int64(0)  # any non-null context: the checks fail before it is used
    G = np.zeros(96 * 96)
    g = G.ctypes.data_as(_F64P)
    U, V = _Vec(n=100 * 4, d=0x10000), _Vec(n=100 * 5, d=0x20000)

    def call(c=C.byref(ctx), n=100, p=4, u=C.byref(U), ldu=100, q=5, v=C.byref(V), ldv=100, out=g):
        return lib.spmv_block_gram(c, n, p, u, ldu, q, v, ldv, out), lib.spmv_last_error()

    cases = {
        "null ctx": (call(c=None), b"null"), "null U": (call(u=None), b"null"), "null V": (call(v=None), b"null"), "null G": (call(out=None), b"null"),
        "p = 0": (call(p=0), b"columns"), "p = 97": (call(p=97), b"columns"), "q = 0": (call(q=0), b"columns"), "q = 97": (call(q=97), b"columns"),
        "n < 0": (call(n=-1), b"rows"),
        "ldu < n": (call(ldu=99), b"at least n"), "ldv < n": (call(ldv=99), b"at least n"),
        "U short": (call(u=C.byref(_Vec(n=399, d=0x10000))), b"too short"), "V short": (call(v=C.byref(_Vec(n=499, d=0x20000))), b"too short"),
        "U short for its ld": (call(ldu=101), b"too short"),
    }
    for what, ((rc, err), needle) in cases.items():
        assert rc == -1 and b"spmv_block_gram" in err and needle in err, (what, rc, err)
    # the last column needs n entries, not ld: (p - 1) * ld + n
    exact = _Vec(n=3 * 137 + 100, d=0x10000)
    rc, err = call(n=0, u=C.byref(_Vec(n=0, d=0)), v=C.byref(_Vec(n=0, d=0)), ldu=0, ldv=0)
    assert rc == 0 and not G.any(), (rc, err)  # n = 0: zeros, nothing launched, no device
    assert call(u=C.byref(_Vec(n=exact.n - 1, d=0x10000)), ldu=137)[0] == -1


def test_block_combine_refusals_without_a_device(pkg):
    lib = pkg.capi.load()
    ctx = C.c_int64(0)
    Cm = np.zeros(96 * 96)
    c = Cm.ctypes.data_as(_F64P)
    S, O = _Vec(n=100 * 4, d=0x10000), _Vec(n=100 * 5, d=0x40000)

    def call(cx=C.byref(ctx), n=100, p=4, s=C.byref(S), lds=100, q=5, cm=c, o=C.byref(O), ldo=100):
        return lib.spmv_block_combine(cx, n, p, s, lds, q, cm, o, ldo), lib.spmv_last_error()

    def at(addr, entries):
        return C.byref(_Vec(n=entries, d=addr))

    cases = {
        "null ctx": (call(cx=None), b"null"), "null S": (call(s=None), b"null"), "null Out": (call(o=None), b"null"), "null C": (call(cm=None), b"null"),
        "p = 0": (call(p=0), b"columns"), "p = 97": (call(p=97), b"columns"), "q = 0": (call(q=0), b"columns"), "q = 97": (call(q=97), b"columns"),
        "n < 0": (call(n=-1), b"rows"),
        "lds < n": (call(lds=99), b"at least n"), "ldo < n": (call(ldo=99), b"at least n"),
        "S short": (call(s=at(0x10000, 399)), b"too short"), "Out short": (call(o=at(0x40000, 499)), b"too short"),
        "Out inside S": (call(o=at(0x10000 + 8 * 100, 500)), b"overlap"),
        "Out a row below S": (call(o=at(0x10000 + 8, 500)), b"overlap"),
        "S inside Out": (call(o=at(0x10000 - 8 * 200, 500)), b"overlap"),
        "same start, another ld": (call(s=at(0x10000, 4 * 120), lds=120, o=at(0x10000, 500)), b"overlap"),
    }
    for what, ((rc, err), needle) in cases.items():
        assert rc == -1 and b"spmv_block_combine" in err and needle in err, (what, rc, err)
    assert call(n=0, s=at(0, 0), o=at(0, 0), lds=0, ldo=0)[0] == 0  # n = 0: nothing to do, no device


def test_lobpcg_refusals_without_a_device(pkg):
    capi = pkg.capi
    lib = capi.load()
    ctx = C.c_int64(0)
    A = _Mat(ctx=None, format=capi.FMT_CSR, nrow=30, ncol=30, k=0, nnz=90, row_begin=0, a=16, b=16, v=16)
    R = _Mat(ctx=None, format=capi.FMT_CSR, nrow=30, ncol=20, k=0, nnz=90, row_begin=0, a=16, b=16, v=16)
    G = _Mat(ctx=None, format=capi.FMT_CSR, nrow=30, ncol=30, k=0, nnz=90, row_begin=0, a=16, b=0, v=0)
    L = _Mat(ctx=None, format=capi.FMT_ELL, nrow=30, ncol=30, k=3, nnz=90, row_begin=0, a=16, b=16, v=16)
    Z = _Mat(ctx=None, format=capi.FMT_CSR, nrow=0, ncol=0, k=0, nnz=0, row_begin=0, a=16, b=16, v=16)
    theta, resid = np.zeros(16), np.zeros(16)
    th, rs, iters = theta.ctypes.data_as(_F64P), resid.ctypes.data_as(_F64P), C.c_int32(7)

    def call(cx=C.byref(ctx), M=A, k=4, nev=4, x=None, max_iter=10, tol=1e-8, precond=0, t=th, r=rs, it=C.byref(iters), xn=None):
        xv = C.byref(_Vec(n=M.nrow * k if xn is None else xn, d=0x10000)) if x is None else x
        m = C.byref(M) if M is not None else None
        return lib.spmv_lobpcg(cx, m, k, nev, 0, xv, max_iter, tol, precond, t, r, it), lib.spmv_last_error()

    cases = {
        "null ctx": (call(cx=None), -1, b"null"), "null A": (call(M=None, xn=120), -1, b"null"), "null theta": (call(t=None), -1, b"null"),
        "null resid": (call(r=None), -1, b"null"), "null iters": (call(it=None), -1, b"null"),
        "not square": (call(M=R), -1, b"square"),
        "k = 0": (call(k=0, nev=0), -1, b"k = 0"), "k = 17": (call(k=17, nev=1), -1, b"k = 17"),
        "nev = 0": (call(nev=0), -1, b"nev"), "nev > k": (call(nev=5), -1, b"nev"),
        "n < 3 k": (call(k=11, nev=1), -1, b"3 k"),
        "X length": (call(xn=119), -1, b"entries"),
        "max_iter": (call(max_iter=-1), -1, b"max_iter"), "tol": (call(tol=-1e-8), -1, b"tol"), "tol nan": (call(tol=float("nan")), -1, b"tol"),
        "precond": (call(precond=7), -1, b"unknown preconditioner"),
        "symgs": (call(precond=capi.PRECOND_SYMGS), -5, b"Gauss-Seidel"),
        "jacobi on ell": (call(M=L, precond=capi.PRECOND_JACOBI), -5, b"Jacobi"),
        "jacobi, arrays released": (call(M=G, precond=capi.PRECOND_JACOBI), -1, b"gave up"),
        "ilu0 on ell": (call(M=L, precond=capi.PRECOND_ILU0), -5, b"ILU"),
        "amg on ell": (call(M=L, precond=capi.PRECOND_AMG), -5, b"AMG"),
    }
    for what, ((rc, err), code, needle) in cases.items():
        assert rc == code and b"spmv_lobpcg" in err and needle in err, (what, rc, err)
    assert lib.spmv_lobpcg(None, None, 4, 4, 0, None, 10, 1e-8, 0, None, None, None) == -1
    # an empty matrix returns at once with its outputs cleared: nothing is launched, no device is needed
    theta[:] = 5.0
    rc, err = call(M=Z, k=4, nev=2)
    assert rc == 0 and iters.value == 0 and not theta[:4].any(), (rc, err)


def test_context_has_the_methods(pkg):
    Ctx = pkg.capi.Context
    for name in ("block_gram", "block_combine", "lobpcg"):
        assert callable(getattr(Ctx, name, None)), name
    sig = inspect.signature(Ctx.lobpcg)
    assert [p for p in sig.parameters][1:] == ["A", "X", "k", "nev", "largest", "max_iter", "tol", "precond"]
    assert (sig.parameters["nev"].default, sig.parameters["largest"].default, sig.parameters["precond"].default) == (None, False, None)
    assert [p for p in inspect.signature(Ctx.block_gram).parameters][1:] == ["n", "p", "U", "ldu", "q", "V", "ldv"]
    assert [p for p in inspect.signature(Ctx.block_combine).parameters][1:] == ["n", "p", "S", "lds", "q", "Cm", "Out", "ldo"]
