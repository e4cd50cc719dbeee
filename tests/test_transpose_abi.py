"""CPU-side checks of the transposed product y += A^T x (spmv_apply_transpose): the library exports it, its argument checks run
before any device use, the Python binding has the methods, and the sharded reduction of dist.py (reduce_transposed) over gloo adds
the ranks' contributions in rank order - with the oracle as the per-shard product, since the engine needs a GPU."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

NAMES = ("spmv_apply_transpose", "spmv_apply_transpose_timed", "spmv_mat_transpose_setup")


def test_library_exports_the_transposed_product(pkg):
    lib = pkg.capi.load()
    for name in NAMES:
        assert hasattr(lib, name), f"libspmv_hip.so does not export {name}"
        assert name in pkg.capi.SIGNATURES


def test_null_arguments_are_refused_without_a_device(pkg):
    lib = pkg.capi.load()
    assert lib.spmv_apply_transpose(None, None, None, None) == -1
    assert b"spmv_apply_transpose" in lib.spmv_last_error()
    ms = C.c_double(0.0)
    assert lib.spmv_apply_transpose_timed(None, None, None, None, 1, C.byref(ms)) == -1
    assert b"spmv_apply_transpose_timed" in lib.spmv_last_error()
    assert lib.spmv_mat_transpose_setup(None) == -1
    assert b"spmv_mat_transpose_setup" in lib.spmv_last_error()


class _Vec(C.Structure):  # struct spmv_vec's leading fields (csrc/common.hpp): ctx, n, d, owned
    _fields_ = [("ctx", C.c_void_p), ("n", C.c_int64), ("d", C.c_void_p), ("owned", C.c_bool)]


class _Mat(C.Structure):  # struct spmv_mat's leading fields: ctx, format, nrow, ncol, k, nnz, row_begin, a, b, v
    _fields_ = [("ctx", C.c_void_p), ("format", C.c_int32), ("nrow", C.c_int32), ("ncol", C.c_int32), ("k", C.c_int32),
                ("nnz", C.c_int64), ("row_begin", C.c_int64), ("a", C.c_void_p), ("b", C.c_void_p), ("v", C.c_void_p)]


def _mat(fmt, nrow, ncol, nnz, b=1, v=1):
    return _Mat(ctx=None, format=fmt, nrow=nrow, ncol=ncol, k=0, nnz=nnz, row_begin=0, a=16, b=b, v=v)


def test_size_errors_are_refused_without_a_device(pkg):
    """lengths, overlap and released CSR arrays: the checks read only host-side fields, so they hold on a machine without a GPU
    (the handles here are host structs with fake device addresses that are never dereferenced)"""
    capi = pkg.capi
    lib = capi.load()
    ctx = C.c_int64(0)  # any non-null context: the checks fail before it is used
    A = _mat(capi.FMT_CSR, 7, 5, 12)
    x, y = _Vec(n=7, d=0x10000), _Vec(n=5, d=0x20000)
    cases = {
        "x length": (_Vec(n=5, d=0x10000), y, A, b"x has 5 entries"),
        "y length": (x, _Vec(n=7, d=0x20000), A, b"y has 7 entries"),
        "overlap": (x, _Vec(n=5, d=0x10000 + 8 * 6), A, b"overlap"),
        "released": (x, y, _mat(capi.FMT_CSR, 7, 5, 12, b=0, v=0), b"panel_keep_csr"),
    }
    ms = C.c_double(0.0)
    for what, (xv, yv, M, needle) in cases.items():
        assert lib.spmv_apply_transpose(C.byref(ctx), C.byref(M), C.byref(xv), C.byref(yv)) == -1, what
        err = lib.spmv_last_error()
        assert b"spmv_apply_transpose" in err and needle in err, (what, err)
        assert lib.spmv_apply_transpose_timed(C.byref(ctx), C.byref(M), C.byref(xv), C.byref(yv), 1, C.byref(ms)) == -1, what
        assert b"spmv_apply_transpose_timed" in lib.spmv_last_error()
    # a released CSR handle has no transposed state to build either
    R = _mat(capi.FMT_CSR, 7, 5, 12, b=0, v=0)
    assert lib.spmv_mat_transpose_setup(C.byref(R)) == -1
    assert b"panel_keep_csr" in lib.spmv_last_error()


def test_context_and_matrix_have_the_transposed_methods(pkg):
    capi = pkg.capi
    assert callable(getattr(capi.Context, "apply_transpose", None))
    assert callable(getattr(capi.Context, "apply_transpose_timed", None))
    assert callable(getattr(capi.Matrix, "transpose_setup", None))


def test_torch_operator_module_imports(pkg):
    import importlib

    tops = importlib.import_module("arm_spmv_amd.torch_ops")
    assert callable(tops.spmv) and callable(getattr(tops.SparseOperator, "rmatvec", None))
    assert callable(getattr(importlib.import_module("arm_spmv_amd.dist").HipShardOps, "product_transpose", None))


# ---- dist.reduce_transposed over gloo ----------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, nrow, ncol, row_bounds, col_bounds, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import importlib
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    sys.path[:0] = [str(root), str(root / "tests")]
    from __graft_entry__ import load_package

    pkg = load_package()
    dmod = importlib.import_module("arm_spmv_amd.dist")
    import oracle_lib as ol

    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        orc = ol.load_oracle()
        rp, col, val = pkg.synth.csr_uniform(0, nrow, ncol, 9, seed=31)
        x = pkg.synth.vec_uniform(nrow, seed=32)
        y0 = pkg.synth.vec_uniform(ncol, seed=33)
        # every rank's shard contribution over all columns: the CSC product of its CSR arrays, from zeros
        partials = []
        for b, e in row_bounds:
            srp = ol.csr_shard_row_ptr(orc, rp, b, e)
            part = np.zeros(ncol)
            ol.csc_spmv(orc, srp, np.ascontiguousarray(col[rp[b]:rp[e]]), np.ascontiguousarray(val[rp[b]:rp[e]]),
                        np.ascontiguousarray(x[b:e]), part)
            partials.append(part)
        cb, ce = (col_bounds or dmod.all_bounds(ncol, world))[rank]
        y_own = torch.from_numpy(y0[cb:ce].copy())
        dmod.reduce_transposed(torch.from_numpy(partials[rank]), y_own, ncol, bounds=col_bounds)
        expect = y0[cb:ce].copy()
        for p in range(world):  # rank order
            expect += partials[p][cb:ce]
        whole = y0.copy()
        ol.csc_spmv(orc, rp, col, val, x, whole)  # the unsharded transposed product
        scale = np.zeros(ncol)
        trp, tcol, tval = ol.coo_to_csr(orc, ncol, np.ascontiguousarray(col), np.repeat(np.arange(nrow, dtype=np.int32), np.diff(rp)), val)
        ol.csr_abs_row_sums(orc, trp, tcol, tval, x, scale)
        scale += np.abs(y0)
        try:
            ol.assert_parity(y_own.numpy(), whole[cb:ce], scale[cb:ce], "reduced against unsharded")
            parity = True
        except AssertionError:
            parity = False
        q.put((rank, bool(np.array_equal(y_own.numpy(), expect)), parity))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,nrow,ncol,ragged", [(2, 1000, 777, False), (2, 1001, 1300, True), (3, 1000, 1000, False),
                                                      (3, 997, 611, True)])
def test_reduce_transposed_over_gloo(world, nrow, ncol, ragged):
    row_bounds = [(0, 101), (101, nrow)] if world == 2 else [(0, 400), (400, 401), (401, nrow)]
    if not ragged:
        rb = [(int(nrow * r // world), int(nrow * (r + 1) // world)) for r in range(world)]
        row_bounds = rb
    col_bounds = None
    if ragged:
        col_bounds = [(0, 17), (17, ncol)] if world == 2 else [(0, 0), (0, ncol - 5), (ncol - 5, ncol)]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, nrow, ncol, row_bounds, col_bounds, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=180) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(r[0] for r in results) == list(range(world))
    assert all(r[1] for r in results), "reduced y differs from y0 + the partials added in rank order"
    assert all(r[2] for r in results), "reduced y is outside the parity gate of the unsharded transposed product"


def _bad_bounds_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import importlib
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    sys.path[:0] = [str(root), str(root / "tests")]
    from __graft_entry__ import load_package

    load_package()
    dmod = importlib.import_module("arm_spmv_amd.dist")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        msgs = []
        for bounds, n_part, n_own in (([(0, 3), (4, 10)], 10, 3), (None, 9, 5), (None, 10, 4)):
            try:
                dmod.reduce_transposed(torch.zeros(n_part, dtype=torch.float64), torch.zeros(n_own, dtype=torch.float64), 10, bounds=bounds)
                msgs.append(None)
            except ValueError as err:
                msgs.append(str(err))
        q.put((rank, msgs))
    finally:
        dist.destroy_process_group()


def test_reduce_transposed_refuses_bad_shapes():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_bad_bounds_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for _, msgs in results:
        assert all(m is not None for m in msgs), msgs
        assert "do not tile" in msgs[0] and "partial_full" in msgs[1]
