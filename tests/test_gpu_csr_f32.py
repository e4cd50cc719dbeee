"""CSR with single-precision value storage (format 6) and spmv_refine on the GPU.

Exact: on dyadic inputs (tests/exact.py) the forward product at every lane count, spmv_apply_dot's overwrite and fused dot and the
transposed product are held to integer arithmetic bit for bit, at the row lengths where the kernel's loops change shape.
Rounded: the conversion and its statistics equal the NumPy twin (tests/csr_f32_ref.py); the product equals, bit for bit, the fp64
CSR handle of the widened values forced to the row-parallel kernel at the same lanes (the kernel's contract), and lies in the derived
gate of the twin's long-double product: a row of t entries is a sum of t + 1 terms, any order of them, with or without fma, stays
within (t + 1) * 2^-52 * (|A||x| + |y0|)_i of the exact sum to first order.
Then the plumbing, the solvers on a format-6 handle, and refinement against the twin's loop - the yardstick, never the engine - with
the branches of the loop that a converging solve never takes; last, the set-up past one trip of its grid on block-diagonal copies
(tests/tiled.py): bytes, statistics, refusals and exact products.
"""
import gc

import numpy as np
import pytest

import csr_f32_ref as ref
import exact
import tiled

pytestmark = pytest.mark.gpu
AUTO, VECTOR, PANEL = 0, 1, 4
INVALID, UNSUPPORTED = -1, -5
GUARD = 12345.0
LANES = (1, 2, 4, 8, 16, 32, 64)
NCOL = 1003


def _pick_lanes(mean):
    lanes = 1
    while lanes < 64 and lanes * 4 < mean:
        lanes *= 2
    return lanes


def _refused(pkg, code, match, call):
    """call() raises SpmvError with this code and a message that matches (the exception is dropped here: it holds the handle's frames)"""
    with pytest.raises(pkg.capi.SpmvError, match=match) as ei:
        call()
    got = ei.value.code
    del ei
    assert got == code, (got, match)


def _guarded(ctx, host):
    """(a Vector over the first len(host) entries of device memory that holds one guard element more, a reader of all of it)"""
    big = ctx.vector_from(np.concatenate([host, [GUARD]]))
    v = ctx.wrap_vector(big.device_ptr, len(host))
    v._keep = big
    return v, big.download


def _lengths(lpr):
    """the row lengths at which csr_f32_kernel<lpr> takes another path: none, one lane, one short of / exactly / one more than a
    group's width, the same around the four entries in flight per lane, a fifth round, and a long row"""
    return sorted({0, 1, lpr - 1, lpr, lpr + 1, 4 * lpr - 1, 4 * lpr, 4 * lpr + 1, 5 * lpr, 1000})


def _structure(rng, counts, ncol=NCOL):
    """row pointer and columns: counts[i] distinct columns per row in random order; every second non-empty row holds the last column"""
    cols = []
    for i, n in enumerate(counts):
        c = rng.permutation(ncol)[:n]
        if n and i % 2 == 0 and ncol - 1 not in c:
            c[rng.integers(n)] = ncol - 1
        cols.append(c)
    cols = np.concatenate(cols).astype(np.int32) if len(counts) else np.zeros(0, np.int32)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), cols


def _exact_matrices(lpr):
    out = [(f"one row of {n}", [n]) for n in _lengths(lpr)]
    L = _lengths(lpr)
    out.append(("37 rows", [L[i % len(L)] for i in range(37)]))  # 256 / lpr rows per workgroup: the last one is part-filled at every lpr
    out.append(("no rows", []))
    out.append(("no entries", [0] * 37))
    return out


@pytest.mark.parametrize("lpr", LANES)
def test_products_are_exact_on_dyadic_inputs(ctx, lpr):
    rng = np.random.default_rng(600 + lpr)
    for name, counts in _exact_matrices(lpr):
        nrow, nnz = len(counts), int(sum(counts))
        rp, col = _structure(rng, counts)
        bits, e = exact.choose_bits_dot(max(nnz, 1), max(nrow, 1))
        val = exact.dyadic(rng, nnz, bits, e)  # mixed signs, a few mantissa bits: floats, every one
        C = ctx.csr(nrow, NCOL, rp, col, val)
        A = ctx.csr_to_f32(C)
        info = A.info
        assert (info.format, info.nrow, info.ncol, info.nnz, info.kernel) == (6, nrow, NCOL, nnz, VECTOR), name
        assert info.max_row_nnz == max(counts, default=0) and info.lanes_per_row == _pick_lanes(nnz / nrow if nrow else 0.0), name
        assert A.f32_info() == (0, 0, 0.0), name
        a, b, v = A.download()
        assert np.array_equal(a, rp) and np.array_equal(b, col) and np.array_equal(v, val), f"{name}: download"
        for got, want in zip(ctx.f32_to_csr(A).download(), (rp, col, val)):
            assert np.array_equal(got, want), f"{name}: f32_to_csr(csr_to_f32(A))"
        A.validate()
        i, j, _ = exact.csr_entries(rp, col, val)
        x = exact.poison(exact.dyadic(rng, NCOL, bits, e), j)  # NaN / inf at every column no entry reads
        y0 = exact.dyadic(rng, nrow, bits, e)
        dx = ctx.vector_from(x)
        A.set_kernel(VECTOR, lpr)
        assert A.info.lanes_per_row == lpr and A.info.kernel == VECTOR
        # forward, y += A x
        dy, read = _guarded(ctx, y0)
        ctx.apply(A, dx, dy)
        ctx.sync()
        got = read()
        assert got[nrow] == GUARD, f"lpr {lpr} {name}: y written at nrow"
        assert np.array_equal(got[:nrow], exact.exact_product(nrow, i, j, val, x, e, y0=y0)), f"lpr {lpr} {name}: forward"
        # spmv_apply_dot: y = A x over whatever y held, and w . y in the same launch
        w = exact.dyadic(rng, nrow, bits, e)
        want = exact.exact_product(nrow, i, j, val, x, e)
        dy, read = _guarded(ctx, np.full(nrow, np.nan))
        dot = ctx.apply_dot(A, dx, dy, ctx.vector_from(w), overwrite=True)
        got = read()
        assert got[nrow] == GUARD and np.array_equal(got[:nrow], want), f"lpr {lpr} {name}: overwrite"
        assert dot == exact.exact_dot(w, want, e, 2 * e), f"lpr {lpr} {name}: fused dot"
        want = exact.exact_product(nrow, i, j, val, x, e, y0=y0)
        dy, read = _guarded(ctx, y0)
        dot = ctx.apply_dot(A, dx, dy, ctx.vector_from(w), overwrite=False)
        assert np.array_equal(read()[:nrow], want) and dot == exact.exact_dot(w, want, e, 2 * e), f"lpr {lpr} {name}: y += A x with the dot"
        # transposed: x has nrow entries (poisoned at the rows without an entry), y NCOL and its guard
        xt = exact.poison(exact.dyadic(rng, nrow, bits, e), i)
        yt0 = exact.dyadic(rng, NCOL, bits, e)
        dyt, read = _guarded(ctx, yt0)
        ctx.apply_transpose(A, ctx.vector_from(xt), dyt)
        ctx.sync()
        got = read()
        assert got[NCOL] == GUARD, f"lpr {lpr} {name}: transposed y written at ncol"
        assert np.array_equal(got[:NCOL], exact.exact_product(NCOL, j, i, val, xt, e, y0=yt0)), f"lpr {lpr} {name}: transposed"
        assert A.get_param("transpose_ready") == 1 and A.get_param("transpose_kernel") == VECTOR


# ---- rounded values -------------------------------------------------------------------------------------------------------------------
def _rounded_inputs():
    rng = np.random.default_rng(71)
    L = sorted({n for lpr in LANES for n in (0, 1, lpr + 1, 4 * lpr + 1)} | {300})
    counts = [L[(5 * i) % len(L)] for i in range(300)]
    rp, col = _structure(rng, counts)
    val = rng.standard_normal(len(col)) * np.ldexp(1.0, rng.integers(-30, 31, size=len(col)))  # essentially every one takes a rounding
    return len(counts), rp, col, val


ROUNDED = _rounded_inputs()


def test_conversion_and_statistics_equal_the_twin(ctx):
    nrow, rp, col, val = ROUNDED
    f, inexact, under, rel = ref.demote(val)
    assert inexact > 0.99 * len(val) and under == 0
    A = ctx.csr_to_f32(ctx.csr(nrow, NCOL, rp, col, val))
    a, b, v = A.download()
    assert np.array_equal(a, rp) and np.array_equal(b, col)
    assert np.array_equal(v.view(np.uint64), ref.widen(f).view(np.uint64)), "the conversion is np.float32's rounding, bit for bit"
    assert A.f32_info() == (inexact, under, rel)
    assert ctx.csr_to_f32(ctx.csr(nrow, NCOL, rp, col, val)).f32_info() == (inexact, under, rel)  # the same bits after every call
    # an uploaded handle holds the same stream and reports zeros
    U = ctx.csr_f32(nrow, NCOL, rp, col, f)
    assert U.f32_info() == (0, 0, 0.0)
    for got, want in zip(U.download(), (a, b, v)):
        assert np.array_equal(got, want)


def test_product_equals_the_row_parallel_product_of_the_widened_values(ctx):
    nrow, rp, col, val = ROUNDED
    f = ref.demote(val)[0]
    A = ctx.csr_to_f32(ctx.csr(nrow, NCOL, rp, col, val))
    W = ctx.csr(nrow, NCOL, rp, col, ref.widen(f))
    rng = np.random.default_rng(72)
    x, y0 = rng.standard_normal(NCOL), rng.standard_normal(nrow)
    want = ref.product(rp, col, f, x, y0)
    scale, t = ref.abs_product(rp, col, f, x)
    bound = (t + 1) * 2.0**-52 * (scale + np.abs(y0))
    dx = ctx.vector_from(x)
    for lanes in LANES:
        A.set_kernel(VECTOR, lanes)
        W.set_kernel(VECTOR, lanes)
        assert (A.info.kernel, A.info.lanes_per_row, W.info.kernel, W.info.lanes_per_row) == (VECTOR, lanes, VECTOR, lanes)
        dya, dyw = ctx.vector_from(y0), ctx.vector_from(y0)
        ctx.apply(A, dx, dya)
        ctx.apply(W, dx, dyw)
        ctx.sync()
        ya, yw = dya.download(), dyw.download()
        assert np.array_equal(ya.view(np.uint64), yw.view(np.uint64)), f"lanes {lanes}: the contract of csr_f32_kernel"
        err = np.abs((ya.astype(np.longdouble) - want).astype(np.float64))
        worst = float(np.max(err / np.maximum(bound, 1e-300), initial=0.0))
        print(f"lanes {lanes}: worst error / bound = {worst:.3f}")
        assert np.all(err <= bound), f"lanes {lanes}: {worst:.3f} of the bound"


def test_values_that_cannot_be_stored_refuse_the_conversion_and_small_ones_are_counted(ctx, pkg):
    nrow, rp, col, val = ROUNDED
    bad = val.copy()
    r_nan, r_big = 17, 140  # (rows with entries)
    assert rp[r_nan + 1] > rp[r_nan] and rp[r_big + 1] > rp[r_big]
    bad[rp[r_big]] = 1e39
    bad[rp[r_nan + 1] - 1] = np.nan
    C = ctx.csr(nrow, NCOL, rp, col, bad)
    _refused(pkg, INVALID, r"spmv_csr_to_f32: 2 values .* row 17\)", lambda: ctx.csr_to_f32(C))
    with np.errstate(over="ignore"):
        as_float = np.where(np.isnan(bad), 1.0, bad).astype(np.float32)  # 1e39 is inf as a float
    _refused(pkg, INVALID, r"spmv_csr_f32_upload: 1 values .* row 140\)", lambda: ctx.csr_f32(nrow, NCOL, rp, col, as_float))
    small = val.copy()
    at = [int(rp[r_big]), int(rp[r_nan]), int(rp[200])]
    small[at] = [1e-46, -1e-40, 2.0**-149]  # to zero; to a subnormal; a subnormal float as it is
    f, inexact, under, rel = ref.demote(small)
    assert under == 3 and f[at[0]] == 0.0
    A = ctx.csr_to_f32(ctx.csr(nrow, NCOL, rp, col, small))
    assert A.f32_info() == (inexact, under, rel)
    assert np.array_equal(A.download()[2].view(np.uint64), ref.widen(f).view(np.uint64))


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------------
def test_info_memory_validate_and_set_kernel(ctx, pkg):
    nrow, rp, col, val = ROUNDED
    nnz = len(col)
    f = ref.demote(val)[0]

    def round_trip():
        A = ctx.csr_f32(nrow, NCOL, rp, col, f)
        info = A.info
        assert (info.format, info.nrow, info.ncol, info.ell_k, info.nnz, info.row_begin, info.kernel) == (6, nrow, NCOL, 0, nnz, 0, VECTOR)
        assert info.max_row_nnz == 300 and info.lanes_per_row == _pick_lanes(nnz / nrow)
        own = 4 * (nrow + 1) + 8 * nnz
        assert info.device_bytes == own  # no array is empty here
        A.validate()
        for lanes in LANES:
            A.set_kernel(VECTOR, lanes)
            assert A.info.lanes_per_row == lanes
        A.set_kernel(VECTOR, 0)
        assert A.info.lanes_per_row == 64  # 0 keeps what is there
        A.set_kernel(AUTO, 0)
        assert A.info.lanes_per_row == info.lanes_per_row and A.info.kernel == VECTOR
        for kernel, lanes in ((PANEL, 0), (2, 0), (VECTOR, 3), (VECTOR, 128)):
            _refused(pkg, UNSUPPORTED, "spmv_mat_set_kernel.*format 6", lambda: A.set_kernel(kernel, lanes))
        assert A.info.lanes_per_row == info.lanes_per_row
        # the device-level refusals
        _refused(pkg, UNSUPPORTED, "spmv_apply_multi.*format 6", lambda: ctx.apply_multi(A, ctx.vector(2 * NCOL), ctx.vector(2 * nrow), 2))
        _refused(pkg, UNSUPPORTED, "spmv_mat_get_plan.*format 6", lambda: A.get_plan())
        plan = ctx.csr(nrow, NCOL, rp, col, val).get_plan()
        _refused(pkg, UNSUPPORTED, "spmv_mat_set_plan.*format 6", lambda: A.set_plan(plan))
        _refused(pkg, UNSUPPORTED, "spmv_mat_set_flags.*format 6", lambda: A.set_flags(pkg.capi.FLAG_DPP_REDUCE))
        A.set_flags(0)
        _refused(pkg, UNSUPPORTED, "spmv_mat_partition_rows.*format 6", lambda: A.partition_rows(4, balance_entries=True))
        assert list(A.partition_rows(3)) == [0, 100, 200, 300]
        # the transposed handle's memory is the handle's: counted at transpose_setup, gone with the handle
        assert A.get_param("transpose_ready") == 0
        A.transpose_setup()
        comp = 4 * (NCOL + 1) + 8 * nnz
        assert A.info.device_bytes == own + comp and A.get_param("transpose_bytes") == comp
        A.transpose_setup()
        assert A.info.device_bytes == own + comp
        B = ctx.f32_to_csr(A)
        assert B.info.format == 1 and B.info.nnz == nnz
        del A, B
        ctx.sync()

    round_trip()  # (what the context itself keeps grows on first use)
    gc.collect()
    before = ctx.mem_info()[0]
    round_trip()
    gc.collect()
    assert ctx.mem_info()[0] == before, "handles, the companion and the fp64 intermediates of its set-up go back"


def test_validate_catches_a_column_out_of_range_and_a_decreasing_pointer(ctx, pkg):
    nrow, rp, col, val = ROUNDED
    f = ref.demote(val)[0]
    bad = col.copy()
    bad[len(bad) // 2] = NCOL
    with pytest.raises(pkg.capi.SpmvError, match="index out of range"):
        ctx.csr_f32(nrow, NCOL, rp, bad, f)
    neg = col.copy()
    neg[3] = -1
    with pytest.raises(pkg.capi.SpmvError, match="index out of range"):
        ctx.csr_f32(nrow, NCOL, rp, neg, f)
    down = rp.copy()
    k = int(np.flatnonzero(np.diff(rp) > 1)[0]) + 1
    down[k] = down[k - 1] - 1 if down[k - 1] > 0 else down[k + 1] + 1
    with pytest.raises(pkg.capi.SpmvError, match="offsets decrease"):
        ctx.csr_f32(nrow, NCOL, down, col, f)


def test_apply_host_adds_the_product_onto_host_vectors(ctx):
    nrow, rp, col, val = ROUNDED
    f = ref.demote(val)[0]
    A = ctx.csr_f32(nrow, NCOL, rp, col, f)
    rng = np.random.default_rng(73)
    x, y0 = rng.standard_normal(NCOL), rng.standard_normal(nrow)
    y = y0.copy()
    ctx.apply_host(A, x, y)
    dy = ctx.vector_from(y0)
    ctx.apply(A, ctx.vector_from(x), dy)
    ctx.sync()
    assert np.array_equal(y.view(np.uint64), dy.download().view(np.uint64))  # the same kernel, the same IEEE add onto y
    scale, t = ref.abs_product(rp, col, f, x)
    err = np.abs((y.astype(np.longdouble) - ref.product(rp, col, f, x, y0)).astype(np.float64))
    assert np.all(err <= (t + 1) * 2.0**-52 * (scale + np.abs(y0)))


# ---- solvers and refinement ---------------------------------------------------------------------------------------------------------------
def _system():
    n, rp, col, val = ref.scaled_laplacian()
    f = ref.demote(val)[0]
    b = np.random.default_rng(11).standard_normal(n)
    return n, rp, col, val, f, ref.dense(n, n, rp, col, val), ref.dense(n, n, rp, col, ref.widen(f)), b


SYSTEM = _system()


def _true_residual(M, x, b):
    """||b - M x|| / ||b|| on the host in long double"""
    r = b.astype(np.longdouble) - M.astype(np.longdouble) @ x.astype(np.longdouble)
    return float(np.sqrt(r @ r) / np.sqrt(b.astype(np.longdouble) @ b.astype(np.longdouble)))


def test_solvers_run_on_a_format_6_handle(ctx):
    """to 1e-8 of ITS OWN system, the widened matrix.  The solvers stop on their recurrence residual; the true one differs from it by
    the rounding of a few hundred iterations, O(iterations * 2^-53 * cond) ~ 1e-11 relative to ||b||: 1e-3 of the tolerance is allowed"""
    n, rp, col, val, f, A64, A32, b = SYSTEM
    A = ctx.csr_to_f32(ctx.csr(n, n, rp, col, val))
    assert A.f32_info()[0] > 0.99 * len(val)
    db = ctx.vector_from(b)
    tol = 1e-8
    for name, run in (("cg", lambda dx: ctx.cg(A, db, dx, max_iter=5000, rel_tol=tol)),
                      ("bicgstab", lambda dx: ctx.bicgstab(A, db, dx, max_iter=5000, rel_tol=tol)),
                      ("gmres", lambda dx: ctx.gmres(A, db, dx, restart=64, max_iter=20000, rel_tol=tol))):
        dx = ctx.vector_from(np.zeros(n))
        iters, res = run(dx)
        ctx.sync()
        true = _true_residual(A32, dx.download(), b)
        print(f"{name}: {iters} iterations, reported {res:.3e}, true {true:.3e}")
        assert 0 < iters and res <= tol and true <= tol * (1 + 1e-3), (name, iters, res, true)
    dx = ctx.vector_from(np.zeros(n))
    iters, nres, res = ctx.cgls(A, db, dx, max_iter=20000, rel_tol=tol)
    ctx.sync()
    x = dx.download()
    r = b.astype(np.longdouble) - A32.astype(np.longdouble) @ x.astype(np.longdouble)
    normal = float(np.linalg.norm((A32.T.astype(np.longdouble) @ r).astype(np.float64)) / np.linalg.norm(A32.T @ b))
    print(f"cgls: {iters} iterations, reported {nres:.3e}, true normal residual {normal:.3e}")
    assert 0 < iters and nres <= tol and normal <= tol * (1 + 1e-3) and A.get_param("transpose_ready") == 1


def test_the_rounded_matrix_alone_stalls_and_refinement_reaches_fp64_accuracy(ctx):
    n, rp, col, val, f, A64, A32, b = SYSTEM
    A = ctx.csr(n, n, rp, col, val)
    L = ctx.csr_to_f32(A)
    db = ctx.vector_from(b)
    # (a) the format-6 handle alone, solved far below its rounding: the residual against the TRUE matrix stays where the rounding
    # of the values put it (the twin's run: 1.7e-7) - this system needs refinement
    dx = ctx.vector_from(np.zeros(n))
    ctx.cg(L, db, dx, max_iter=5000, rel_tol=1e-13)
    ctx.sync()
    alone = _true_residual(A64, dx.download(), b)
    print(f"(a) spmv_cg on the format-6 handle alone: true residual {alone:.3e}")
    assert alone > 1e-9
    # (b) refinement
    dx = ctx.vector_from(np.zeros(n))
    outer, inner, res = ctx.refine(A, L, db, dx, solver=0, precond=0, max_outer=20, inner_max_iter=1000, inner_tol=1e-4, rel_tol=1e-12)
    true = _true_residual(A64, dx.download(), b)
    xt = np.zeros(n)
    t_outer, t_inner, t_res = ref.refine(A64, A32, b, xt, 1e-4, 1e-12, 20, 1000)
    print(f"(b) spmv_refine: outer {outer} inner {inner} reported {res:.3e} true {true:.3e}; twin: outer {t_outer} inner {t_inner} resid {t_res:.3e}")
    assert true <= 1e-12 and res <= 1e-12
    assert abs(res - true) <= 1e-3 * true
    assert abs(outer - t_outer) <= 1 and abs(inner - t_inner) <= 0.1 * t_inner + 2
    # (f) BiCGSTAB as the inner solver
    dx = ctx.vector_from(np.zeros(n))
    outer, inner, res = ctx.refine(A, L, db, dx, solver=1, precond=0, max_outer=20, inner_max_iter=1000, inner_tol=1e-4, rel_tol=1e-12)
    true = _true_residual(A64, dx.download(), b)
    print(f"(f) inner BiCGSTAB: outer {outer} inner {inner} reported {res:.3e} true {true:.3e}")
    assert true <= 1e-12 and res <= 1e-12 and 1 <= outer <= 20


def test_the_edges_of_the_refinement_loop(ctx):
    n, rp, col, val, f, A64, A32, b = SYSTEM
    A = ctx.csr(n, n, rp, col, val)
    L = ctx.csr_to_f32(A)
    db = ctx.vector_from(b)
    # (c) A_lo = A, the inner solve to 1e-12: one outer step.  (The outer tolerance is 1e-10: the inner solver stops on its
    # recurrence residual, which its true residual - what the next outer step measures - follows to O(iterations * 2^-53 * cond)
    # ~ 1e-11 relative to ||b||, not to the last digit of 1e-12.)
    dx = ctx.vector_from(np.zeros(n))
    outer, inner, res = ctx.refine(A, A, db, dx, inner_max_iter=5000, inner_tol=1e-12, rel_tol=1e-10)
    assert outer == 1 and inner > 0 and res <= 1e-10 and _true_residual(A64, dx.download(), b) <= 1e-10
    # (d) b = 0 leaves x untouched
    x0 = np.arange(1.0, n + 1.0)
    dx = ctx.vector_from(x0)
    assert ctx.refine(A, L, ctx.vector_from(np.zeros(n)), dx) == (0, 0, 0.0)
    assert np.array_equal(dx.download(), x0)
    # (e) max_outer = 1 returns after one step, with the residual of the x it returns
    dx = ctx.vector_from(np.zeros(n))
    outer, inner, res = ctx.refine(A, L, db, dx, max_outer=1, inner_tol=1e-4, rel_tol=1e-12)
    true = _true_residual(A64, dx.download(), b)
    assert outer == 1 and inner > 0 and 1e-12 < res < 1e-2 and abs(res - true) <= 1e-3 * true
    # max_outer = 0: the residual of the x passed in, nothing else
    dx = ctx.vector_from(np.zeros(n))
    assert ctx.refine(A, L, db, dx, max_outer=0) == (0, 0, 1.0) and np.array_equal(dx.download(), np.zeros(n))
    # an inner solve that runs out of iterations is no error: its correction is used
    dx = ctx.vector_from(np.zeros(n))
    outer, inner, res = ctx.refine(A, L, db, dx, max_outer=3, inner_max_iter=5, inner_tol=1e-4, rel_tol=1e-12)
    assert outer == 3 and inner == 15 and res < 1.0


def test_a_step_that_grows_the_residual_gives_the_iterate_back(ctx):
    """A_lo = 0.4 A: the correction is 2.5 times the right one, x = 0 + 2.5 A^-1 b has the residual 1.5 ||b||, and the loop takes the
    branch "the step did not reduce ||r||": x is the iterate before the step, bit for bit, and res is its residual (the twin:
    (1, 88, 1.0) with x back at zeros)"""
    n, rp, col, val, f, A64, A32, b = SYSTEM
    A = ctx.csr(n, n, rp, col, val)
    A.set_kernel(VECTOR)  # the same bits of every residual from call to call
    A_lo = ctx.csr(n, n, rp, col, 0.4 * val)
    db = ctx.vector_from(b)
    dx = ctx.vector_from(np.zeros(n))
    outer, inner, res = ctx.refine(A, A_lo, db, dx, inner_tol=1e-4, rel_tol=1e-12)
    assert (outer, res) == (1, 1.0) and inner > 0, (outer, inner, res)
    assert np.array_equal(dx.download().view(np.uint64), np.zeros(n).view(np.uint64)), "x is not the iterate before the step"
    x0 = np.random.default_rng(12).standard_normal(n)
    dx = ctx.vector_from(x0)
    res0 = ctx.refine(A, A_lo, db, dx, max_outer=0)
    assert res0[:2] == (0, 0) and res0[2] > 1e-3 and np.array_equal(dx.download().view(np.uint64), x0.view(np.uint64))
    outer, inner, res = ctx.refine(A, A_lo, db, dx, inner_tol=1e-4, rel_tol=1e-12)
    assert outer == 1 and inner > 0 and res == res0[2], (outer, inner, res, res0)
    assert np.array_equal(dx.download().view(np.uint64), x0.view(np.uint64)), "x is not the x0 passed in"


def test_refinement_converges_then_stalls_and_returns_the_best_iterate(ctx):
    """rel_tol = 0 can never be met: the residual falls to the rounding of the fp64 residual itself, a step no longer reduces it, and
    the loop returns the iterate before that step with ITS residual (the twin stops after 6 outer steps at 6.65e-16)"""
    n, rp, col, val, f, A64, A32, b = SYSTEM
    A = ctx.csr(n, n, rp, col, val)
    A.set_kernel(VECTOR)
    L = ctx.csr_to_f32(A)
    db = ctx.vector_from(b)
    dx = ctx.vector_from(np.zeros(n))
    outer, inner, res = ctx.refine(A, L, db, dx, max_outer=50, inner_tol=1e-4, rel_tol=0.0)
    x = dx.download()
    true = _true_residual(A64, x, b)
    print(f"rel_tol = 0: outer {outer} inner {inner} reported {res:.3e} true {true:.3e}")
    assert 1 < outer < 50 and inner > 0
    again = ctx.refine(A, L, db, dx, max_outer=0)
    assert again == (0, 0, res), (again, res)
    assert np.array_equal(dx.download().view(np.uint64), x.view(np.uint64))
    assert true <= 1e-14


def test_refinement_with_a_preconditioned_inner_solver(ctx, pkg):
    """precond reaches the inner solver: with A_lo = A from x = 0 the first residual is b itself and the inner solve is spmv_cg's
    driver on (A, b), so its count is that of ctx.cg with the Jacobi preconditioner; a format-6 A_lo has no diagonal to read"""
    n, rp, col, val, f, A64, A32, b = SYSTEM
    JACOBI = pkg.capi.PRECOND_JACOBI
    A = ctx.csr(n, n, rp, col, val)
    A.set_kernel(VECTOR)
    db = ctx.vector_from(b)
    dx = ctx.vector_from(np.zeros(n))
    iters, _ = ctx.cg(A, db, dx, max_iter=5000, rel_tol=1e-12, jacobi=True)
    dx0 = ctx.vector_from(np.zeros(n))
    plain, _ = ctx.cg(A, db, dx0, max_iter=5000, rel_tol=1e-12)
    dx = ctx.vector_from(np.zeros(n))
    outer, inner, res = ctx.refine(A, A, db, dx, precond=JACOBI, inner_max_iter=5000, inner_tol=1e-12, rel_tol=1e-10)
    print(f"precond = JACOBI: outer {outer} inner {inner} (spmv_cg: {iters} with Jacobi, {plain} without) reported {res:.3e}")
    assert outer == 1 and inner == iters and 0 < iters and res <= 1e-10, (outer, inner, iters, res)
    assert _true_residual(A64, dx.download(), b) <= 1e-10
    L = ctx.csr_to_f32(A)
    x0 = np.arange(1.0, n + 1.0)
    dx = ctx.vector_from(x0)
    _refused(pkg, UNSUPPORTED, "Jacobi", lambda: ctx.refine(A, L, db, dx, precond=JACOBI))
    assert np.array_equal(dx.download().view(np.uint64), x0.view(np.uint64))


# ---- set-up kernels past one trip of their grid (tests/tiled.py) ---------------------------------------------------------------------------
TRIP = tiled.max_grid() * tiled.block_lanes()  # items of one trip of a grid-stride kernel of csrc/convert_f32.hip
TNCOL = ref.TILED_NCOL


def _copies(rp):
    k, cond = ref.tiled_copies(rp, TRIP)
    assert all(cond.values()), (k, cond)
    return k


def _same_bytes(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        at = int(np.flatnonzero(got.view(np.uint64 if got.dtype == np.float64 else np.int32) != want.view(np.uint64 if got.dtype == np.float64 else np.int32))[0])
        raise AssertionError(f"{what}[{at}] is {got[at]!r} against {want[at]!r}, trip {at // TRIP} of a kernel over this array")


def test_conversion_and_statistics_of_block_diagonal_copies_past_one_trip(ctx):
    """k copies of a 128-row base with the row lengths of ROUNDED: f32_pack, f32_widen and the row maximum take a later trip; the
    words are the base's tiled, the counts k times the base's, the largest change the base's - or that of one value of the LAST copy"""
    rp0, col0, val0 = ref.tiled_rounded()
    nrow0, nnz0 = len(rp0) - 1, len(val0)
    k = _copies(rp0)
    nrow, ncol = k * nrow0, k * TNCOL
    f0, inexact0, under0, rel0 = ref.demote(val0)
    assert under0 == 3 and inexact0 > 0.99 * nnz0
    rp, col, val = tiled.tile_csr(k, TNCOL, rp0, col0, val0)
    print(f"{k} copies: {nrow} rows, {len(val)} entries, one trip {TRIP}")
    A = ctx.csr_to_f32(ctx.csr(nrow, ncol, rp, col, val))
    assert A.f32_info() == (k * inexact0, k * under0, rel0)
    assert (A.info.nnz, A.info.max_row_nnz) == (k * nnz0, 300)
    assert tiled.tiled_mismatch(A.download(), (rp0, col0, ref.widen(f0)), k, TNCOL) is None
    assert tiled.tiled_mismatch(ctx.f32_to_csr(A).download(), (rp0, col0, ref.widen(f0)), k, TNCOL) is None
    del A
    # one value of the last copy raises the largest relative change: the maximum over the bits is formed across the trips
    worse = val.copy()
    worse[-1] = ref.WORST_VALUE
    assert ref.WORST_REL > rel0 and ref.demote(worse[-nnz0:])[1:] == (inexact0, under0, ref.WORST_REL)
    assert ctx.csr_to_f32(ctx.csr(nrow, ncol, rp, col, worse)).f32_info() == (k * inexact0, k * under0, ref.WORST_REL)
    # the float stream uploaded: the same bytes, no statistics
    U = ctx.csr_f32(nrow, ncol, rp, col, np.tile(f0, k))
    assert U.f32_info() == (0, 0, 0.0) and U.info.max_row_nnz == 300
    assert tiled.tiled_mismatch(U.download(), (rp0, col0, ref.widen(f0)), k, TNCOL) is None


def test_products_of_block_diagonal_copies_are_exact_past_one_trip(ctx):
    """dyadic values on the same pattern: the forward product, spmv_apply_dot and the transposed product - whose set-up widens,
    transposes and packs 4.4 M entries - are the base's integer results tiled"""
    rp0, col0 = ref.tiled_structure()
    nrow0, nnz0 = len(rp0) - 1, len(col0)
    k = _copies(rp0)
    nrow, ncol = k * nrow0, k * TNCOL
    rng = np.random.default_rng(173)
    bits, e = exact.choose_bits_dot(k * nnz0, max(nrow, ncol))
    val0 = exact.dyadic(rng, nnz0, bits, e)
    i, j, _ = exact.csr_entries(rp0, col0, val0)
    x0, y00, w0 = exact.poison(exact.dyadic(rng, TNCOL, bits, e), j), exact.dyadic(rng, nrow0, bits, e), exact.dyadic(rng, nrow0, bits, e)
    xt0, yt00 = exact.poison(exact.dyadic(rng, nrow0, bits, e), i), exact.dyadic(rng, TNCOL, bits, e)
    A = ctx.csr_to_f32(ctx.csr(nrow, ncol, *tiled.tile_csr(k, TNCOL, rp0, col0, val0)))
    assert A.f32_info() == (0, 0, 0.0)
    dx, dw = ctx.vector_from(np.tile(x0, k)), ctx.vector_from(np.tile(w0, k))
    onto, over = exact.exact_product(nrow0, i, j, val0, x0, e, y0=y00), exact.exact_product(nrow0, i, j, val0, x0, e)
    dy = ctx.vector_from(np.tile(y00, k))
    ctx.apply(A, dx, dy)
    ctx.sync()
    _same_bytes(dy.download(), np.tile(onto, k), "forward: y")
    dy = ctx.vector_from(np.full(nrow, np.nan))
    dot = ctx.apply_dot(A, dx, dy, dw, overwrite=True)
    _same_bytes(dy.download(), np.tile(over, k), "apply_dot: y")
    assert dot == exact.exact_dot(np.tile(w0, k), np.tile(over, k), e, 2 * e), "the dot over every copy"
    dyt = ctx.vector_from(np.tile(yt00, k))
    ctx.apply_transpose(A, ctx.vector_from(np.tile(xt0, k)), dyt)
    ctx.sync()
    _same_bytes(dyt.download(), np.tile(exact.exact_product(TNCOL, j, i, val0, xt0, e, y0=yt00), k), "transposed: y")


def test_refusals_find_values_and_columns_on_a_later_trip(ctx, pkg):
    """a NaN in the last copy and a 1e39 in a copy beyond the first trip: both counted, and the first refused row is the EARLIER one,
    by its global index; a packed column equal to ncol in the last entry is refused at upload"""
    rp0, col0, val0 = ref.tiled_rounded()
    nrow0, nnz0 = len(rp0) - 1, len(val0)
    k = _copies(rp0)
    nrow, ncol = k * nrow0, k * TNCOL
    rp, col, val = tiled.tile_csr(k, TNCOL, rp0, col0, val0)
    copy, r_big, r_nan = TRIP // nnz0 + 2, 43, 11  # (rows with entries)
    assert rp0[r_big + 1] > rp0[r_big] and rp0[r_nan + 1] > rp0[r_nan] and copy * nnz0 > TRIP and copy < k - 1
    val[copy * nnz0 + rp0[r_big]] = 1e39
    val[(k - 1) * nnz0 + rp0[r_nan]] = np.nan
    C = ctx.csr(nrow, ncol, rp, col, val)
    _refused(pkg, INVALID, rf"spmv_csr_to_f32: 2 values .* row {copy * nrow0 + r_big}\)", lambda: ctx.csr_to_f32(C))
    del C
    f = np.tile(ref.demote(val0)[0], k)
    bad = col.copy()
    bad[-1] = ncol
    with pytest.raises(pkg.capi.SpmvError, match="index out of range"):
        ctx.csr_f32(nrow, ncol, rp, bad, f)


def test_the_longest_row_is_found_on_a_later_trip(ctx):
    """csr_f32_row_max_kernel: one trip and 5 rows of one entry each, the last of three"""
    nrow = TRIP + 5
    rp = np.concatenate([np.arange(nrow), [nrow + 2]]).astype(np.int32)
    col = np.concatenate([np.arange(nrow - 1) % 3, [0, 1, 2]]).astype(np.int32)
    A = ctx.csr_f32(nrow, 3, rp, col, np.ones(len(col), np.float32))
    assert (A.info.nnz, A.info.max_row_nnz) == (len(col), 3)
