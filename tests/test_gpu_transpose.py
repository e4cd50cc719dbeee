"""The transposed product y += A^T x (spmv_apply_transpose) on the GPU, every format.

CSR, COO and ELL handles run on a companion handle whose kernel differs from the oracle's order, so they are held to the parity
gate; a CSC handle whose CSR companion is forced to the SCALAR kernel, and the DIA transposed kernel, are bit-identical to the
oracle's fma order (np.array_equal).  Every check runs after 1 call and after 50 accumulating calls from a non-zero y.
"""
import numpy as np
import pytest

import cases
import oracle_lib as ol
from conftest import perf_expect

pytestmark = pytest.mark.gpu
NUM_TEST = 50
AUTO, VECTOR, SCALAR, PANEL = 0, 1, 3, 4
COMPANION_KERNELS = (AUTO, VECTOR, PANEL)  # AUTO, the companion format's own kernel, the row-grouped copy


def _fixtures():
    """(name, nrow, ncol, row, col, val) of every golden case: tests/cases.py ALL_CASES and live_matrices()"""
    out = []
    for make in cases.ALL_CASES:
        c = make()
        out.append((c["name"], c["nrow"], c["ncol"], ol.i32(c["row"]), ol.i32(c["col"]), ol.f64(c["val"])))
    for i, (nrow, ncol, row, col, val, _x) in enumerate(cases.live_matrices()):
        out.append((f"live{i}", nrow, ncol, ol.i32(row), ol.i32(col), ol.f64(val)))
    return out


FIXTURES = _fixtures()


def _xy(nrow, ncol, seed):
    """x (nrow entries: A^T x) and a non-zero y0 (ncol)"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, size=nrow)
    y0 = rng.uniform(0.5, 1.5, size=ncol) * np.where(rng.random(ncol) < 0.5, -1.0, 1.0)
    return x, y0


def _engine(ctx, A, x, y0):
    """y after 1 and after NUM_TEST calls of apply_transpose"""
    dx, dy = ctx.vector_from(x), ctx.vector_from(y0)
    ctx.apply_transpose(A, dx, dy)
    ctx.sync()
    y1 = dy.download()
    for _ in range(NUM_TEST - 1):
        ctx.apply_transpose(A, dx, dy)
    ctx.sync()
    return y1, dy.download()


def _oracle(spmv, x, y0, reps):
    y = y0.copy()
    for _ in range(reps):
        spmv(x, y)
    return y


def _transposed_scale(orc, nrow, ncol, row, col, val, x):
    """(|A^T| |x|)_j from the host-transposed arrays (coo_to_csr with rows and columns swapped)"""
    trp, tcol, tval = ol.coo_to_csr(orc, ncol, ol.i32(col), ol.i32(row), ol.f64(val))
    s = np.zeros(ncol)
    ol.csr_abs_row_sums(orc, trp, tcol, tval, x, s)
    return s


def _check_parity(ctx, A, spmv, scale, x, y0, what):
    y1, y50 = _engine(ctx, A, x, y0)
    ol.assert_parity(y1, _oracle(spmv, x, y0, 1), scale + np.abs(y0), f"{what}: 1 call")
    ol.assert_parity(y50, _oracle(spmv, x, y0, NUM_TEST), NUM_TEST * scale + np.abs(y0), f"{what}: {NUM_TEST} calls")


def _check_bitwise(ctx, A, spmv, x, y0, what):
    y1, y50 = _engine(ctx, A, x, y0)
    assert np.array_equal(y1, _oracle(spmv, x, y0, 1)), f"{what}: 1 call"
    assert np.array_equal(y50, _oracle(spmv, x, y0, NUM_TEST)), f"{what}: {NUM_TEST} calls"


def _expect_companion_kernel(A, kernel, nnz):
    got = A.get_param("transpose_kernel")
    if kernel == AUTO:
        assert got in (VECTOR, PANEL), got
    elif nnz > 0:
        assert got == kernel, (got, kernel)
    assert A.get_param("transpose_ready") == 1


# ---- every format against its oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fx", FIXTURES, ids=lambda f: f[0])
def test_csr_transposed_matches_csc_oracle(ctx, orc, fx):
    name, nrow, ncol, row, col, val = fx
    rp, cc, cv = ol.coo_to_csr(orc, nrow, row, col, val)
    x, y0 = _xy(nrow, ncol, 11)
    scale = _transposed_scale(orc, nrow, ncol, row, col, val, x)
    for kernel in COMPANION_KERNELS:
        A = ctx.csr(nrow, ncol, rp, cc, cv)
        A.set_param("transpose_kernel", kernel)
        _check_parity(ctx, A, lambda xx, yy: ol.csc_spmv(orc, rp, cc, cv, xx, yy), scale, x, y0, f"{name} CSR kernel {kernel}")
        _expect_companion_kernel(A, kernel, len(cv))


@pytest.mark.parametrize("fx", FIXTURES, ids=lambda f: f[0])
def test_csc_transposed_with_scalar_companion_is_bitwise(ctx, orc, fx):
    name, nrow, ncol, row, col, val = fx
    cp, cr, cv = ol.coo_to_csc(orc, ncol, row, col, val)
    x, y0 = _xy(nrow, ncol, 12)
    A = ctx.csc(nrow, ncol, cp, cr, cv)
    A.set_param("transpose_kernel", SCALAR)
    # the CSC arrays ARE the CSR arrays of A^T: the scalar kernel's row sums are the oracle's fma order
    _check_bitwise(ctx, A, lambda xx, yy: ol.csr_spmv(orc, cp, cr, cv, xx, yy, fma=True), x, y0, f"{name} CSC, SCALAR companion")
    assert A.get_param("transpose_kernel") == SCALAR
    B = ctx.csc(nrow, ncol, cp, cr, cv)  # and AUTO
    scale = _transposed_scale(orc, nrow, ncol, row, col, val, x)
    _check_parity(ctx, B, lambda xx, yy: ol.csr_spmv(orc, cp, cr, cv, xx, yy), scale, x, y0, f"{name} CSC, AUTO companion")


@pytest.mark.parametrize("fx", FIXTURES, ids=lambda f: f[0])
def test_coo_transposed_matches_swapped_oracle(ctx, orc, fx):
    name, nrow, ncol, row, col, val = fx
    x, y0 = _xy(nrow, ncol, 13)
    scale = _transposed_scale(orc, nrow, ncol, row, col, val, x)
    for kernel in COMPANION_KERNELS:
        A = ctx.coo(nrow, ncol, row, col, val)
        A.set_param("transpose_kernel", kernel)
        _check_parity(ctx, A, lambda xx, yy: ol.coo_spmv(orc, col, row, val, xx, yy), scale, x, y0, f"{name} COO kernel {kernel}")
        _expect_companion_kernel(A, kernel, len(val))


@pytest.mark.parametrize("fx", FIXTURES, ids=lambda f: f[0])
def test_ell_transposed_matches_slot_list_oracle(ctx, orc, fx):
    """every slot counts, padding included: the oracle is the COO product over (col_ind, slot row) of all nrow * k slots"""
    name, nrow, ncol, row, col, val = fx
    k, ec, ev = ol.coo_to_ell(orc, nrow, row, col, val)
    slot_rows = ol.i32(np.tile(np.arange(nrow, dtype=np.int32), k))
    x, y0 = _xy(nrow, ncol, 14)
    scale = _transposed_scale(orc, nrow, ncol, slot_rows, ec, ev, x)
    for kernel in COMPANION_KERNELS:
        A = ctx.ell(nrow, ncol, k, len(val), ec, ev)
        A.set_param("transpose_kernel", kernel)
        _check_parity(ctx, A, lambda xx, yy: ol.coo_spmv(orc, ec, slot_rows, ev, xx, yy), scale, x, y0, f"{name} ELL kernel {kernel}")
        _expect_companion_kernel(A, kernel, nrow * k)
        assert A.get_param("transpose_bytes") >= 4 * nrow * k  # (the slot rows, plus the companion's own layouts)


def _dia_entries_jd(nrow, ncol, offsets, dval, jmax=None, js=None):
    """(row = output j, col = i, val) of every term of the DIA transposed product in (j, d) order (the kernel's contract)"""
    nd = len(offsets)
    jmax = min(nrow, ncol) if jmax is None else jmax
    js = np.arange(jmax, dtype=np.int64) if js is None else np.asarray(js, dtype=np.int64)
    J = np.repeat(js, nd)
    D = np.tile(np.arange(nd, dtype=np.int64), len(js))
    i = J - offsets.astype(np.int64)[D]
    keep = (i >= 0) & (i < nrow)
    return J[keep], i[keep], dval[i[keep] * nd + D[keep]]


def _check_dia(ctx, orc, nrow, ncol, offsets, dval, what, jmax=None, set_bound=False, seed=15):
    A = ctx.dia(nrow, ncol, offsets, dval)
    if set_bound:
        A.set_param("dia_col_bound", jmax)
    x, y0 = _xy(nrow, ncol, seed)
    r, c, v = _dia_entries_jd(nrow, ncol, offsets, dval, jmax)
    r, c, v = ol.i32(r), ol.i32(c), ol.f64(v)
    _check_bitwise(ctx, A, lambda xx, yy: ol.coo_spmv(orc, r, c, v, xx, yy, fma=True), x, y0, what)
    assert A.get_param("transpose_ready") == 1


# the fixtures with few enough diagonals to be stored as DIA (rectangular ones included)
DIA_FIXTURES = [f for f in FIXTURES if len(np.unique(f[4].astype(np.int64) - f[3])) <= 6000]


@pytest.mark.parametrize("fx", DIA_FIXTURES, ids=lambda f: f[0])
def test_dia_transposed_is_bitwise_in_jd_order(ctx, orc, fx):
    name, nrow, ncol, row, col, val = fx
    rp, cc, cv = ol.coo_to_csr(orc, nrow, row, col, val)
    offsets, dval = ol.csr_to_dia(orc, nrow, ncol, rp, cc, cv)
    _check_dia(ctx, orc, nrow, ncol, offsets, dval, f"{name} DIA ({len(offsets)} diagonals)")


@pytest.mark.parametrize("nrow,ncol,nd", [(3000, 3000, 16), (3001, 2500, 7), (2000, 3333, 33), (1000, 1000, 64), (4097, 4097, 9)])
def test_dia_bands_tiled_and_general(ctx, orc, nrow, ncol, nd):
    """bands (the tiled kernel, even and odd ndiags) and spread-out offsets (the general kernel), square and rectangular"""
    rng = np.random.default_rng(nrow + nd)
    band = ol.i32(np.arange(nd) - nd // 2)
    spread = ol.i32(np.sort(rng.choice(np.arange(-nrow + 1, ncol), size=nd, replace=False)))
    for offsets, kind in ((band, "band"), (spread, "spread"), (ol.i32(band[::-1].copy()), "band reversed")):
        dval = rng.uniform(-1, 1, size=nrow * nd)
        _check_dia(ctx, orc, nrow, ncol, offsets, dval, f"{kind} {nrow}x{ncol} nd={nd}")


def test_dia_row_shard_with_column_bound(ctx, orc):
    """a DIA row shard: offsets shifted by the shard's first row, dia_col_bound = the whole matrix's bound"""
    n, nd, r0, r1 = 5000, 12, 1700, 3400
    rng = np.random.default_rng(3)
    off = np.arange(nd) - 5
    dval = rng.uniform(-1, 1, size=(r1 - r0) * nd)
    _check_dia(ctx, orc, r1 - r0, n, ol.i32(off + r0), dval, "DIA shard", jmax=n, set_bound=True)


# ---- shards, isolation, edges -------------------------------------------------------------------------------------------------
def test_csr_shards_sum_to_the_whole(ctx, orc, pkg):
    n, ncol = 20_000, 17_000
    rp, cc, cv = pkg.synth.csr_uniform(0, n, ncol, 11, seed=21)
    rp64 = rp.astype(np.int64)
    x, _ = _xy(n, ncol, 22)
    total = np.zeros(ncol)
    for b, e in ((0, 7_001), (7_001, 7_002), (7_002, n)):
        S = ctx.csr_shard(b, e, ncol, rp64, cc, cv)
        srp = ol.csr_shard_row_ptr(orc, rp, b, e)
        scc, scv = np.ascontiguousarray(cc[rp[b]:rp[e]]), np.ascontiguousarray(cv[rp[b]:rp[e]])
        dx, dy = ctx.vector_from(x[b:e]), ctx.vector_from(np.zeros(ncol))
        ctx.apply_transpose(S, dx, dy)
        ctx.sync()
        got = dy.download()
        ref = np.zeros(ncol)
        ol.csc_spmv(orc, srp, scc, scv, np.ascontiguousarray(x[b:e]), ref)
        rows = np.repeat(np.arange(e - b, dtype=np.int32), np.diff(srp))
        ol.assert_parity(got, ref, _transposed_scale(orc, e - b, ncol, rows, scc, scv, np.ascontiguousarray(x[b:e])), f"shard [{b},{e})")
        total += got
    whole = np.zeros(ncol)
    ol.csc_spmv(orc, rp, cc, cv, x, whole)
    rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(rp))
    ol.assert_parity(total, whole, _transposed_scale(orc, n, ncol, rows, cc, cv, x), "sum over the shards")


def _handles(ctx, orc, pkg):
    n, ncol = 40_000, 30_000
    rp, cc, cv = pkg.synth.csr_uniform(0, n, ncol, 9, seed=23)
    row = np.repeat(np.arange(n, dtype=np.int32), np.diff(rp))
    cp, cr, ccv = ol.coo_to_csc(orc, ncol, row, cc, cv)
    k, ec, ev = ol.coo_to_ell(orc, n, row, cc, cv)
    return n, ncol, {
        "csr": lambda: ctx.csr(n, ncol, rp, cc, cv),
        "coo": lambda: ctx.coo(n, ncol, row, cc, cv),
        "csc": lambda: ctx.csc(n, ncol, cp, cr, ccv),
        "ell": lambda: ctx.ell(n, ncol, k, len(cv), ec, ev),
    }


def test_transposed_state_leaves_the_forward_state_alone(ctx, orc, pkg):
    n, ncol, makers = _handles(ctx, orc, pkg)
    x, y0 = _xy(ncol, n, 24)  # forward: x has ncol entries, y nrow
    xt, yt0 = _xy(n, ncol, 25)
    for fmt, make in makers.items():
        A = make()
        info0, plan0, bytes0 = A.info, A.get_plan(), A.get_param("device_bytes")
        dx, dy = ctx.vector_from(x), ctx.vector_from(y0)
        ctx.apply(A, dx, dy)
        ctx.sync()
        fwd0 = dy.download()
        assert A.get_param("transpose_ready") == 0
        A.transpose_setup()
        A.transpose_setup()  # idempotent
        assert A.get_param("transpose_ready") == 1 and A.get_param("transpose_bytes") >= 0
        # interleaved: forward and transposed products alternate on the same stream
        dxt, dyt = ctx.vector_from(xt), ctx.vector_from(yt0)
        dy2 = ctx.vector_from(y0)
        for _ in range(3):
            ctx.apply(A, dx, dy2)
            ctx.apply_transpose(A, dxt, dyt)
        ctx.sync()
        dyt_alone = ctx.vector_from(yt0)
        for _ in range(3):
            ctx.apply_transpose(A, dxt, dyt_alone)
        dy3 = ctx.vector_from(y0)
        for _ in range(3):
            ctx.apply(A, dx, dy3)
        ctx.sync()
        assert np.array_equal(dy2.download(), dy3.download()), f"{fmt}: forward products interleaved with transposed ones differ"
        assert np.array_equal(dyt.download(), dyt_alone.download()), f"{fmt}: transposed products interleaved with forward ones differ"
        dy4 = ctx.vector_from(y0)
        ctx.apply(A, dx, dy4)
        ctx.sync()
        assert np.array_equal(dy4.download(), fwd0), f"{fmt}: the forward result moved"
        info1 = A.info
        assert (info1.kernel, info1.device_bytes) == (info0.kernel, info0.device_bytes), fmt
        assert A.get_param("device_bytes") == bytes0, fmt
        assert A.get_plan() == plan0, f"{fmt}: the transposed state changed the plan"


def test_empty_and_degenerate_handles(ctx, orc):
    # nnz = 0: y unchanged
    A = ctx.csr(5, 7, np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0))
    y0 = np.arange(7, dtype=np.float64)
    dx, dy = ctx.vector_from(np.ones(5)), ctx.vector_from(y0)
    ctx.apply_transpose(A, dx, dy)
    ctx.sync()
    assert np.array_equal(dy.download(), y0)
    # nrow = 0 (x empty): y unchanged
    B = ctx.csr(0, 4, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    dy = ctx.vector_from(np.ones(4))
    ctx.apply_transpose(B, ctx.vector(0), dy)
    ctx.sync()
    assert np.array_equal(dy.download(), np.ones(4))
    for M in (ctx.coo(5, 7, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0)), ctx.dia(5, 7, np.zeros(0, np.int32), np.zeros(0))):
        dy = ctx.vector_from(y0)
        ctx.apply_transpose(M, ctx.vector_from(np.ones(5)), dy)
        ctx.sync()
        assert np.array_equal(dy.download(), y0)
    # wrong lengths
    with pytest.raises(Exception, match="x has"):
        ctx.apply_transpose(A, ctx.vector(7), ctx.vector(7))


def test_released_csr_arrays_are_refused(ctx, pkg):
    n = 50_000
    rp, cc, cv = pkg.synth.csr_uniform(0, n, n, 8, seed=26)
    A = ctx.csr(n, n, rp, cc, cv)
    A.set_kernel(PANEL)
    A.transpose_setup()
    assert A.get_param("transpose_ready") == 1
    A.set_param("panel_keep_csr", 0)
    assert A.get_param("transpose_ready") == 0  # (the companion read the arrays just released)
    with pytest.raises(Exception, match="panel_keep_csr"):
        ctx.apply_transpose(A, ctx.vector(n), ctx.vector(n))
    with pytest.raises(Exception, match="panel_keep_csr"):
        A.transpose_setup()
    dx, dy = ctx.vector_from(np.ones(n)), ctx.vector_from(np.zeros(n))
    ctx.apply(A, dx, dy)  # the forward product still runs
    ctx.sync()


def test_transpose_kernel_parameter_checks(ctx, orc):
    rp = np.array([0, 1, 2], np.int32)
    A = ctx.csr(2, 2, rp, np.array([1, 0], np.int32), np.array([2.0, 3.0]))
    with pytest.raises(Exception, match="transpose_kernel"):
        A.set_param("transpose_kernel", SCALAR)  # a CSC companion has no scalar kernel
    A.set_param("transpose_kernel", VECTOR)
    assert A.get_param("transpose_kernel") == VECTOR
    A.transpose_setup()
    assert A.get_param("transpose_kernel") == VECTOR
    A.set_param("transpose_kernel", PANEL)  # a new request drops the state built under the old one
    assert A.get_param("transpose_ready") == 0
    dy = ctx.vector_from(np.zeros(2))
    ctx.apply_transpose(A, ctx.vector_from(np.array([1.0, 10.0])), dy)
    ctx.sync()
    assert np.array_equal(dy.download(), np.array([30.0, 2.0]))
    assert A.get_param("transpose_kernel") == PANEL


# ---- full size ----------------------------------------------------------------------------------------------------------------
def test_full_size_c2_transposed_against_the_scatter(ctx):
    """10M x 10M, 32 uniform entries per row: the transposed product under AUTO against the CSC companion's scatter"""
    n = 10_000_000
    A = ctx.gen_csr_uniform(0, n, n, 32, 0, seed=2)
    x = ctx.gen_vector(n, seed=3)
    y = ctx.vector(n)
    y.fill(0.0)
    ctx.apply_transpose(A, x, y)
    ctx.sync()
    got = y.download()
    t_tr = ctx.apply_transpose_timed(A, x, y, 20)
    t_fwd = ctx.apply_timed(A, x, y, 20)
    auto_kernel = A.get_param("transpose_kernel")
    A.set_param("transpose_kernel", VECTOR)
    y.fill(0.0)
    ctx.apply_transpose(A, x, y)
    ctx.sync()
    ref = y.download()
    rel = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
    assert rel <= ol.REL_TOL, f"C2 transposed (companion kernel {auto_kernel}) against the scatter: {rel:.3e}"
    perf_expect(t_tr <= 1.25 * t_fwd, f"C2 transposed {t_tr:.3f} ms > 1.25 x forward {t_fwd:.3f} ms (companion kernel {auto_kernel})")


def test_full_size_dia_band_transposed_is_bitwise_on_samples(ctx, orc):
    """the 4M x 64 DIA band: sampled outputs (both ends included) bit-identical to the (j, d) order"""
    n, nd = 4_000_000, 64
    A = ctx.gen_dia_banded(n, nd, seed=5)
    offsets, _, dval = A.download()
    x = ctx.gen_vector(n, seed=6)
    xh = x.download()
    y0 = np.random.default_rng(7).uniform(-1, 1, size=n)
    y = ctx.vector_from(y0)
    ctx.apply_transpose(A, x, y)
    ctx.sync()
    got = y.download()
    rng = np.random.default_rng(8)
    js = np.unique(np.concatenate([np.arange(80), np.arange(n - 80, n), rng.integers(0, n, size=4000)]))
    J, i, v = _dia_entries_jd(n, n, ol.i32(offsets), dval, js=js)
    pos = ol.i32(np.searchsorted(js, J))  # output j -> its place in the sample
    ref = y0[js].copy()
    ol.coo_spmv(orc, pos, ol.i32(i), ol.f64(v), xh, ref, fma=True)
    assert np.array_equal(got[js], ref)
    t_tr = ctx.apply_transpose_timed(A, x, y, 20)
    t_fwd = ctx.apply_timed(A, x, y, 20)
    perf_expect(t_tr <= 1.25 * t_fwd, f"DIA 4M x 64 transposed {t_tr:.3f} ms > 1.25 x forward {t_fwd:.3f} ms")


# ---- torch ---------------------------------------------------------------------------------------------------------------------
def _torch_child(case):
    """tests/child_transpose_torch.py in a fresh process: torch initialises its HIP runtime before the engine's library is loaded"""
    import subprocess
    import sys
    from pathlib import Path

    child = Path(__file__).with_name("child_transpose_torch.py")
    r = subprocess.run([sys.executable, str(child), case], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"TRANSPOSE_TORCH_OK {case}" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])


def test_torch_gradcheck_of_the_sparse_product():
    _torch_child("gradcheck")


def test_torch_rmatvec_on_a_csc_handle():
    _torch_child("rmatvec")
