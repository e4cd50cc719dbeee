"""The multi-vector product Y += A*X (spmv_apply_multi) on the GPU.

X (ncol, k) and Y (nrow, k) are row-major.  The contract is bit-identity: column c of Y equals the oracle's fma flavour applied
to column c of X (CSR: orc_csr_spmv_fma, ELL: orc_ell_spmv_fma), after one call and after 50 accumulating calls, so every
comparison here is np.array_equal / torch.equal, never a tolerance.
"""
import numpy as np
import pytest

import cases
import oracle_lib as ol
from conftest import perf_expect

pytestmark = pytest.mark.gpu
NUM_TEST = 50
KS = (1, 2, 3, 4, 5, 8, 13, 16, 17, 32, 64)


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


def _xy(nrow, ncol, k, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 1.0, size=(ncol, k))
    Y0 = rng.uniform(0.5, 1.5, size=(nrow, k)) * np.where(rng.random((nrow, k)) < 0.5, -1.0, 1.0)
    return X, Y0


def _oracle_columns(spmv, X, Y0, reps, overwrite):
    """column by column: `spmv(x, y)` (y += A x in the oracle's fma order) repeated `reps` times from Y0 (from 0 with overwrite)"""
    Y = np.empty_like(Y0)
    for c in range(X.shape[1]):
        x = np.ascontiguousarray(X[:, c])
        y = np.zeros(Y0.shape[0]) if overwrite else Y0[:, c].copy()
        for _ in range(1 if overwrite else reps):  # y = A x repeated is y = A x once
            spmv(x, y)
        Y[:, c] = y
    return Y


def _engine(ctx, A, X, Y0, k, overwrite):
    """Y after 1 and after NUM_TEST calls of apply_multi"""
    dX = ctx.vector_from(X.ravel())
    dY = ctx.vector_from(Y0.ravel())
    ctx.apply_multi(A, dX, dY, k, overwrite=overwrite)
    ctx.sync()
    y1 = dY.download().reshape(Y0.shape)
    for _ in range(NUM_TEST - 1):
        ctx.apply_multi(A, dX, dY, k, overwrite=overwrite)
    ctx.sync()
    return y1, dY.download().reshape(Y0.shape)


def _check(ctx, A, spmv, nrow, ncol, k, seed, what, X=None, equal_nan=False):
    Xr, Y0 = _xy(nrow, ncol, k, seed)
    X = Xr if X is None else X
    for overwrite in (False, True):
        y1, y50 = _engine(ctx, A, X, Y0, k, overwrite)
        r1 = _oracle_columns(spmv, X, Y0, 1, overwrite)
        r50 = _oracle_columns(spmv, X, Y0, NUM_TEST, overwrite)
        assert np.array_equal(y1, r1, equal_nan=equal_nan), f"{what} k={k} overwrite={overwrite}: 1 call"
        assert np.array_equal(y50, r50, equal_nan=equal_nan), f"{what} k={k} overwrite={overwrite}: {NUM_TEST} calls"


@pytest.mark.parametrize("fx", FIXTURES, ids=lambda f: f[0])
def test_csr_multi_is_bitwise_oracle_fma_per_column(ctx, orc, fx):
    name, nrow, ncol, row, col, val = fx
    rp, cc, cv = ol.coo_to_csr(orc, nrow, row, col, val)
    A = ctx.csr(nrow, ncol, rp, cc, cv)
    spmv = lambda x, y: ol.csr_spmv(orc, rp, cc, cv, x, y, fma=True)  # noqa: E731
    for k in KS:
        _check(ctx, A, spmv, nrow, ncol, k, seed=k, what=f"{name} csr")


@pytest.mark.parametrize("fx", FIXTURES, ids=lambda f: f[0])
def test_ell_multi_is_bitwise_oracle_fma_per_column(ctx, orc, fx):
    name, nrow, ncol, row, col, val = fx
    slots, ec, ev = ol.coo_to_ell(orc, nrow, row, col, val)
    A = ctx.ell(nrow, ncol, slots, len(val), ec, ev)
    spmv = lambda x, y: ol.ell_spmv(orc, nrow, slots, ec, ev, x, y, fma=True)  # noqa: E731
    for k in KS:
        _check(ctx, A, spmv, nrow, ncol, k, seed=100 + k, what=f"{name} ell")
    # padding slots contribute 0.0 * X[0, c]: inf and NaN in X's first row reach every padded row as NaN, as in the oracle
    for k in (3, 8, 17):
        X, _ = _xy(nrow, ncol, k, seed=200 + k)
        X[0, :] = np.where(np.arange(k) % 2 == 0, np.inf, np.nan)
        _check(ctx, A, spmv, nrow, ncol, k, seed=200 + k, what=f"{name} ell non-finite X[0]", X=X, equal_nan=True)


def _band_with_long_row(n=20_000, half=4, long_row=137, long_len=8192, seed=5):
    """a band of 2 * half + 1 diagonals and one row of long_len entries: most CSR kernels accept it (SPLIT for the long row)"""
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.int64)
    r = [np.repeat(i, 2 * half + 1), np.full(long_len, long_row, np.int64)]
    c = [(i[:, None] + np.arange(-half, half + 1)[None, :]).ravel(), rng.choice(n, long_len, replace=False).astype(np.int64)]
    r, c = np.concatenate(r), np.concatenate(c)
    keep = (c >= 0) & (c < n)
    key = np.unique(r[keep] * n + c[keep])  # row-major order, no duplicates
    r, c = key // n, (key % n).astype(np.int32)
    rp = np.searchsorted(r, np.arange(n + 1)).astype(np.int32)
    return n, rp, c, rng.uniform(-1.0, 1.0, c.size)


def test_multi_ignores_the_kernel_and_the_plan_of_the_handle(ctx, orc, pkg):
    """whatever kernel the handle runs for spmv_apply, apply_multi reads its own arrays: the same bits every time, the oracle's,
    and the handle's plan is byte-identical before and after"""
    capi = pkg.capi
    n, rp, cc, cv = _band_with_long_row()
    k = 8
    X, Y0 = _xy(n, n, k, seed=3)
    ref = _oracle_columns(lambda x, y: ol.csr_spmv(orc, rp, cc, cv, x, y, fma=True), X, Y0, 1, False)
    A = ctx.csr(n, n, rp, cc, cv)
    dX = ctx.vector_from(X.ravel())
    accepted = []
    for kernel in (capi.CSR_AUTO, capi.CSR_VECTOR, capi.CSR_SCALAR, capi.CSR_PANEL, capi.CSR_TWOPHASE, capi.CSR_SPLIT, capi.CSR_ELL):
        if kernel != capi.CSR_AUTO:
            try:
                A.set_kernel(kernel)
            except capi.SpmvError:
                continue
        accepted.append(kernel)
        plan = A.get_plan()
        dY = ctx.vector_from(Y0.ravel())
        ctx.apply_multi(A, dX, dY, k)
        ctx.sync()
        assert np.array_equal(dY.download().reshape(n, k), ref), f"kernel {kernel}"
        assert A.get_plan() == plan, f"kernel {kernel}: apply_multi changed the plan"
    assert len(accepted) >= 5, accepted


def _torch_child(case):
    """tests/child_spmm_torch.py in a fresh process: torch must initialise its HIP runtime BEFORE the engine's library is loaded
    (as bench.py does), and this process has long loaded the engine"""
    import subprocess
    import sys
    from pathlib import Path

    child = Path(__file__).with_name("child_spmm_torch.py")
    r = subprocess.run([sys.executable, str(child), case], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"SPMM_TORCH_OK {case}" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])


def test_shards_and_wrapped_handles_with_torch_tensors():
    """a csr_upload_shard handle and a wrap_csr handle over torch tensors, X / Y wrapped (n, k) torch tensors: the bits of the
    uploaded whole matrix's rows (and of the oracle)"""
    _torch_child("wrapped")


def test_full_size_c2_k8_equals_the_scalar_kernel_per_column():
    """10M x 10M, 32 uniform entries per row, k = 8: every column of Y equals spmv_apply with the SCALAR kernel on that column
    (on the device, whole vectors)"""
    _torch_child("c2")


def test_x_offsets_past_2_to_the_31(ctx, orc, pkg):
    """ncol = 34M and k = 64: X holds 2.18e9 entries (17.4 GB), filled on the device; entries in the last columns"""
    synth = pkg.synth
    ncol, k, nrow, per_row, seed = 34_000_000, 64, 3_000, 6, 9
    rng = np.random.default_rng(1)
    cols = np.concatenate([ncol - 1 - np.arange(200), rng.integers(0, ncol, 100)])  # the last 200 columns and a few others
    col = np.stack([np.sort(rng.choice(cols, per_row, replace=False)) for _ in range(nrow)]).astype(np.int32).ravel()
    val = rng.uniform(-1.0, 1.0, col.size)
    rp = (np.arange(nrow + 1) * per_row).astype(np.int32)
    A = ctx.csr(nrow, ncol, rp, col, val)
    X = ctx.gen_vector(ncol * k, seed=seed)  # X[j, c] = U(0,1) of index j * k + c
    Y0 = rng.uniform(-1.0, 1.0, (nrow, k))
    dY = ctx.vector_from(Y0.ravel())
    ctx.apply_multi(A, X, dY, k)
    ctx.sync()
    got = dY.download().reshape(nrow, k)
    # host oracle over the distinct columns only (their rows of X from the generator's numpy twin)
    uniq, local = np.unique(col, return_inverse=True)
    Xs = np.stack([synth.vec_uniform(k, int(j) * k, seed) for j in uniq])
    assert np.array_equal(Xs[-1], X.download(int(uniq[-1]) * k, k))  # the twin is the device generator
    ref = _oracle_columns(lambda x, y: ol.csr_spmv(orc, rp, local.astype(np.int32), val, x, y, fma=True), Xs, Y0, 1, False)
    assert np.array_equal(got, ref)


def test_errors_leave_the_context_working(ctx, orc, pkg):
    capi = pkg.capi
    c = cases.tri8()
    n = c["nrow"]
    rp, cc, cv = ol.coo_to_csr(orc, n, ol.i32(c["row"]), ol.i32(c["col"]), ol.f64(c["val"]))
    A = ctx.csr(n, n, rp, cc, cv)
    k = 4
    X, Y0 = _xy(n, n, k, seed=1)
    ref = _oracle_columns(lambda x, y: ol.csr_spmv(orc, rp, cc, cv, x, y, fma=True), X, Y0, 1, False)
    dX = ctx.vector_from(X.ravel())

    def good_call():
        dY = ctx.vector_from(Y0.ravel())
        ctx.apply_multi(A, dX, dY, k)
        ctx.sync()
        assert np.array_equal(dY.download().reshape(n, k), ref)

    def expect(code, fn):
        with pytest.raises(capi.SpmvError) as e:
            fn()
        assert e.value.code == code and "spmv_apply_multi" in str(e.value), e.value
        good_call()

    dY = ctx.vector_from(Y0.ravel())
    for bad_k in (0, 65, -1):
        expect(-1, lambda: ctx.apply_multi(A, ctx.vector(n * max(bad_k, 0)), ctx.vector(n * max(bad_k, 0)), bad_k))
    expect(-1, lambda: ctx.apply_multi(A, ctx.vector(n * k - 1), dY, k))
    expect(-1, lambda: ctx.apply_multi(A, dX, ctx.vector(n * k + 1), k))
    expect(-1, lambda: ctx.apply_multi(A, dX, dX, k))
    big = ctx.vector(3 * n * k)
    expect(-1, lambda: ctx.apply_multi(A, ctx.wrap_vector(big.device_ptr, n * k), ctx.wrap_vector(big.device_ptr + 8 * 5, n * k), k))
    with pytest.raises(capi.SpmvError) as e:
        ctx.apply_multi_timed(A, dX, dY, k, 0)
    assert e.value.code == -1
    good_call()
    coo = ctx.coo(n, n, c["row"], c["col"], c["val"])
    csc = ctx.csc(n, n, *ol.coo_to_csc(orc, n, ol.i32(c["row"]), ol.i32(c["col"]), ol.f64(c["val"])))
    offsets, dv = ol.csr_to_dia(orc, n, n, rp, cc, cv)
    dia = ctx.dia(n, n, offsets, dv)
    for M in (coo, csc, dia):
        expect(-5, lambda: ctx.apply_multi(M, dX, dY, k))
    # a PANEL handle that released its CSR arrays (panel_keep_csr = 0): nothing left for this product to read, refused on the host
    nb = 1_000_000
    P = ctx.gen_csr_uniform(0, nb, nb, 16, seed=31)
    P.set_kernel(capi.CSR_PANEL)
    P.set_param("panel_keep_csr", 0)
    assert P.get_param("panel_keep_csr") == 0
    PX, PY = ctx.vector(nb * k), ctx.vector(nb * k)
    expect(-1, lambda: ctx.apply_multi(P, PX, PY, k))
    with pytest.raises(capi.SpmvError, match="gave up"):
        ctx.apply_multi_timed(P, PX, PY, k, 1)
    good_call()
    ms = ctx.apply_multi_timed(A, dX, dY, k, 3)
    assert ms > 0.0


@pytest.mark.gpu_perf
@pytest.mark.parametrize("shape", ["band65536_10M", "uniform_1M"])
def test_multi_beats_k_separate_products(ctx, shape):
    """k = 8: one apply_multi takes less time than 8 spmv_apply of the handle's AUTO kernel on 8 vectors"""
    k = 8
    if shape == "band65536_10M":
        n, A = 10_000_000, ctx.gen_csr_uniform(0, 10_000_000, 10_000_000, 32, 65536, seed=3)
    else:
        n, A = 1_000_000, ctx.gen_csr_uniform(0, 1_000_000, 1_000_000, 32, 0, seed=3)
    X = ctx.gen_vector(n * k, seed=4)
    Y = ctx.vector(n * k)
    Y.fill(0.0)
    xs = [ctx.gen_vector(n, seed=10 + c) for c in range(k)]
    ys = [ctx.vector(n) for _ in range(k)]
    for y in ys:
        y.fill(0.0)
    multi, single = [], []
    ctx.apply_multi_timed(A, X, Y, k, 3)
    for x, y in zip(xs, ys):
        ctx.apply_timed(A, x, y, 3)
    for _ in range(5):
        multi.append(ctx.apply_multi_timed(A, X, Y, k, 5))
        single.append(sum(ctx.apply_timed(A, x, y, 5) for x, y in zip(xs, ys)))
    m, s = float(np.median(multi)), float(np.median(single))
    perf_expect(m < s, f"{shape}: apply_multi k={k} {m:.3f} ms, {k} x apply {s:.3f} ms")
