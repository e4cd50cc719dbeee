"""Aggregation AMG on the GPU where tests/test_gpu_amg.py does not go: the application on irregular hierarchies (one aggregate of 300
rows, aggregates of 70, line aggregates, a stalled 16-row coarsest level), matrices as untidy as CSR allows (duplicates, unsorted
columns, stored zeros, a split diagonal, theta > 0 on a nonsymmetric pattern), every kernel id forced on the coarse handles, a forced
id that a coarse operator cannot run, the dense / Chebyshev switch at 1024 rows, several states on one handle, a context's plan.

The twin is tests/amg_ref.py; tests/test_amg_ref.py holds it, on the CPU, to P^T A P in int64 on the same fuzz systems and holds
every application compared here to five mutations of the method, each of which moves it by more than the gate below.  Hierarchies
are compared exactly, applications within oracle_lib.REL_TOL (test_gpu_amg._close)."""
import numpy as np
import pytest

import amg_ref as ar
import chebyshev_ref as cr
import exact
import oracle_lib as ol
from test_gpu_amg import _apply, _close

pytestmark = pytest.mark.gpu

UNSUPPORTED = -5
KERNEL_NAMES = ("AUTO", "VECTOR", "LDSWIN", "SCALAR", "PANEL", "TWOPHASE", "SEGSCAN", "SPLIT", "ELL")
PLAIN_STORE = (1, 2, 3, 4, 5, 8)  # VECTOR, LDSWIN, SCALAR, PANEL, TWOPHASE, ELL: their kernels touch every y_i once (adds_into_y_with_atomics)
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _system(name):
    return _once(("system", name), ar.EDGE_CASES[name][0])


def _twin(name):
    return _once(("twin", name), lambda: ar.Hierarchy(*_system(name), **ar.EDGE_CASES[name][1]))


def _setup_args(name):
    kw = dict(ar.EDGE_CASES[name][1])
    kw.pop("level0_smoother", None)
    return kw


def _rhs(name):
    return _once(("r", name), lambda: ar.edge_rhs(name, _system(name)[0]))


def _want(name):
    return _once(("want", name), lambda: _twin(name).apply(_rhs(name)))


def _hierarchy_bytes(ctx, A):
    """every array of every level, as spmv_amg_level returns them"""
    return [tuple(None if a is None else np.ascontiguousarray(a).tobytes() for a in ctx.amg_level(A, l)) for l in range(ctx.amg_info(A)[0])]


def _check_hierarchy(ctx, A, H, what):
    """counts, rounds and launches; on every level aggregates, row pointers and columns equal the twin's, values equal its bytes"""
    levels, rows, nnz = ctx.amg_info(A)
    assert levels == len(H.levels) == A.get_param("amg_levels") and list(rows) == H.rows and list(nnz) == H.nnz, (what, list(rows), H.rows)
    assert A.get_param("amg_mis_rounds") == H.mis_rounds and A.get_param("amg_ready") == 1 and A.get_param("amg_launches") == H.launches(), what
    for l, L in enumerate(H.levels):
        agg, rp, cc, cv = ctx.amg_level(A, l)
        if l + 1 < levels:
            assert np.array_equal(agg, L.agg), (what, l)
        else:
            assert agg is None
        assert np.array_equal(rp, L.rp) and np.array_equal(cc, L.cc), (what, l)
        assert cv.tobytes() == L.cv.tobytes(), (what, l)


def _state(A):
    return [A.get_param(p) for p in ("amg_ready", "amg_levels", "amg_bytes", "amg_launches", "amg_mis_rounds", "cheby_bytes", "device_bytes")]


# ---- 1. the application on the irregular hierarchies -------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ("default", "degree1"))
@pytest.mark.parametrize("name", ar.IRREGULAR)
def test_application_matches_the_twin_on_irregular_hierarchies(ctx, name, config):
    case = name if config == "default" else name + "_degree1"
    n, rp, cc, cv = _system(case)
    A = ctx.csr(n, n, rp, cc, cv)
    ctx.amg_setup(A, **_setup_args(case))
    H = _twin(case)
    _check_hierarchy(ctx, A, H, case)
    sizes = [int(np.bincount(L.agg).max()) for L in H.levels[:-1]]
    for aligned in (True, False):
        _close(_apply(ctx, A, _rhs(case), aligned), _want(case), f"{case}: rows {H.rows}, largest aggregates {sizes}, aligned {aligned}")


# ---- 2. fuzz: duplicates, unsorted columns, stored zeros, split diagonals, theta > 0 on nonsymmetric patterns ----------------------
@pytest.mark.parametrize("seed", ar.FUZZ_SEEDS)
def test_fuzz_hierarchy_and_application(ctx, seed):
    case = f"fuzz{seed:02d}"
    n, rp, cc, cv = _system(case)
    A = ctx.csr(n, n, rp, cc, cv)
    ctx.amg_setup(A, **_setup_args(case))
    H = _twin(case)
    _check_hierarchy(ctx, A, H, case)
    # the values once more, against P^T A P in int64 of the level above as the DEVICE returned it
    for l in range(len(H.levels) - 1):
        agg, rp_l, cc_l, cv_l = ctx.amg_level(A, l)
        _, rp_c, cc_c, cv_c = ctx.amg_level(A, l + 1)
        want, stored = ar.galerkin_int64(len(rp_l) - 1, rp_l, cc_l, cv_l, agg, len(rp_c) - 1)
        rows = np.repeat(np.arange(len(rp_c) - 1), np.diff(rp_c))
        assert np.array_equal(exact.scaled(cv_c, ar.FUZZ_E), want[rows, cc_c]) and int(stored.sum()) == len(cc_c) and stored[rows, cc_c].all(), (case, l)
    print(f"{case}: n {n}, {len(cc)} entries, {_setup_args(case)}, rows {H.rows}")
    _close(_apply(ctx, A, _rhs(case)), _want(case), f"{case}: rows {H.rows}")


# ---- 3. every kernel id forced on the coarse handles ---------------------------------------------------------------------------------
def _plain_products(ctx, pkg, H, kernel):
    """the project's own product as the oracle of what a coarse handle can run: a plain CSR handle of every coarse level from the
    twin's arrays, set_kernel(kernel), one product.  Returns the error code of the first level that refuses (None: all ran) and a
    line per level"""
    lines, refused = [], None
    for l, L in enumerate(H.levels[1:], start=1):
        x_host = np.random.default_rng(50 + l).uniform(-1, 1, L.n)
        try:
            C = ctx.csr(L.n, L.n, L.rp, L.cc, L.cv)
            C.set_kernel(kernel)
            x, y = ctx.vector_from(x_host), ctx.vector(L.n)
            y.fill(0.0)
            ctx.apply(C, x, y)
            ctx.sync()
        except pkg.capi.SpmvError as e:
            lines.append(f"level {l} ({L.n} rows, {L.nnz} entries): refused, code {e.code}: {e}")
            refused = e.code if refused is None else refused
            continue
        want = L.mv(x_host)
        err = np.max(np.abs(y.download() - want)) / max(np.max(np.abs(want)), 1e-300)
        assert err <= ol.REL_TOL, (kernel, l, err)
        lines.append(f"level {l} ({L.n} rows, {L.nnz} entries): ran")
    return refused, lines


@pytest.mark.parametrize("kernel", range(1, 9), ids=KERNEL_NAMES[1:])
@pytest.mark.parametrize("name", ("laplacian32x32", "arrow300", "nonsymmetric500", "anisotropic16x16_quarter"))
def test_every_forced_level_kernel(ctx, pkg, name, kernel):
    capi = pkg.capi
    n, rp, cc, cv = _system(name)
    H, r_host, want = _twin(name), _rhs(name), _want(name)
    refused, lines = _plain_products(ctx, pkg, H, kernel)
    print(f"{name}, {KERNEL_NAMES[kernel]}: " + "; ".join(lines))
    A = ctx.csr(n, n, rp, cc, cv)
    A.set_kernel(capi.CSR_VECTOR)  # (level 0 runs the handle's own kernel: a fixed tree per row)
    ctx.amg_setup(A, **_setup_args(name))
    auto, z_auto, before = _hierarchy_bytes(ctx, A), _apply(ctx, A, r_host), _state(A)
    _close(z_auto, want, f"{name}, AUTO on the coarse handles")
    A.set_param("amg_level_kernel", kernel)
    if refused is not None:  # what a plain handle refuses, the set-up refuses, and leaves everything as it was
        with pytest.raises(capi.SpmvError) as e:
            ctx.amg_setup(A, **_setup_args(name))
        assert e.value.code == refused, (e.value.code, refused, str(e.value))
        assert _state(A) == before and _apply(ctx, A, r_host).tobytes() == z_auto.tobytes()
        return
    out = []
    for _ in range(2):
        ctx.amg_setup(A, **_setup_args(name))
        assert _hierarchy_bytes(ctx, A) == auto, "the hierarchy does not depend on the kernel of the coarse handles"
        assert A.get_param("amg_launches") == H.launches()
        for _ in range(2):
            z = _apply(ctx, A, r_host)
            _close(z, want, f"{name}, {KERNEL_NAMES[kernel]} on the coarse handles")
            out.append(z.tobytes())
    if kernel in PLAIN_STORE:
        assert len(set(out)) == 1, "two set-ups and two applications give the same bits"


# ---- 4. a forced id that a coarse operator cannot run ---------------------------------------------------------------------------------
def test_a_forced_lds_window_wider_than_the_tile_fails_the_setup(ctx, pkg):
    """the periodic tridiagonal matrix of 100,000 rows coarsens to 27,529 rows whose first block of 256 spans every column: the
    LDS-window kernel's tile holds 16,384.  The set-up says so, and no application fails in the middle of a cycle"""
    capi = pkg.capi
    name = "periodic100000"
    n, rp, cc, cv = _system(name)
    H, r_host, want = _twin(name), _rhs(name), _want(name)
    assert H.rows == [100000, 27529, 7601, 2091, 574, 154]
    A = ctx.csr(n, n, rp, cc, cv)
    ctx.amg_setup(A)
    _check_hierarchy(ctx, A, H, name)
    z_auto, before = _apply(ctx, A, r_host), _state(A)
    _close(z_auto, want, f"{name}, AUTO")
    A.set_param("amg_level_kernel", capi.CSR_LDSWIN)
    with pytest.raises(capi.SpmvError) as e:
        ctx.amg_setup(A)
    print("refused:", e.value)
    assert e.value.code == UNSUPPORTED and all(word in str(e.value) for word in ("level 1", "amg_level_kernel=2", "27529", "16384")), str(e.value)
    assert _state(A) == before and _apply(ctx, A, r_host).tobytes() == z_auto.tobytes(), "the earlier state still applies"
    # a solver meets the same state: no step fails half way through a cycle
    b, x = ctx.vector_from(r_host), ctx.vector(n)
    x.fill(0.0)
    iters, res = ctx.cg(A, b, x, max_iter=200, rel_tol=ar.REL_TOL, precond=capi.PRECOND_AMG)
    assert res <= ar.REL_TOL, (iters, res)
    A.set_param("amg_level_kernel", capi.CSR_VECTOR)
    ctx.amg_setup(A)
    _check_hierarchy(ctx, A, H, name)
    _close(_apply(ctx, A, r_host), want, f"{name}, VECTOR")


# ---- 5. the dense / Chebyshev switch of the coarsest level ------------------------------------------------------------------------------
def test_1024_rows_are_inverted_and_1025_are_smoothed(ctx):
    for name, n in (("tridiagonal1024", 1024), ("tridiagonal1025", 1025)):
        _, rp, cc, cv = _system(name)
        A = ctx.csr(n, n, rp, cc, cv)
        ctx.amg_setup(A, max_levels=1)
        assert ctx.amg_info(A)[0] == 1
        r_host = _rhs(name)
        if n == 1024:
            assert A.get_param("amg_launches") == 1 and A.get_param("cheby_ready") == 0
            want = np.linalg.solve(ar.dense_of(n, rp, cc, cv), r_host)
        else:
            d = A.get_param("cheby_degree")
            assert d == 2 and A.get_param("amg_launches") == 2 * d + 1
            H = _twin(name)
            assert H.inv is None and H.launches() == 2 * d + 1
            want = H.apply(r_host)
        for aligned in (True, False):
            _close(_apply(ctx, A, r_host, aligned), want, f"{n} rows, one level, aligned {aligned}")


# ---- 6. several states on one handle ---------------------------------------------------------------------------------------------------
def test_the_cycle_among_the_other_states_of_its_handle(ctx, pkg):
    capi = pkg.capi
    name = "laplacian32x32"
    n, rp, cc, cv = _system(name)
    r_host = _rhs(name)
    A = ctx.csr(n, n, rp, cc, cv)
    bare = A.get_param("device_bytes")
    ctx.amg_setup(A, coarse_max=8)
    z0 = _apply(ctx, A, r_host)
    _close(z0, _want(name), name)
    launches = A.get_param("amg_launches")
    # the ILU(0) factors, the transposed state, another kernel and back, the handle's own plan: none of them is the cycle's
    b, x = ctx.vector_from(r_host), ctx.vector(n)
    x.fill(0.0)
    assert ctx.cg(A, b, x, max_iter=500, rel_tol=ar.REL_TOL, precond=capi.PRECOND_ILU0)[1] <= ar.REL_TOL
    A.transpose_setup()
    y = ctx.vector(n)
    y.fill(0.0)
    ctx.apply_transpose(A, b, y)
    ctx.sync()
    _close(y.download(), _twin(name).levels[0].mv(r_host), "the transposed product of the symmetric matrix")
    kernel = A.info.kernel
    A.set_kernel(capi.CSR_SCALAR)
    assert A.info.kernel == capi.CSR_SCALAR
    A.set_kernel(kernel)
    A.set_plan(A.get_plan())
    assert A.info.kernel == kernel
    assert _apply(ctx, A, r_host).tobytes() == z0.tobytes(), "the cycle after the other states were built"
    parts = {p: A.get_param(p) for p in ("amg_bytes", "cheby_bytes", "ilu0_bytes", "transpose_bytes")}
    print(f"device_bytes {A.get_param('device_bytes')}, the bare handle {bare}, {parts}")
    assert all(parts[p] > 0 for p in ("amg_bytes", "cheby_bytes", "ilu0_bytes")) and A.get_param("transpose_ready") == 1
    # (the transposed state is never counted in device_bytes - include/spmv_abi.h, spmv_mat_transpose_setup - and a CSR handle's
    # companion borrows its arrays: transpose_bytes may be 0)
    assert A.get_param("device_bytes") == bare + parts["amg_bytes"] + parts["cheby_bytes"] + parts["ilu0_bytes"] == A.info.device_bytes
    # level 0's smoother IS the handle's Chebyshev state: a later set-up of it changes the cycle, and the cycle alone
    lmin, lmax = cr.laplacian_2d_bounds(32)
    ctx.chebyshev_setup(A, 3, scaled=False, lmin=lmin, lmax=lmax)
    assert A.get_param("amg_launches") == launches + 4 and A.get_param("amg_ready") == 1
    G = _twin("laplacian32x32_unscaled3")
    assert G.launches() == launches + 4
    changed = G.apply(r_host)  # (the same right-hand side as before)
    for aligned in (True, False):
        _close(_apply(ctx, A, r_host, aligned), changed, f"{name} under an unscaled level-0 smoother of degree 3, aligned {aligned}")
    assert np.max(np.abs(changed - _want(name))) > ol.REL_TOL * np.max(np.abs(_want(name))), "the two cycles differ"
    x.fill(0.0)
    iters, res = ctx.cg(A, b, x, max_iter=500, rel_tol=ar.REL_TOL, precond=capi.PRECOND_AMG)
    LD = np.longdouble
    rows = np.repeat(np.arange(n), np.diff(rp))
    ax = np.zeros(n, dtype=LD)
    np.add.at(ax, rows, cv.astype(LD) * x.download().astype(LD)[cc])
    true = float(np.sqrt(np.sum((r_host.astype(LD) - ax) ** 2)) / np.sqrt(np.sum(r_host.astype(LD) ** 2)))
    print(f"CG under the changed cycle: {iters} iterations, reported {res:.3e}, true {true:.3e}")
    assert res <= ar.REL_TOL and true <= ar.REL_TOL
    assert ctx.chebyshev_info(A) == (3, False, lmin, lmax)
    x.fill(0.0)
    assert ctx.cg(A, b, x, max_iter=2000, rel_tol=ar.REL_TOL, precond=capi.PRECOND_CHEBYSHEV)[1] <= ar.REL_TOL
    assert ctx.chebyshev_info(A) == (3, False, lmin, lmax), "a solver uses the state as it stands"
    assert A.get_param("amg_ready") == 1 and A.get_param("amg_launches") == launches + 4


# ---- 7. a context's plan is for the handles the caller creates ----------------------------------------------------------------------
def test_a_context_plan_does_not_reach_the_coarse_handles(ctx, pkg):
    capi = pkg.capi
    name = "laplacian32x32"
    n, rp, cc, cv = _system(name)
    A = ctx.csr(n, n, rp, cc, cv)
    S = ctx.csr(n, n, rp, cc, cv)
    S.set_kernel(capi.CSR_SCALAR)
    ctx.set_plan(S.get_plan())
    try:
        ctx.amg_setup(A, coarse_max=8)
        _check_hierarchy(ctx, A, _twin(name), name)
        _close(_apply(ctx, A, _rhs(name)), _want(name), f"{name} under a context plan")
        T = ctx.csr(n, n, rp, cc, cv)  # the plan is still there for the handle it was meant for
        assert T.info.kernel == capi.CSR_SCALAR
    finally:
        ctx.set_plan(None)
    assert ctx.csr(n, n, rp, cc, cv).info.kernel == A.info.kernel
