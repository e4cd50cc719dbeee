"""Aggregation AMG on the GPU (spmv_amg_*; SPMV_PRECOND_AMG in spmv_cg, spmv_bicgstab and spmv_gmres) against the NumPy twin
tests/amg_ref.py, which tests/test_amg_ref.py holds to facts of its own on the CPU.

Aggregates and coarse operators are compared exactly (indices equal, values equal bytes: every sum has a defined order of plain
additions); applications within oracle_lib.REL_TOL; iteration counts one either side of the twin's.

Shapes, for the paths of the kernels: n = 1, 2, 3 and 257, diagonal (every row a root: the hierarchy stalls) and tridiagonal; 32 x 32
and 64 x 64 and 12^3 Laplacians; the 40 x 40 upwind convection-diffusion system (nonsymmetric values); an arrow matrix of 300 rows
(one row wider than a wavefront); 500 rows of a structurally nonsymmetric pattern; the anisotropic 16 x 16 stencil at theta = 0.5
(where no coupling is strong) and 0.25 (the x couplings are);
n = 2 kMaxGrid kBlock + 3 = 1,048,579 tridiagonal (the grid-stride loops' second trip and an odd tail)."""
import numpy as np
import pytest

import amg_ref as ar
import chebyshev_ref as cr
import ilu0_ref as ir
import oracle_lib as ol

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
BIG = 2 * 2048 * 256 + 3
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


CASES = {  # name: (builder, set-up arguments)
    "tridiagonal1": (lambda: cr.tridiagonal(1), dict(coarse_max=1)),
    "tridiagonal2": (lambda: cr.tridiagonal(2), dict(coarse_max=1)),
    "tridiagonal3": (lambda: cr.tridiagonal(3), dict(coarse_max=1)),
    "tridiagonal257": (lambda: cr.tridiagonal(257), dict(coarse_max=1)),
    "diagonal1": (lambda: cr.diagonal(np.full(1, 3.0)), dict(coarse_max=1)),
    "diagonal2": (lambda: cr.diagonal(np.linspace(1.0, 2.0, 2)), dict(coarse_max=1)),
    "diagonal3": (lambda: cr.diagonal(np.linspace(1.0, 2.0, 3)), dict(coarse_max=1)),
    "diagonal257": (lambda: cr.diagonal(np.linspace(1.0, 2.0, 257)), dict(coarse_max=1)),
    "laplacian32x32": (lambda: cr.laplacian_2d_csr(32), dict(coarse_max=8)),
    "laplacian64x64": (lambda: cr.laplacian_2d_csr(64), dict()),
    "laplacian12^3": (lambda: ir.laplacian_3d(12), dict(coarse_max=8)),
    "convdiff40": (lambda: ir.convection_diffusion_2d(40), dict(coarse_max=8)),
    "arrow300": (lambda: ar.arrow(300), dict(coarse_max=8)),
    "nonsymmetric500": (lambda: ar.random_nonsymmetric(500), dict(coarse_max=8)),
    "anisotropic16x16": (lambda: ar.anisotropic_2d(16), dict(coarse_max=8, strength=0.5)),  # (1 < 0.25 * 2.02^2: no neighbours, it stalls)
    "anisotropic16x16_quarter": (lambda: ar.anisotropic_2d(16), dict(coarse_max=8, strength=0.25)),  # the x couplings alone: line aggregates
    "tridiagonal_big": (lambda: cr.tridiagonal(BIG), dict()),
}


def _system(name):
    return _once(("system", name), CASES[name][0])


def _twin(name, **extra):
    kw = dict(CASES[name][1], **extra)
    return _once(("twin", name, tuple(sorted(kw.items()))), lambda: ar.Hierarchy(*_system(name), **kw))


def _handle(ctx, name):
    n, rp, cc, cv = _system(name)
    if name == "tridiagonal_big":
        return _once(("handle", name), lambda: ctx.csr(n, n, rp, cc, cv))
    return ctx.csr(n, n, rp, cc, cv)


def _device_vector(ctx, host, aligned):
    """host on the device, 256-byte aligned or 8 bytes past a 16-byte boundary (a wrapped pointer into a vector of n + 1)"""
    n = len(host)
    if aligned:
        v = ctx.vector_from(host)
        assert v.device_ptr % 16 == 0
        return v, None
    base = ctx.vector(n + 1)
    base.fill(0.0)
    v = ctx.wrap_vector(base.device_ptr + 8, n)
    assert (base.device_ptr + 8) % 16 == 8
    v.upload(host)
    return v, base


def _apply(ctx, A, r_host, aligned=True):
    r, keep_r = _device_vector(ctx, r_host, aligned)
    z, keep_z = _device_vector(ctx, np.full(len(r_host), 7.0), aligned)  # (whatever z holds is ignored)
    ctx.amg_solve(A, r, z)
    ctx.sync()
    assert r.download().tobytes() == r_host.tobytes(), "the application wrote into r"
    return z.download()


def _close(got, want, what):
    err = np.max(np.abs(got - want)) / max(np.max(np.abs(want)), 1e-300)
    print(f"{what}: {err:.3e}")
    assert err <= ol.REL_TOL, (what, err)


# ---- 1. aggregates and coarse operators, exactly ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_hierarchy_equals_the_twins(ctx, name):
    A = _handle(ctx, name)
    ctx.amg_setup(A, **CASES[name][1])
    H = _twin(name)
    levels, rows, nnz = ctx.amg_info(A)
    print(f"{name}: rows {rows.tolist()}, entries {nnz.tolist()}, {A.get_param('amg_mis_rounds')} MIS rounds")
    assert levels == len(H.levels) == A.get_param("amg_levels") and list(rows) == H.rows and list(nnz) == H.nnz
    assert A.get_param("amg_mis_rounds") == H.mis_rounds and A.get_param("amg_ready") == 1
    assert A.get_param("amg_launches") == H.launches()
    if name.startswith("diagonal"):
        assert levels == 1, "every row is a root: the hierarchy stalls"
    for l, L in enumerate(H.levels):
        agg, rp, cc, cv = ctx.amg_level(A, l)
        if l + 1 < levels:
            assert np.array_equal(agg, L.agg), (name, l)
        else:
            assert agg is None
        assert np.array_equal(rp, L.rp) and np.array_equal(cc, L.cc), (name, l)
        assert cv.tobytes() == L.cv.tobytes(), (name, l)


# ---- 2. the empty system, a single level, a stalled coarsest level ----------------------------------------------------------------------
def test_an_empty_system(ctx):
    A = ctx.csr(0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    ctx.amg_setup(A)
    levels, rows, nnz = ctx.amg_info(A)
    assert (levels, list(rows), list(nnz)) == (1, [0], [0]) and A.get_param("amg_bytes") == 0 and A.get_param("amg_launches") == 0
    ctx.amg_solve(A, ctx.vector(0), ctx.vector(0))
    ctx.sync()


@pytest.mark.parametrize("aligned", (True, False), ids=["aligned", "narrow"])
def test_a_single_level_is_a_dense_solve(ctx, aligned):
    n, rp, cc, cv = cr.laplacian_2d_csr(14)  # 196 rows <= coarse_max = 256
    A = ctx.csr(n, n, rp, cc, cv)
    ctx.amg_setup(A)
    assert ctx.amg_info(A)[0] == 1 and A.get_param("amg_launches") == 1 and A.get_param("cheby_ready") == 0
    r_host = np.random.default_rng(3).uniform(-1, 1, n)
    _close(_apply(ctx, A, r_host, aligned), np.linalg.solve(ar.dense_of(n, rp, cc, cv), r_host), f"196 rows, aligned {aligned}")


def test_a_stalled_coarsest_level_beyond_the_dense_limit_takes_chebyshev(ctx):
    n, rp, cc, cv = cr.diagonal(np.linspace(1.0, 2.0, 1100))
    A = ctx.csr(n, n, rp, cc, cv)
    ctx.amg_setup(A)
    H = ar.Hierarchy(n, rp, cc, cv)
    assert ctx.amg_info(A)[0] == 1 == len(H.levels) and H.inv is None and A.get_param("amg_launches") == 5 == H.launches()
    assert A.get_param("amg_mis_rounds") == H.mis_rounds == 1
    r_host = np.random.default_rng(4).uniform(-1, 1, n)
    _close(_apply(ctx, A, r_host), H.apply(r_host), "1100 diagonal rows")


# ---- 3. the application against the twin ------------------------------------------------------------------------------------------
CONFIGS = (dict(), dict(smooth_degree=1, overcorrection=1.0), dict(smooth_degree=3, overcorrection=1.5), dict(max_levels=2), dict(coarse_max=1))


@pytest.mark.parametrize("config", range(len(CONFIGS)))
@pytest.mark.parametrize("name", ("laplacian64x64", "laplacian12^3", "convdiff40"))
def test_application_matches_the_twin(ctx, name, config):
    extra = CONFIGS[config]
    n = _system(name)[0]
    A = _handle(ctx, name)
    ctx.amg_setup(A, **dict(CASES[name][1], **extra))
    H = _twin(name, **extra)
    assert list(ctx.amg_info(A)[1]) == H.rows and A.get_param("amg_launches") == H.launches()
    r_host = _once(("r", name), lambda: np.random.default_rng(200 + n).uniform(-1, 1, n))
    want = _once(("want", name, config), lambda: H.apply(r_host))
    for aligned in (True, False):
        _close(_apply(ctx, A, r_host, aligned), want, f"{name} {extra}, rows {H.rows}, aligned {aligned}")


@pytest.mark.parametrize("aligned", (True, False), ids=["aligned", "narrow"])
def test_application_matches_the_twin_beyond_one_trip_of_the_grid(ctx, aligned):
    name = "tridiagonal_big"
    A = _handle(ctx, name)
    if not A.get_param("amg_ready"):
        ctx.amg_setup(A)
    H = _twin(name)
    r_host = _once(("r", name), lambda: np.random.default_rng(7).uniform(-1, 1, BIG))
    want = _once(("want", name), lambda: H.apply(r_host))
    _close(_apply(ctx, A, r_host, aligned), want, f"n = {BIG}, rows {H.rows}, aligned {aligned}")


# ---- 4. determinism, symmetry ----------------------------------------------------------------------------------------------------------
def test_two_setups_and_two_applications_give_the_same_bits(ctx, pkg):
    n, rp, cc, cv = _system("laplacian64x64")
    r_host = np.random.default_rng(29).uniform(-1, 1, n)
    out, operators = [], []
    for _ in range(2):
        A = ctx.csr(n, n, rp, cc, cv)
        A.set_kernel(pkg.capi.CSR_VECTOR)
        A.set_param("amg_level_kernel", pkg.capi.CSR_VECTOR)
        assert A.get_param("amg_level_kernel") == pkg.capi.CSR_VECTOR
        for _ in range(2):
            ctx.amg_setup(A, coarse_max=8)
            out += [_apply(ctx, A, r_host).tobytes(), _apply(ctx, A, r_host).tobytes()]
            operators.append(b"".join(np.ascontiguousarray(a).tobytes() for l in range(ctx.amg_info(A)[0] - 1) for a in ctx.amg_level(A, l)))
    assert len(set(out)) == 1 and len(set(operators)) == 1
    with pytest.raises(pkg.capi.SpmvError):
        A.set_param("amg_level_kernel", 9)


def test_the_cycle_is_symmetric_on_the_device(ctx):
    n, rp, cc, cv = _system("laplacian32x32")
    A = ctx.csr(n, n, rp, cc, cv)
    ctx.amg_setup(A, coarse_max=8)
    rng = np.random.default_rng(31)
    u, v = rng.uniform(0.5, 1.5, n), rng.uniform(0.5, 1.5, n)
    LD = np.longdouble
    ubv, vbu = np.dot(u.astype(LD), _apply(ctx, A, v).astype(LD)), np.dot(v.astype(LD), _apply(ctx, A, u).astype(LD))
    print(f"u.Bv = {float(ubv)!r}, v.Bu = {float(vbu)!r}")
    assert ubv > 0 and abs(ubv - vbu) <= 1e-12 * abs(ubv)


# ---- 5. the solvers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("system", list(ar.SYSTEMS))
def test_preconditioned_solvers_take_the_iterations_of_the_twins(ctx, pkg, system):
    capi = pkg.capi
    solver, n, rp, cc, cv, b_host = ar.solver_system(system)
    A = ctx.csr(n, n, rp, cc, cv)
    b, x = ctx.vector_from(b_host), ctx.vector(n)
    solve = {"cg": ctx.cg, "bicgstab": ctx.bicgstab, "gmres": ctx.gmres}[solver]
    x.fill(0.0)
    assert A.get_param("amg_ready") == 0
    iters, res = solve(A, b, x, max_iter=2000, rel_tol=ar.REL_TOL, precond=capi.PRECOND_AMG)
    # the solver's own set-up: the defaults
    H = _once(("solver twin", n, len(cc), system.split("_")[1]), lambda: ar.Hierarchy(n, rp, cc, cv))
    assert A.get_param("amg_ready") == 1 and list(ctx.amg_info(A)[1]) == H.rows and A.get_param("cheby_degree") == 2
    assert A.get_param("amg_launches") == H.launches()
    LD = np.longdouble
    rows = np.repeat(np.arange(n), np.diff(rp))
    ax = np.zeros(n, dtype=LD)
    np.add.at(ax, rows, cv.astype(LD) * x.download().astype(LD)[cc])
    true = float(np.sqrt(np.sum((b_host.astype(LD) - ax) ** 2)) / np.sqrt(np.sum(b_host.astype(LD) ** 2)))
    twin_iters = ar.run_twin(system)[1]
    print(f"{system}: {iters} iterations (twin {twin_iters}, recorded {ar.TWIN_ITERATIONS[system]}; plain twin "
          f"{ar.UNPRECONDITIONED_ITERATIONS[system]}), reported {res:.3e}, true {true:.3e}")
    assert twin_iters == ar.TWIN_ITERATIONS[system]
    assert abs(iters - twin_iters) <= 1, (iters, twin_iters)
    assert res <= ar.REL_TOL and true <= ar.REL_TOL, (res, true)
    # a handle that was set up explicitly is used as it stands
    ctx.amg_setup(A, smooth_degree=1, overcorrection=1.0)
    x.fill(0.0)
    again, res = solve(A, b, x, max_iter=2000, rel_tol=ar.REL_TOL, precond=capi.PRECOND_AMG)
    print(f"{system}: {again} iterations with degree 1 and no overcorrection")
    assert A.get_param("cheby_degree") == 1 and res <= ar.REL_TOL


def test_cg_multi_refuses_the_preconditioner(ctx, pkg):
    n, rp, cc, cv = _system("laplacian32x32")
    A = ctx.csr(n, n, rp, cc, cv)
    with pytest.raises(pkg.capi.SpmvError) as e:
        ctx.cg_multi(A, ctx.vector(2 * n), ctx.vector(2 * n), 2, precond=pkg.capi.PRECOND_AMG)
    assert e.value.code == UNSUPPORTED and "AMG" in str(e.value)


# ---- 6. accounting ---------------------------------------------------------------------------------------------------------------------
def _neumann_1d(n):
    """the singular 1-D Laplacian with natural boundary rows: every coarse operator keeps the zero row sums exactly"""
    n, rp, cc, cv = cr.tridiagonal(n)
    cv = cv.copy()
    cv[0] = cv[-1] = 1.0
    return n, rp, cc, cv


def test_parameters_device_bytes_and_a_failed_setup(ctx, pkg):
    capi = pkg.capi
    n, rp, cc, cv = _neumann_1d(1100)
    A = ctx.csr(n, n, rp, cc, cv)
    before, plan, kernel = A.get_param("device_bytes"), A.get_plan(), A.info.kernel
    assert [A.get_param(p) for p in ("amg_ready", "amg_levels", "amg_bytes", "amg_launches", "amg_mis_rounds", "amg_level_kernel")] == [0] * 6

    def expect(call, code, word):
        with pytest.raises(capi.SpmvError) as e:
            call()
        assert e.value.code == code and word in str(e.value), (code, word, e.value)

    expect(lambda: ctx.amg_solve(A, ctx.vector(n), ctx.vector(n)), INVALID, "not set up")
    expect(lambda: ctx.amg_info(A), INVALID, "not set up")
    expect(lambda: ctx.amg_level(A, 0), INVALID, "not set up")
    # one level, served by Chebyshev: the singular operator is never inverted
    ctx.amg_setup(A, max_levels=1)
    grown, cheby = A.get_param("amg_bytes"), A.get_param("cheby_bytes")
    assert ctx.amg_info(A)[0] == 1 and A.get_param("amg_launches") == 5 and grown >= 8 * n and cheby >= 8 * 4 * n
    assert A.get_param("device_bytes") == before + grown + cheby and A.info.device_bytes == before + grown + cheby
    r_host = np.random.default_rng(6).uniform(-1, 1, n)
    z = _apply(ctx, A, r_host)
    # a set-up that fails on the device - a singular coarsest operator - leaves all of it as it was
    expect(lambda: ctx.amg_setup(A, smooth_degree=3), INVALID, "singular coarsest operator")
    assert A.get_param("amg_bytes") == grown and A.get_param("device_bytes") == before + grown + cheby and ctx.amg_info(A)[0] == 1
    assert A.get_param("cheby_degree") == 2 and _apply(ctx, A, r_host).tobytes() == z.tobytes()
    assert A.get_plan() == plan and A.info.kernel == kernel
    expect(lambda: ctx.amg_level(A, 1), INVALID, "level=1")
    expect(lambda: ctx.amg_setup(ctx.csr_to_ell(A)), UNSUPPORTED, "CSR")
    zero = ctx.csr(n, n, rp, cc, np.where((np.repeat(np.arange(n), np.diff(rp)) == cc) & (cc == 5), 0.0, cv))
    expect(lambda: ctx.amg_setup(zero, coarse_max=8), INVALID, "diagonal")
    other = capi.Context(0)
    expect(lambda: other.amg_setup(A), INVALID, "context")
    other.close()


def test_destroying_the_handle_frees_everything(ctx):
    """free device memory (hipMemGetInfo) around two handles of 1,048,579 rows with their hierarchies: what the second one took is
    visible while it lives and is back when it is gone (the first pass also grows what the context keeps)"""
    n, rp, cc, cv = _system("tridiagonal_big")
    r = ctx.vector_from(np.ones(n))
    z = ctx.vector(n)
    free = []
    for _ in range(2):
        ctx.sync()
        free.append(ctx.mem_info()[0])
        A = ctx.csr(n, n, rp, cc, cv)
        ctx.amg_setup(A)
        ctx.amg_solve(A, r, z)
        ctx.sync()
        held, inside = A.get_param("device_bytes"), ctx.mem_info()[0]
        assert A.get_param("amg_bytes") >= 8 * n
        del A
    ctx.sync()
    free.append(ctx.mem_info()[0])
    print(f"free device memory around two handles: {free}, inside the second {inside}, its device_bytes {held}")
    assert free[1] - inside >= held // 2 and free[2] >= free[1]
