"""ILU(0) on the GPU (spmv_ilu0_setup / _solve / _factors / _order; SPMV_PRECOND_ILU0 in spmv_cg and spmv_bicgstab) against the
NumPy reference tests/ilu0_ref.py, which tests/test_ilu0_ref.py holds to facts of its own on the CPU.

Problems, each in both sweep orders (0 the matrix's own row order, 1 multicolour); all strictly diagonally dominant or M-matrices,
so ILU(0) exists in any order:
  tridiagonal_8         n = 8: folded runs of one-row levels, the 1-lane solve
  tridiagonal_nonsym    n = 33, nonsymmetric
  laplacian_3d          24^3 = 13,824 rows: two colours of 6,912 rows (single-level launches, the 4-lane solve), 70 levels in row order
  random_pattern        30,000 rows, nonsymmetric pattern, unsorted columns, the diagonal entry stored twice
  lower_triangular      5,000 rows, the lower-triangular cut of such a matrix: U is the diagonal
  band33                4,099 rows, 33 diagonals: 16 entries in either triangle, the 16-lane solve.  (cgls_ref's band4099 has 4099 x
                        4093 entries on 7 diagonals - not square, 3 entries per triangle; this is the square band of 4,099 rows with
                        33 entries per row in its place, values drawn the same way.)
The reference of a (problem, order) is computed once and shared.  test_every_case_ran asserts at the end that every case ran."""
import gc
from collections import defaultdict

import numpy as np
import pytest

import ilu0_ref as ir
import oracle_lib as ol
import solver_ref

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
PROBLEMS = {
    "tridiagonal_8": ir.tridiagonal_8,
    "tridiagonal_nonsym": ir.tridiagonal_nonsym,
    "laplacian_3d": lambda: ir.laplacian_3d(24),
    "random_pattern": lambda: ir.dominant_random(30_000, 7, 4),
    "lower_triangular": lambda: ir.lower_triangular_cut(5_000, 5, 6),
    "band33": ir.band33,
}
EXACT_IN_ROW_ORDER = ("tridiagonal_nonsym", "lower_triangular")  # no fill: the application is the solve
RUNS = defaultdict(int)
_CSR, _REF, _TWIN = {}, {}, {}


def _matrix(problem):
    if problem not in _CSR:
        _CSR[problem] = PROBLEMS[problem]()
    return _CSR[problem]


def _reference(problem, order, seq):
    if (problem, order) not in _REF:
        n, rp, cc, cv = _matrix(problem)
        _REF[problem, order] = ir.Ilu0(n, rp, cc, cv, seq)
    ref = _REF[problem, order]
    assert np.array_equal(ref.order, seq)
    return ref


def _handle(ctx, problem, order):
    n, rp, cc, cv = _matrix(problem)
    A = ctx.csr(n, n, rp, cc, cv)
    A.set_param("ilu0_order", order)
    return A


def _close(got, want, what):
    err = np.max(np.abs(got - want)) / max(np.max(np.abs(want)), 1e-300)
    print(f"{what}: {err:.3e}")
    assert err <= ol.REL_TOL, (what, err)


# ---- 1. order, factors, application, level structure ------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1], ids=["row_order", "multicolour"])
@pytest.mark.parametrize("problem", list(PROBLEMS))
def test_factors_and_application_match_the_reference(ctx, orc, pkg, problem, order):
    n, rp, cc, cv = _matrix(problem)
    A = _handle(ctx, problem, order)
    assert A.get_param("ilu0_ready") == 0 and A.get_param("ilu0_bytes") == 0
    seq = ctx.ilu0_order(A)
    assert A.get_param("ilu0_order") == order and A.get_param("ilu0_ready") == 1
    if order == 0:
        assert np.array_equal(seq, np.arange(n)) and A.get_param("ilu0_colours") == 0
    else:
        ncol, colour, want_seq = ol.greedy_colour_order(orc, rp, cc)
        assert A.get_param("ilu0_colours") == ncol and np.array_equal(seq, want_seq)
    ref = _reference(problem, order, seq)
    fac = ctx.ilu0_factors(A)
    _close(fac, ref.values, f"{problem} order {order}: factors")
    # duplicates: the first stored one carries the value, the later ones hold 0.0
    rows = np.repeat(np.arange(n), np.diff(rp))
    firsts = np.zeros(len(cc), bool)
    firsts[np.unique(rows.astype(np.int64) * n + cc, return_index=True)[1]] = True
    assert np.all(fac[~firsts] == 0.0)
    if problem == "random_pattern":
        assert (~firsts).sum() >= n  # (the doubled diagonal)
    # the application
    r_host = np.random.default_rng(23).uniform(-1, 1, n)
    r, z = ctx.vector_from(r_host), ctx.vector(n)
    z.fill(7.0)  # (whatever z holds is ignored)
    ctx.ilu0_solve(A, r, z)
    ctx.sync()
    got, want = z.download(), ref.apply(r_host)
    _close(got, want, f"{problem} order {order}: application")
    if problem in EXACT_IN_ROW_ORDER and order == 0:
        resid = lambda v: np.max(np.abs(ir.csr_mv(n, rp, cc, cv, v) - r_host)) / np.max(np.abs(r_host))
        print(f"{problem}: |A z - r|_inf / |r|_inf = {resid(got):.3e}, the reference's {resid(want):.3e}")
        assert resid(got) <= solver_ref.F * resid(want), (resid(got), resid(want))
    # the level structure
    lf, lb, launches = A.get_param("ilu0_levels_forward"), A.get_param("ilu0_levels_backward"), A.get_param("ilu0_launches")
    assert 1 <= lf <= n and 1 <= lb <= n and launches >= 2
    if problem == "tridiagonal_8":
        assert (lf, lb) == ((n, n) if order == 0 else (2, 2)) and A.get_param("ilu0_colours") == (0 if order == 0 else 2)
    if problem == "laplacian_3d":
        assert (lf, lb) == ((3 * 24 - 2, 3 * 24 - 2) if order == 0 else (2, 2)) and A.get_param("ilu0_colours") == (0 if order == 0 else 2)
    if problem == "lower_triangular" and order == 0:
        assert lb == 1
    RUNS["factors"] += 1


# ---- 2. determinism ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1], ids=["row_order", "multicolour"])
@pytest.mark.parametrize("problem", ["laplacian_3d", "random_pattern", "lower_triangular"])
def test_two_setups_and_two_applications_give_the_same_bits(ctx, pkg, problem, order):
    n = _matrix(problem)[0]
    A, B = _handle(ctx, problem, order), _handle(ctx, problem, order)
    ctx.ilu0_setup(A)
    fac = ctx.ilu0_factors(A).tobytes()
    assert ctx.ilu0_factors(B).tobytes() == fac, "a fresh handle of the same matrix has other factors"
    A.set_param("ilu0_order", 1 - order)
    assert A.get_param("ilu0_ready") == 0
    ctx.ilu0_setup(A)
    assert A.get_param("ilu0_ready") == 1 and (A.get_param("ilu0_colours") > 0) == (order == 0)
    A.set_param("ilu0_order", order)
    ctx.ilu0_setup(A)
    assert ctx.ilu0_factors(A).tobytes() == fac, "there and back: other factors"
    r = ctx.vector_from(np.random.default_rng(29).uniform(-1, 1, n))
    out = []
    for M in (A, A, B):
        z = ctx.vector(n)
        ctx.ilu0_solve(M, r, z)
        ctx.sync()
        out.append(z.download().tobytes())
    assert out[0] == out[1] == out[2], "two applications differ"
    RUNS["bits"] += 1


# ---- 3. the solvers ----------------------------------------------------------------------------------------------------------------
def _twin(system, order, seq):
    """(x of the pairwise twin, its host residual) at REL_TOL, once per (system, order)"""
    if (system, order) not in _TWIN:
        solver, n, rp, cc, cv, b = ir.solver_system(system)
        mv = lambda v: ir.csr_mv(n, rp, cc, cv, v)
        run = ir.run_bicgstab if solver == "bicgstab" else ir.run_cg
        x, iters = run(mv, ir.Ilu0(n, rp, cc, cv, seq).apply, b, ir.REL_TOL, 500)
        _TWIN[system, order] = (iters, np.linalg.norm(b - mv(x)) / np.linalg.norm(b))
    return _TWIN[system, order]


@pytest.mark.parametrize("order", [0, 1], ids=["row_order", "multicolour"])
@pytest.mark.parametrize("system", ir.SOLVER_SYSTEMS)
def test_preconditioned_solvers_take_the_iterations_of_the_twins(ctx, pkg, system, order):
    capi = pkg.capi
    solver, n, rp, cc, cv, b_host = ir.solver_system(system)
    A = ctx.csr(n, n, rp, cc, cv)
    A.set_param("ilu0_order", order)
    b, x = ctx.vector_from(b_host), ctx.vector(n)
    x.fill(0.0)
    solve = ctx.bicgstab if solver == "bicgstab" else ctx.cg
    iters, res = solve(A, b, x, max_iter=500, rel_tol=ir.REL_TOL, precond=capi.PRECOND_ILU0)
    assert A.get_param("ilu0_ready") == 1
    lo, hi = ir.TWIN_ITERATIONS[system, order]
    twin_iters, twin_true = _twin(system, order, ctx.ilu0_order(A))
    true = np.linalg.norm(b_host - ir.csr_mv(n, rp, cc, cv, x.download())) / np.linalg.norm(b_host)
    print(f"{system} order {order}: {iters} iterations (twins {lo}..{hi}, here {twin_iters}), reported {res:.3e}, true {true:.3e} (twin's {twin_true:.3e})")
    assert lo - 1 <= iters <= hi + 1, (iters, lo, hi)
    assert res <= ir.REL_TOL and true <= solver_ref.F * max(ir.REL_TOL, twin_true), (res, true, twin_true)
    # far fewer than without a preconditioner or with Jacobi (a constant diagonal), which take the same
    x.fill(0.0)
    plain = solve(A, b, x, max_iter=500, rel_tol=ir.REL_TOL)[0]
    print(f"{system}: {plain} iterations without a preconditioner (twins {ir.UNPRECONDITIONED_ITERATIONS[system]})")
    assert iters * 1.5 < plain, (plain, iters)
    # stopped by max_iter, a look every fourth iteration leaves the x of a look at every one
    xs = []
    for every in (1, 4):
        x.fill(0.0)
        assert solve(A, b, x, max_iter=7, rel_tol=0.0, check_every=every, precond=capi.PRECOND_ILU0)[0] == 7
        xs.append(x.download())
    if solver == "bicgstab":  # deterministic dot products: the same bits
        assert xs[0].tobytes() == xs[1].tobytes()
    else:  # spmv_cg adds its dot products up in arrival order: the same x up to that rounding, held to the parity tolerance
        _close(xs[1], xs[0], f"{system} order {order}: check_every 4 against 1")
    RUNS["solvers"] += 1


@pytest.mark.parametrize("problem", EXACT_IN_ROW_ORDER)
def test_an_exact_factorisation_ends_both_solvers_after_one_iteration(ctx, pkg, problem):
    capi = pkg.capi
    n, rp, cc, cv = _matrix(problem)
    A = _handle(ctx, problem, 0)
    b_host = np.random.default_rng(31).uniform(-1, 1, n)
    b, x = ctx.vector_from(b_host), ctx.vector(n)
    for solve in (ctx.bicgstab, ctx.cg):
        x.fill(0.0)
        iters, res = solve(A, b, x, max_iter=50, rel_tol=1e-9, precond=capi.PRECOND_ILU0)
        true = np.linalg.norm(b_host - ir.csr_mv(n, rp, cc, cv, x.download())) / np.linalg.norm(b_host)
        print(f"{problem} {solve.__name__}: {iters} iteration(s), reported {res:.3e}, true {true:.3e}")
        assert iters == 1 and res <= 1e-9 and true <= 1e-9, (solve.__name__, iters, res, true)
    RUNS["exact"] += 1


# ---- 4. refusals and hygiene ---------------------------------------------------------------------------------------------------------
def test_refusals(ctx, pkg):
    capi = pkg.capi

    def expect(call, code, word):
        with pytest.raises(capi.SpmvError) as e:
            call()
        assert e.value.code == code and word in str(e.value), (code, word, e.value)

    n, rp, cc, cv = _matrix("tridiagonal_8")
    A = ctx.csr(n, n, rp, cc, cv)
    r, z = ctx.vector_from(np.ones(n)), ctx.vector(n)
    rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(rp))
    others = {"ell": ctx.csr_to_ell(A), "coo": ctx.coo(n, n, rows, cc, cv), "dia": ctx.gen_dia_banded(64, 3, seed=2)}
    for fmt, M in others.items():
        m = M.info.nrow
        expect(lambda: ctx.ilu0_setup(M), UNSUPPORTED, "CSR")
        expect(lambda: ctx.ilu0_solve(M, ctx.vector(m), ctx.vector(m)), UNSUPPORTED, "CSR")
        expect(lambda: ctx.bicgstab(M, ctx.vector(m), ctx.vector(m), precond=capi.PRECOND_ILU0), UNSUPPORTED, "CSR")
        expect(lambda: ctx.cg(M, ctx.vector(m), ctx.vector(m), precond=capi.PRECOND_ILU0), UNSUPPORTED, "CSR")
    rp0 = np.arange(4, dtype=np.int32)
    R = ctx.csr(3, 4, rp0, np.array([0, 1, 2], np.int32), np.ones(3))
    expect(lambda: ctx.ilu0_setup(R), INVALID, "square")
    S = ctx.csr_shard(4, 8, n, rp.astype(np.int64), cc, cv)  # rows 4..7 of the 8 x 8 matrix
    expect(lambda: ctx.ilu0_setup(S), INVALID, "square")
    nb = 1_000_000
    P = ctx.gen_csr_uniform(0, nb, nb, 16, seed=31)
    P.set_kernel(capi.CSR_PANEL)
    P.set_param("panel_keep_csr", 0)
    assert P.get_param("panel_keep_csr") == 0
    expect(lambda: ctx.ilu0_setup(P), INVALID, "arrays")
    expect(lambda: ctx.bicgstab(P, ctx.vector(nb), ctx.vector(nb), precond=capi.PRECOND_ILU0), INVALID, "arrays")
    # no diagonal entries at all; a diagonal of stored zeros; a pivot that the elimination makes zero
    Z = ctx.csr(3, 3, rp0, np.array([1, 2, 0], np.int32), np.ones(3))
    expect(lambda: ctx.ilu0_setup(Z), INVALID, "diagonal")
    zero_diag = np.where(rows == cc, 0.0, cv)
    for order in (0, 1):
        D = ctx.csr(n, n, rp, cc, zero_diag)
        D.set_param("ilu0_order", order)
        expect(lambda: ctx.ilu0_setup(D), INVALID, "row 0")
        assert D.get_param("ilu0_ready") == 0 and D.get_param("ilu0_bytes") == 0
        O = ctx.csr(2, 2, np.array([0, 2, 4], np.int32), np.array([0, 1, 0, 1], np.int32), np.ones(4))
        O.set_param("ilu0_order", order)
        before = O.get_param("device_bytes")
        expect(lambda: ctx.ilu0_setup(O), INVALID, "row 1")
        assert O.get_param("ilu0_ready") == 0 and O.get_param("device_bytes") == before, "a failed set-up left state behind"
        expect(lambda: ctx.ilu0_solve(O, ctx.vector(2), ctx.vector(2)), INVALID, "row 1")
    # vectors
    expect(lambda: ctx.ilu0_solve(A, r, r), INVALID, "overlap")
    expect(lambda: ctx.ilu0_solve(A, r, ctx.vector(n + 1)), INVALID, "entries")
    other = capi.Context(0)
    expect(lambda: other.ilu0_setup(A), INVALID, "context")
    other.close()
    # the solvers
    expect(lambda: ctx.cg_multi(A, ctx.vector(2 * n), ctx.vector(2 * n), 2, precond=capi.PRECOND_ILU0), UNSUPPORTED, "ILU")
    expect(lambda: ctx.bicgstab(A, r, z, precond=capi.PRECOND_SYMGS), UNSUPPORTED, "Gauss-Seidel")
    for call in (lambda: ctx.cg(A, r, z, precond=7), lambda: ctx.bicgstab(A, r, z, precond=7),
                 lambda: ctx.cg_multi(A, ctx.vector(2 * n), ctx.vector(2 * n), 2, precond=7)):
        expect(call, INVALID, "unknown preconditioner")
    with pytest.raises(capi.SpmvError):
        A.set_param("ilu0_order", 2)
    with pytest.raises(capi.SpmvError):
        A.get_param("ilu0_nonsense")
    RUNS["refusals"] += 1


def test_the_state_is_the_handles_own(ctx, pkg):
    """a set-up and a solve leave the forward kernel, the plan and the transposed state alone; device_bytes grows by exactly
    "ilu0_bytes"; destroying the handle gives the memory back (ten handles of 36 MB of factors each against the suite's leak
    tolerance of 256 MiB, as tests/test_gpu_bicgstab.py checks its work vectors)"""
    n, rp, cc, cv = ir.laplacian_3d(64)
    r = ctx.vector_from(np.random.default_rng(37).uniform(-1, 1, n))
    z = ctx.vector(n)
    gc.collect()
    ctx.sync()
    free0, _ = ctx.mem_info()
    total = 0
    for rep in range(10):
        A = ctx.csr(n, n, rp, cc, cv)
        A.set_param("ilu0_order", rep & 1)
        plan, kernel, before, info_before = A.get_plan(), A.info.kernel, A.get_param("device_bytes"), A.info.device_bytes
        assert A.get_param("transpose_ready") == 0
        ctx.ilu0_setup(A)
        ctx.ilu0_solve(A, r, z)
        ctx.sync()
        grown = A.get_param("ilu0_bytes")
        assert grown >= 12 * (len(cc) - n) + 8 * n, grown  # at least the two triangles and the diagonal
        assert A.get_param("device_bytes") == before + grown and A.info.device_bytes == info_before + grown
        assert A.get_plan() == plan and A.info.kernel == kernel and A.get_param("transpose_ready") == 0
        total += grown
        del A
        gc.collect()
    ctx.sync()
    free1, _ = ctx.mem_info()
    assert total > 256 << 20, total
    assert abs(free0 - free1) < 256 << 20, f"{(free0 - free1) >> 20} MiB of device memory not returned"
    RUNS["state"] += 1


# ---- 5. coverage ---------------------------------------------------------------------------------------------------------------------
def test_every_case_ran():
    expect = {"factors": 2 * len(PROBLEMS), "bits": 6, "solvers": 2 * len(ir.SOLVER_SYSTEMS), "exact": len(EXACT_IN_ROW_ORDER), "refusals": 1, "state": 1}
    if any(RUNS[k] != c for k, c in expect.items()):
        pytest.skip(f"the coverage check needs every test of this module (ran {dict(RUNS)}, expected {expect})")
    assert {p for p, _ in _REF} == set(PROBLEMS) and {o for _, o in _REF} == {0, 1}
