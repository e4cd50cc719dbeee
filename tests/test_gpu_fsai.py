"""FSAI on the GPU (spmv_fsai_setup / _solve / _info / _factor; SPMV_PRECOND_FSAI in spmv_cg, spmv_bicgstab, spmv_gmres and
spmv_lobpcg) against the NumPy twin tests/fsai_ref.py, which tests/test_fsai_ref.py holds to facts of its own on the CPU.

Problems - the smallest that reach each path (pattern sizes: tests/test_fsai_ref.py) - with the levels they run at:
  tridiagonal_8       1        m <= 2: the 4-lane class, a partially filled group
  laplacian_2d_33     1, 2, 3  the 5-point Laplacian on 33 x 33: m up to 3 / 7 / 13, the classes of 4, 8 and 16 lanes, the pattern of
                               one and of two sparse products
  stencil27_12        1, 2     a 27-point diagonally dominant SPD stencil on 12^3: m up to 14, and up to 63 at level 2 - the 64-lane
                               class one below the cap; level 3 (m up to 172) is refused
  dense_blocks        1        three dense SPD blocks of order 64, rows interleaved: every m from 1 to 64, G the inverse Cholesky factor;
                               a block of order 65 is the refusal exactly at the cap
  random_symmetric    1        30,000 rows, unsorted columns, the diagonal entry stored twice, stored zeros: m up to 13; level 2 has a
                               row of 81 and is the realistic refusal
  diagonal            1        diag(4^k): G = diag(2^-k) and z = r / d bit for bit
The twin of a (problem, level) is computed once and shared.  test_every_case_ran asserts at the end that every case ran.
Section 7 takes every lane class of the row kernel on a later trip over its grid, with block-diagonal copies of bases of a few
rows (fsai_ref.GRID_LOOP_BASES, tests/tiled.py): more rows than any problem above, and the twin runs on the base alone."""
import functools
import gc
from collections import defaultdict

import numpy as np
import pytest

import fsai_ref as fr
import oracle_lib as ol
import solver_ref
import tiled

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
PROBLEMS = {
    "tridiagonal_8": (fr.tridiagonal_8, (1,)),
    "laplacian_2d_33": (lambda: fr.laplacian_2d(33), (1, 2, 3)),
    "stencil27_12": (lambda: fr.stencil27(12), (1, 2)),
    "dense_blocks": (lambda: fr.dense_blocks()[:4], (1,)),
    "random_symmetric": (fr.random_symmetric, (1,)),
    "diagonal": (fr.diagonal_powers_of_four, (1,)),
}
CASES = [(p, lv) for p, (_, levels) in PROBLEMS.items() for lv in levels]
BITS_CASES = [("laplacian_2d_33", 2), ("stencil27_12", 2), ("dense_blocks", 1), ("random_symmetric", 1)]
RUNS = defaultdict(int)
_CSR, _REF = {}, {}


def _matrix(problem):
    if problem not in _CSR:
        _CSR[problem] = PROBLEMS[problem][0]()
    return _CSR[problem]


def _twin(problem, level):
    if (problem, level) not in _REF:
        _REF[problem, level] = fr.Fsai(*_matrix(problem), level)
    return _REF[problem, level]


def _close(got, want, what):
    err = np.max(np.abs(got - want)) / max(np.max(np.abs(want)), 1e-300)
    print(f"{what}: {err:.3e}")
    assert err <= ol.REL_TOL, (what, err)


def _expect(capi, call, code, *words):
    with pytest.raises(capi.SpmvError) as e:
        call()
    assert e.value.code == code and all(w in str(e.value) for w in words), (code, words, e.value)


# ---- 1. pattern, values, defining facts, application, handle state --------------------------------------------------------------------
@pytest.mark.parametrize("problem,level", CASES)
def test_factor_application_and_state_match_the_twin(ctx, pkg, problem, level):
    n, rp, cc, cv = _matrix(problem)
    ref = _twin(problem, level)
    A = ctx.csr(n, n, rp, cc, cv)
    x_host = np.random.default_rng(19).uniform(-1, 1, n)
    x, y = ctx.vector_from(x_host), ctx.vector(n)

    def product():
        y.fill(0.0)
        ctx.apply(A, x, y)
        ctx.sync()
        return y.download().tobytes()

    plan, kernel, before, y_before = A.get_plan(), A.info.kernel, A.get_param("device_bytes"), product()
    assert [A.get_param(p) for p in ("fsai_ready", "fsai_bytes", "fsai_max_row")] == [0, 0, 0] and A.get_param("fsai_level") == 1
    ctx.fsai_setup(A, level)
    # the pattern integer for integer, the values at the parity tolerance
    g_rp, g_cc, g_val = ctx.fsai_factor(A)
    assert np.array_equal(g_rp, ref.rp) and np.array_equal(g_cc, ref.cc)
    _close(g_val, ref.values, f"{problem} level {level}: values of G")
    # the two facts that define G, from the engine's own G, in np.longdouble
    diag, off = fr.residuals(n, rp, cc, cv, g_rp, g_cc, g_val)
    print(f"{problem} level {level}: (G A G^T)_ii - 1: {diag:.2f} eps, (G A)_ij on S: {off:.2f} eps "
          f"(bounds {solver_ref.F} x {fr.DIAG_BOUND_EPS} and {solver_ref.F} x {fr.OFF_BOUND_EPS})")
    assert diag <= solver_ref.F * fr.DIAG_BOUND_EPS and off <= solver_ref.F * fr.OFF_BOUND_EPS, (diag, off)
    # the application against G^T (G r) formed on the host from the downloaded G
    r_host = np.random.default_rng(23).uniform(-1, 1, n)
    r, z = ctx.vector_from(r_host), ctx.vector(n)
    z.fill(7.0)  # (whatever z holds is overwritten)
    ctx.fsai_solve(A, r, z)
    ctx.sync()
    got = z.download()
    _close(got, fr.apply_factor(n, g_rp, g_cc, g_val, r_host), f"{problem} level {level}: application")
    if problem == "diagonal":
        assert g_val.tobytes() == (1.0 / np.sqrt(cv)).tobytes() and got.tobytes() == (r_host / cv).tobytes()
    if problem == "dense_blocks":  # the inverse Cholesky factor: z = A^-1 r
        resid = np.max(np.abs(fr.csr_mv(n, rp, cc, cv, got) - r_host)) / np.max(np.abs(r_host))
        print(f"dense_blocks: |A z - r|_inf / |r|_inf = {resid:.3e}")
        assert resid <= ol.REL_TOL
    # the handle's state
    assert A.get_param("fsai_ready") == 1 and A.get_param("fsai_max_row") == ref.max_row
    assert ctx.fsai_info(A) == (level, ref.nnz, ref.max_row)
    assert A.get_param("fsai_bytes") >= 2 * 12 * ref.nnz + 2 * 4 * (n + 1) + 8 * n
    assert A.get_param("fsai_level") == 1  # (what a solver's own set-up takes, not what this set-up was given)
    assert A.get_param("device_bytes") == before and A.get_plan() == plan and A.info.kernel == kernel and product() == y_before
    assert A.get_param("transpose_ready") == 0
    RUNS["factor"] += 1


# ---- 2. determinism ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem,level", BITS_CASES)
def test_two_setups_and_two_applications_give_the_same_bits(ctx, pkg, problem, level):
    """G: the same bytes from a second handle and from a rebuilt one.  z: the same bytes from two applications and from both handles;
    the products are the engine's, so the kernel choice is pinned to the model's where AUTO would time candidates (G of
    random_symmetric has 120,000 entries) - "panel_trial" 0 is handed down to G and G^T."""
    n, rp, cc, cv = _matrix(problem)
    A, B = ctx.csr(n, n, rp, cc, cv), ctx.csr(n, n, rp, cc, cv)
    for M in (A, B):
        M.set_param("panel_trial", 0)
        ctx.fsai_setup(M, level)
    fac = [a.tobytes() for a in ctx.fsai_factor(A)]
    assert [a.tobytes() for a in ctx.fsai_factor(B)] == fac, "a fresh handle of the same matrix has another factor"
    if level > 1:
        ctx.fsai_setup(A, 1)  # (there and back)
        assert ctx.fsai_info(A)[0] == 1
    ctx.fsai_setup(A, level)
    assert [a.tobytes() for a in ctx.fsai_factor(A)] == fac, "rebuilt: another factor"
    r = ctx.vector_from(np.random.default_rng(29).uniform(-1, 1, n))
    out = []
    for M in (A, A, B):
        z = ctx.vector(n)
        ctx.fsai_solve(M, r, z)
        ctx.sync()
        out.append(z.download().tobytes())
    assert out[0] == out[1] == out[2], "two applications differ"
    RUNS["bits"] += 1


# ---- 3. the cap -------------------------------------------------------------------------------------------------------------------------
def test_rows_beyond_the_cap_are_refused_and_the_earlier_state_stays(ctx, pkg):
    capi = pkg.capi
    # the 27-point stencil at level 3: refused, and the level-2 state still applies
    n, rp, cc, cv = _matrix("stencil27_12")
    A = ctx.csr(n, n, rp, cc, cv)
    ctx.fsai_setup(A, 2)
    r, z = ctx.vector_from(np.random.default_rng(31).uniform(-1, 1, n)), ctx.vector(n)
    ctx.fsai_solve(A, r, z)
    ctx.sync()
    z2, bytes2 = z.download().tobytes(), A.get_param("fsai_bytes")
    with pytest.raises(fr.RowTooLong) as twin:
        fr.Fsai(n, rp, cc, cv, 3)
    _expect(capi, lambda: ctx.fsai_setup(A, 3), UNSUPPORTED, f"row {twin.value.row} ", f"m = {twin.value.m} ", "cap is 64", "172")
    assert ctx.fsai_info(A) == (2, _twin("stencil27_12", 2).nnz, 63) and A.get_param("fsai_bytes") == bytes2
    z.fill(0.0)
    ctx.fsai_solve(A, r, z)
    ctx.sync()
    assert z.download().tobytes() == z2
    # exactly at the cap: a dense block of order 65 has one row of 65
    n, rp, cc, cv = fr.dense_blocks((64, 65, 3))[:4]
    with pytest.raises(fr.RowTooLong) as twin:
        fr.Fsai(n, rp, cc, cv, 1)
    assert twin.value.m == 65
    D = ctx.csr(n, n, rp, cc, cv)
    _expect(capi, lambda: ctx.fsai_setup(D, 1), UNSUPPORTED, f"row {twin.value.row} ", "m = 65 ", "cap is 64")
    assert D.get_param("fsai_ready") == 0
    _expect(capi, lambda: ctx.fsai_solve(D, ctx.vector(n), ctx.vector(n)), INVALID, "not set up")
    # the realistic one: the random matrix at level 2
    n, rp, cc, cv = _matrix("random_symmetric")
    with pytest.raises(fr.RowTooLong) as twin:
        fr.Fsai(n, rp, cc, cv, 2)
    R = ctx.csr(n, n, rp, cc, cv)
    _expect(capi, lambda: ctx.fsai_setup(R, 2), UNSUPPORTED, f"row {twin.value.row} ", f"m = {twin.value.m} ")
    # ... and as a solver's own set-up: the refusal is the solve's
    R.set_param("fsai_level", 2)
    _expect(capi, lambda: ctx.cg(R, ctx.vector(n), ctx.vector(n), precond=capi.PRECOND_FSAI), UNSUPPORTED, "cap is 64")
    RUNS["cap"] += 1


# ---- 4. edges ---------------------------------------------------------------------------------------------------------------------------
def test_edges(ctx, pkg):
    capi = pkg.capi
    # n = 0: nothing is launched, everything answers
    E = ctx.csr(0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    ctx.fsai_setup(E, 3)
    assert ctx.fsai_info(E) == (3, 0, 0) and E.get_param("fsai_ready") == 1 and E.get_param("fsai_bytes") == 0
    ctx.fsai_solve(E, ctx.vector(0), ctx.vector(0))
    e_rp, e_cc, e_cv = ctx.fsai_factor(E)
    assert e_rp.tolist() == [0] and len(e_cc) == 0 and len(e_cv) == 0
    assert ctx.cg(E, ctx.vector(0), ctx.vector(0), precond=capi.PRECOND_FSAI)[0] == 0
    # n = 1, at every level
    for level in (1, 2, 3):
        O = ctx.csr(1, 1, np.array([0, 1], np.int32), np.zeros(1, np.int32), np.array([16.0]))
        ctx.fsai_setup(O, level)
        o_rp, o_cc, o_cv = ctx.fsai_factor(O)
        assert o_rp.tolist() == [0, 1] and o_cc.tolist() == [0] and o_cv.tolist() == [0.25]
        r, z = ctx.vector_from(np.array([3.0])), ctx.vector(1)
        ctx.fsai_solve(O, r, z)
        ctx.sync()
        assert z.download().tolist() == [3.0 / 16.0]
    # a row without a stored diagonal entry names the row; nothing is left, an earlier state included
    rp3 = np.arange(4, dtype=np.int32)
    Z = ctx.csr(3, 3, rp3, np.array([0, 1, 0], np.int32), np.ones(3))
    before = Z.get_param("device_bytes")
    _expect(capi, lambda: ctx.fsai_setup(Z, 1), INVALID, "row 2 ", "diagonal")
    assert Z.get_param("fsai_ready") == 0 and Z.get_param("device_bytes") == before
    # a pivot that is not positive: [[1, 2], [2, 1]] names row 1, at every level
    for level in (1, 2):
        N = ctx.csr(2, 2, np.array([0, 2, 4], np.int32), np.array([0, 1, 0, 1], np.int32), np.array([1.0, 2.0, 2.0, 1.0]))
        _expect(capi, lambda: ctx.fsai_setup(N, level), INVALID, "row 1 ", "pivot")
        assert N.get_param("fsai_ready") == 0 and N.get_param("fsai_bytes") == 0
        _expect(capi, lambda: ctx.fsai_solve(N, ctx.vector(2), ctx.vector(2)), INVALID, "not set up")
        _expect(capi, lambda: ctx.cg(N, ctx.vector_from(np.ones(2)), ctx.vector(2), precond=capi.PRECOND_FSAI), INVALID, "row 1 ")
    # a pivot that is not finite is a bad pivot too
    W = ctx.csr(2, 2, np.array([0, 1, 3], np.int32), np.array([0, 0, 1], np.int32), np.array([np.nan, 1.0, 1.0]))
    _expect(capi, lambda: ctx.fsai_setup(W, 1), INVALID, "row 0 ")
    # only the lower triangle is read: an upper triangle of garbage changes nothing
    n, rp, cc, cv = _matrix("laplacian_2d_33")
    rows = np.repeat(np.arange(n), np.diff(rp))
    L = ctx.csr(n, n, rp, cc, np.where(cc > rows, 1e30, cv))
    ctx.fsai_setup(L, 1)
    assert ctx.fsai_factor(L)[2].tobytes() == _gpu_values(ctx, "laplacian_2d_33", 1)
    RUNS["edges"] += 1


def _gpu_values(ctx, problem, level):
    n, rp, cc, cv = _matrix(problem)
    A = ctx.csr(n, n, rp, cc, cv)
    ctx.fsai_setup(A, level)
    return ctx.fsai_factor(A)[2].tobytes()


# ---- 5. the solvers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [1, 2, 3])
@pytest.mark.parametrize("system", fr.SOLVER_SYSTEMS)
def test_cg_takes_the_iterations_of_the_twins(ctx, pkg, system, level):
    capi = pkg.capi
    n, rp, cc, cv, b_host = fr.solver_system(system)
    A = ctx.csr(n, n, rp, cc, cv)
    A.set_param("fsai_level", level)
    assert A.get_param("fsai_level") == level
    b, x = ctx.vector_from(b_host), ctx.vector(n)
    x.fill(0.0)
    iters, res = ctx.cg(A, b, x, max_iter=500, rel_tol=fr.REL_TOL, precond=capi.PRECOND_FSAI)
    assert A.get_param("fsai_ready") == 1 and ctx.fsai_info(A)[0] == level
    lo, hi = fr.TWIN_ITERATIONS[system, level]
    mv = lambda v: fr.csr_mv(n, rp, cc, cv, v)
    x_twin, twin_iters = fr.run_cg(mv, fr.Fsai(n, rp, cc, cv, level).apply, b_host, fr.REL_TOL, 500)
    twin_true = np.linalg.norm(b_host - mv(x_twin)) / np.linalg.norm(b_host)
    true = np.linalg.norm(b_host - mv(x.download())) / np.linalg.norm(b_host)
    print(f"{system} level {level}: {iters} iterations (twins {lo}..{hi}, here {twin_iters}), reported {res:.3e}, true {true:.3e} (twin's {twin_true:.3e})")
    assert lo - 1 <= iters <= hi + 1, (iters, lo, hi)
    assert res <= fr.REL_TOL and true <= solver_ref.F * max(fr.REL_TOL, twin_true), (res, true, twin_true)
    x.fill(0.0)
    plain = ctx.cg(A, b, x, max_iter=500, rel_tol=fr.REL_TOL)[0]
    print(f"{system}: {plain} iterations without a preconditioner (twins {fr.UNPRECONDITIONED_ITERATIONS[system]})")
    assert iters < plain, (plain, iters)
    RUNS["cg"] += 1


def test_a_handle_that_was_set_up_is_used_as_it_stands(ctx, pkg):
    """set up at level 2 and then solved with SPMV_PRECOND_FSAI: level 2, not the "fsai_level" default of 1"""
    capi = pkg.capi
    n, rp, cc, cv, b_host = fr.solver_system("laplacian_2d_33")
    A = ctx.csr(n, n, rp, cc, cv)
    ctx.fsai_setup(A, 2)
    b, x = ctx.vector_from(b_host), ctx.vector(n)
    x.fill(0.0)
    iters, res = ctx.cg(A, b, x, max_iter=500, rel_tol=fr.REL_TOL, precond=capi.PRECOND_FSAI)
    lo, hi = fr.TWIN_ITERATIONS["laplacian_2d_33", 2]
    assert ctx.fsai_info(A)[0] == 2 and A.get_param("fsai_level") == 1 and lo - 1 <= iters <= hi + 1, (iters, lo, hi)
    assert hi + 1 < fr.TWIN_ITERATIONS["laplacian_2d_33", 1][0] - 1  # (the two levels cannot be mistaken for one another)
    RUNS["reuse"] += 1


def test_the_other_solvers_converge_under_it(ctx, pkg):
    capi = pkg.capi
    n, rp, cc, cv, b_host = fr.solver_system("laplacian_2d_33")
    mv = lambda v: fr.csr_mv(n, rp, cc, cv, v)
    A = ctx.csr(n, n, rp, cc, cv)
    b, x = ctx.vector_from(b_host), ctx.vector(n)
    for name, solve in (("bicgstab", ctx.bicgstab), ("gmres", ctx.gmres)):
        x.fill(0.0)
        plain = solve(A, b, x, max_iter=500, rel_tol=fr.REL_TOL)[0]
        x.fill(0.0)
        iters, res = solve(A, b, x, max_iter=500, rel_tol=fr.REL_TOL, precond=capi.PRECOND_FSAI)
        true = np.linalg.norm(b_host - mv(x.download())) / np.linalg.norm(b_host)
        print(f"{name}: {iters} iterations under FSAI level 1 ({plain} without), reported {res:.3e}, true {true:.3e}")
        assert res <= fr.REL_TOL and true <= solver_ref.F * fr.REL_TOL and iters < plain, (name, iters, plain, res, true)
    # spmv_lobpcg: the two smallest eigenvalues of the 5-point Laplacian, 4 - 2 cos(i pi / 34) - 2 cos(j pi / 34)
    k, nev, tol = 4, 2, 1e-7
    c = np.cos(np.arange(1, 4) * np.pi / 34)
    want = np.sort((4 - 2 * c[:, None] - 2 * c[None, :]).ravel())[:nev]
    counts = {}
    for code in (capi.PRECOND_NONE, capi.PRECOND_FSAI):
        X = ctx.gen_vector(n * k, seed=5)
        theta, resid, it = ctx.lobpcg(A, X, k, nev=nev, max_iter=400, tol=tol, precond=code)
        print(f"lobpcg precond {code}: {it} iterations, theta {theta[:nev]}, resid {resid[:nev]}")
        assert np.all(resid[:nev] <= tol) and np.allclose(theta[:nev], want, rtol=0, atol=1e-6), (code, theta, resid, want)
        counts[code] = it
    assert counts[capi.PRECOND_FSAI] < counts[capi.PRECOND_NONE], counts
    RUNS["others"] += 1


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, pkg):
    capi = pkg.capi
    n, rp, cc, cv = _matrix("tridiagonal_8")
    A = ctx.csr(n, n, rp, cc, cv)
    r, z = ctx.vector_from(np.ones(n)), ctx.vector(n)
    rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(rp))
    others = {"ell": ctx.csr_to_ell(A), "coo": ctx.coo(n, n, rows, cc, cv), "bsr": ctx.csr_to_bsr(A, 2)}
    for fmt, M in others.items():
        m = M.info.nrow
        _expect(capi, lambda: ctx.fsai_setup(M, 1), UNSUPPORTED, "CSR")
        _expect(capi, lambda: ctx.fsai_solve(M, ctx.vector(m), ctx.vector(m)), UNSUPPORTED, "CSR")
        _expect(capi, lambda: ctx.fsai_factor(M), UNSUPPORTED, "CSR")
        for solve in (ctx.cg, ctx.bicgstab, ctx.gmres):
            _expect(capi, lambda: solve(M, ctx.vector(m), ctx.vector(m), precond=capi.PRECOND_FSAI), UNSUPPORTED, "CSR")
    rp0 = np.arange(4, dtype=np.int32)
    R = ctx.csr(3, 4, rp0, np.array([0, 1, 2], np.int32), np.ones(3))
    _expect(capi, lambda: ctx.fsai_setup(R, 1), INVALID, "square")
    S = ctx.csr_shard(4, 8, n, rp.astype(np.int64), cc, cv)  # rows 4..7 of the 8 x 8 matrix
    _expect(capi, lambda: ctx.fsai_setup(S, 1), INVALID, "square")
    _expect(capi, lambda: ctx.bicgstab(S, ctx.vector(4), ctx.vector(4), precond=capi.PRECOND_FSAI), INVALID)
    nb = 1_000_000
    P = ctx.gen_csr_uniform(0, nb, nb, 16, seed=31)
    P.set_kernel(capi.CSR_PANEL)
    P.set_param("panel_keep_csr", 0)
    assert P.get_param("panel_keep_csr") == 0
    _expect(capi, lambda: ctx.fsai_setup(P, 1), INVALID, "arrays")
    _expect(capi, lambda: ctx.gmres(P, ctx.vector(nb), ctx.vector(nb), precond=capi.PRECOND_FSAI), INVALID, "arrays")
    del P
    # levels
    for level in (-1, 4):
        _expect(capi, lambda: ctx.fsai_setup(A, level), INVALID, "level")
    for value in (0, 4):
        with pytest.raises(capi.SpmvError):
            A.set_param("fsai_level", value)
    for name in ("fsai_ready", "fsai_bytes", "fsai_max_row"):  # read-only
        with pytest.raises(capi.SpmvError):
            A.set_param(name, 1)
    with pytest.raises(capi.SpmvError):
        A.get_param("fsai_nonsense")
    # vectors, set-up, context
    _expect(capi, lambda: ctx.fsai_solve(A, r, z), INVALID, "not set up")
    _expect(capi, lambda: ctx.fsai_factor(A), INVALID, "not set up")
    _expect(capi, lambda: ctx.fsai_info(A), INVALID, "not set up")
    ctx.fsai_setup(A)
    _expect(capi, lambda: ctx.fsai_solve(A, r, r), INVALID, "overlap")
    _expect(capi, lambda: ctx.fsai_solve(A, r, ctx.vector(n + 1)), INVALID, "entries")
    other = capi.Context(0)
    _expect(capi, lambda: other.fsai_setup(A, 1), INVALID, "context")
    other.close()
    # the solvers: spmv_cg_multi is not built for it; 7 and 9 stay unknown.  (spmv_cgls takes no preconditioner argument at all)
    _expect(capi, lambda: ctx.cg_multi(A, ctx.vector(2 * n), ctx.vector(2 * n), 2, precond=capi.PRECOND_FSAI), UNSUPPORTED, "FSAI")
    for bad in (7, 9):
        for call in (lambda: ctx.cg(A, r, z, precond=bad), lambda: ctx.bicgstab(A, r, z, precond=bad), lambda: ctx.gmres(A, r, z, precond=bad),
                     lambda: ctx.cg_multi(A, ctx.vector(2 * n), ctx.vector(2 * n), 2, precond=bad)):
            _expect(capi, call, INVALID, "unknown preconditioner")
    RUNS["refusals"] += 1


def test_destroying_the_handle_gives_the_memory_back(ctx, pkg):
    """six handles of the 64^3 Laplacian at level 2 - G and G^T of 3.3 million entries each, with their layouts - against the suite's
    leak tolerance of 256 MiB, as tests/test_gpu_ilu0.py checks its factors"""
    n, rp, cc, cv = fr.laplacian_3d(64)
    r = ctx.vector_from(np.random.default_rng(37).uniform(-1, 1, n))
    z = ctx.vector(n)
    gc.collect()
    ctx.sync()
    free0, _ = ctx.mem_info()
    total = 0
    for rep in range(6):
        A = ctx.csr(n, n, rp, cc, cv)
        before = A.get_param("device_bytes")
        ctx.fsai_setup(A, 2)
        ctx.fsai_solve(A, r, z)
        ctx.sync()
        assert A.get_param("device_bytes") == before
        total += A.get_param("fsai_bytes")
        del A
        gc.collect()
    ctx.sync()
    free1, _ = ctx.mem_info()
    assert total > 256 << 20, total
    assert abs(free0 - free1) < 256 << 20, f"{(free0 - free1) >> 20} MiB of device memory not returned"
    RUNS["state"] += 1


# ---- 7. later trips over the grid -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grid_loop_case(lanes):
    return fr.grid_loop_case(lanes)


@pytest.mark.parametrize("lanes", sorted(fr.GRID_LOOP_BASES))
def test_rows_on_a_later_trip_over_the_grid_repeat_the_first_trip(ctx, pkg, lanes):
    """fsai_rows_kernel launches at most kMaxGrid workgroups and loops beyond; on a later trip a group starts from the LDS its row
    before left behind.  Block-diagonal copies of a small base (tests/tiled.py) put more rows into the class of `lanes` lanes than
    one trip takes: G's pattern is the base twin's tiled, the values of every copy are the bytes of copy 0, and copy 0 is held to
    the base twin as test_factor_application_and_state_match_the_twin holds a factor."""
    case = _grid_loop_case(lanes)
    n0, rp0, cc0, cv0, level, ref, k = case["n"], case["rp"], case["cc"], case["cv"], case["level"], case["ref"], case["copies"]
    rows, groups, grid = case["rows"], case["groups"], case["grid"]
    print(f"{lanes} lanes: {k} copies x {rows} rows = {k * rows} > {groups} x {grid} = {groups * grid}: {tiled.trips(k * rows, groups, grid)} trips; "
          f"n = {k * n0}, nnz(G) = {k * ref.nnz}, level {level}")
    assert k * rows > groups * grid, f"the class of {lanes} lanes makes one trip over the grid: nothing of this test is left"
    assert (groups * grid) % rows != 0, f"{rows} rows a copy divide a trip of the class of {lanes} lanes: every trip holds the same rows"
    n = k * n0
    A = ctx.csr(n, n, *tiled.tile_csr(k, n0, rp0, cc0, cv0))
    ctx.fsai_setup(A, level)
    g_rp, g_cc, g_val = ctx.fsai_factor(A)
    # the pattern integer for integer, the values of every copy the bytes of copy 0
    nnz0 = ref.nnz
    bad = tiled.tiled_mismatch((g_rp, g_cc, g_val), (ref.rp.astype(np.int32), ref.cc.astype(np.int32), g_val[:nnz0]), k, n0, case["where"])
    assert bad is None, bad
    # copy 0 against the base twin, and the two facts that define G from the engine's first n0 rows, in np.longdouble
    _close(g_val[:nnz0], ref.values, f"{lanes} lanes: values of copy 0")
    diag, off = fr.residuals(n0, rp0, cc0, cv0, g_rp[:n0 + 1], g_cc[:nnz0], g_val[:nnz0])
    print(f"{lanes} lanes: (G A G^T)_ii - 1: {diag:.2f} eps, (G A)_ij on S: {off:.2f} eps")
    assert diag <= solver_ref.F * fr.DIAG_BOUND_EPS and off <= solver_ref.F * fr.OFF_BOUND_EPS, (diag, off)
    assert ctx.fsai_info(A) == (level, k * nnz0, ref.max_row) and A.get_param("fsai_max_row") == ref.max_row
    # the application against G^T (G r) formed on the host from the downloaded G
    r_host = np.random.default_rng(23).uniform(-1, 1, n)
    r, z = ctx.vector_from(r_host), ctx.vector(n)
    z.fill(7.0)
    ctx.fsai_solve(A, r, z)
    ctx.sync()
    _close(z.download(), fr.apply_factor(n, g_rp, g_cc, g_val, r_host), f"{lanes} lanes: application")


# ---- 8. coverage ------------------------------------------------------------------------------------------------------------------------
def test_every_case_ran():
    expect = {"factor": len(CASES), "bits": len(BITS_CASES), "cap": 1, "edges": 1, "cg": 3 * len(fr.SOLVER_SYSTEMS), "reuse": 1, "others": 1,
              "refusals": 1, "state": 1}
    if any(RUNS[k] != c for k, c in expect.items()):
        pytest.skip(f"the coverage check needs every test of this module (ran {dict(RUNS)}, expected {expect})")
    assert {p for p, _ in _REF} >= set(PROBLEMS)
