"""The NumPy twin of the Chebyshev preconditioner and of the Lanczos estimate (tests/chebyshev_ref.py) held to facts of its own, on
the CPU: the closed form on diagonal matrices in longdouble, the contraction bound, definiteness, the row bound, mutations that
must each be caught, Lanczos against a longdouble run and its breakdown, and the iteration counts the GPU test compares with."""
import numpy as np
import pytest

import chebyshev_ref as cr
import ilu0_ref as ir

LD = np.longdouble
DEGREES = (1, 2, 5, 16)


def _diagonal_case(scaled):
    """(a, s, lambda, r): A = diag(a), B = diag(s a) = diag(lambda), the family of chebyshev_ref.diagonal_family"""
    lam = cr.diagonal_family(*cr.DIAGONAL_BOUNDS)
    rng = np.random.default_rng(5)
    r = rng.uniform(0.5, 1.5, len(lam))
    s = rng.uniform(0.5, 2.0, len(lam)) if scaled else None
    a = lam / s if scaled else lam
    return a, s, lam, r


def _deviation(d, scaled, mutate=None):
    """largest relative deviation of z_i / r_i from s_i p_d(lambda_i) in longdouble"""
    lmin, lmax = cr.DIAGONAL_BOUNDS
    a, s, lam, r = _diagonal_case(scaled)
    c0, c1, c2 = cr.coefficients(d, lmin, lmax, mutate=mutate)
    z = cr.apply(lambda x: a * x, s, r, c0, c1, c2, mutate=mutate)
    want = cr.closed_form(lam if not scaled else (LD(1) * s) * a, d, lmin, lmax) * (LD(1) * s if scaled else LD(1))
    return float(np.max(np.abs((LD(1) * z) / r - want) / np.abs(want)))


@pytest.mark.parametrize("d", DEGREES + (9,))
def test_diagonal_matrices_follow_the_closed_form(d):
    e = _deviation(d, scaled=False)
    e_scaled = _deviation(d, scaled=True)
    print(f"degree {d}: E_d = {e:.3e} (recorded {cr.E_D[d]:.1e}), with a scaling vector {e_scaled:.3e}")
    assert cr.E_D[d] / 2 <= e <= cr.E_D[d], "chebyshev_ref.E_D is the record of this figure"
    assert e_scaled <= 4 * cr.E_D[d]
    # the residual polynomial has degree d + 1 (the start and d terms): with T_d in its place the closed form is off by O(1)
    lmin, lmax = cr.DIAGONAL_BOUNDS
    lam = cr.diagonal_family(lmin, lmax)
    wrong = cr.closed_form(lam, d - 1, lmin, lmax) if d > 1 else None
    if wrong is not None:
        assert np.max(np.abs(cr.closed_form(lam, d, lmin, lmax) - wrong) / np.abs(wrong)) > 1e-2


@pytest.mark.parametrize("d", DEGREES)
def test_every_mutation_is_caught(d):
    for mutate in cr.MUTATIONS:
        if mutate == "rho" and d == 1:
            continue  # (rho_1 is the last one a single term uses)
        e = _deviation(d, scaled=True, mutate=mutate)
        print(f"degree {d}, {mutate}: {e:.3e}")
        assert e > 1000 * cr.E_D[d], (d, mutate, e)


@pytest.mark.parametrize("d", range(1, 9))
def test_the_error_contracts_by_the_chebyshev_bound(d):
    """32^2 Laplacian, unscaled, the exact extreme eigenvalues as bounds: e - M^-1 A e is T_{d+1}((theta - A) / delta) e /
    T_{d+1}(sigma), at most 1 / T_{d+1}(sigma) times e in the 2-norm (which is below 1 / T_d(sigma))"""
    n, rp, cc, cv = cr.laplacian_2d_csr(32)
    lmin, lmax = cr.laplacian_2d_bounds(32)
    mv = lambda x: ir.csr_mv(n, rp, cc, cv, x)
    c0, c1, c2 = cr.coefficients(d, lmin, lmax)
    e = np.random.default_rng(7).uniform(-1, 1, n)
    after = e - cr.apply(mv, None, mv(e), c0, c1, c2)
    ratio, bound = np.linalg.norm(after) / np.linalg.norm(e), cr.contraction(d, lmin, lmax)
    print(f"degree {d}: {ratio:.6e} against 1 / T_{d + 1}(sigma) = {bound:.6e}")
    assert ratio <= bound * (1 + 1e-12)
    assert bound < float(1 / cr.chebyshev_t(d, np.asarray(LD(lmax + lmin) / LD(lmax - lmin))))


def test_the_operator_is_positive_definite_under_the_row_bound():
    n, rp, cc, cv = ir.laplacian_3d(12)
    minv = cr.default_preconditioner(n, rp, cc, cv, 4)
    rng = np.random.default_rng(11)
    for _ in range(20):
        r = rng.uniform(-1, 1, n)
        assert np.dot(r, minv(r)) > 0.0


def test_row_bound():
    for n, rp, cc, cv in (ir.laplacian_3d(6), cr.laplacian_2d_csr(9), cr.tridiagonal(17)):
        assert cr.row_bound(n, rp, cc, cv, cr.inverse_diagonal(n, rp, cc, cv)) == 2.0
    # at or above the spectral radius of B: the 300-row leading block of a random dominant matrix, rebuilt as its own matrix
    n, rp, cc, cv = ir.dominant_random(3000, 7, 4)
    rows = np.repeat(np.arange(n), np.diff(rp))
    keep = (rows < 300) & (cc < 300)
    dense = np.zeros((300, 300))
    np.add.at(dense, (rows[keep], cc[keep]), cv[keep])
    m, rp2, cc2, cv2 = ir.from_dense(dense)
    s = cr.inverse_diagonal(m, rp2, cc2, cv2)
    radius = np.max(np.abs(np.linalg.eigvals(s[:, None] * dense)))
    bound = cr.row_bound(m, rp2, cc2, cv2, s)
    print(f"row bound {bound:.6f}, spectral radius {radius:.6f}")
    assert bound >= radius
    # every stored entry counts, duplicates separately
    assert cr.row_bound(2, np.array([0, 3, 4]), np.array([0, 0, 1, 1]), np.array([1.0, -1.0, 0.5, 2.0])) == 2.5


@pytest.mark.parametrize("m", (8, 16, 30))
def test_lanczos_agrees_with_a_longdouble_run(m):
    n, rp, cc, cv = cr.laplacian_2d_csr(32)
    s = cr.inverse_diagonal(n, rp, cc, cv)
    rows = np.repeat(np.arange(n), np.diff(rp))

    def mv(x):  # keeps x's precision
        out = np.zeros(n, dtype=x.dtype)
        np.add.at(out, rows, cv.astype(x.dtype) * x[cc])
        return out

    v0 = np.random.default_rng(13).uniform(-1, 1, n)
    a, b, done, lo, hi = cr.lanczos(mv, s, v0, m)
    al, bl, done_l, _, _ = cr.lanczos(mv, s, v0, m, kind=LD)
    assert done == done_l == m
    dev = max(float(np.max(np.abs(a - al))), float(np.max(np.abs(b - bl))))
    print(f"m = {m}: coefficients within {dev:.3e} of the longdouble run; Ritz extremes {lo:.6f}, {hi:.6f}")
    assert dev <= 1e-13
    lmin, lmax = cr.laplacian_2d_bounds(32)
    v = v0 / np.linalg.norm(v0)
    rayleigh = float(np.dot(v, np.sqrt(s) * mv(np.sqrt(s) * v)))
    assert rayleigh <= hi <= lmax / 4.0 and lmin / 4.0 <= lo <= rayleigh
    assert a[0] == pytest.approx(rayleigh, rel=1e-14)


def test_lanczos_breakdown():
    n = 50
    v0 = np.random.default_rng(17).uniform(-1, 1, n)
    a, b, done, lo, hi = cr.lanczos(lambda x: x.copy(), None, np.ones(64), 8)  # (||v_0|| = 8: the normalisation is exact)
    assert done == 1 and lo == 1.0 and hi == 1.0
    a, b, done, lo, hi = cr.lanczos(lambda x: x.copy(), None, v0, 8)  # alpha_0 = v_0 . v_0 is 1 up to the normalisation's rounding
    assert done == 1 and lo == hi == a[0] and abs(lo - 1.0) <= 4 * np.spacing(1.0)
    values = np.array([1.0, 1.25, 1.75])
    diag = np.repeat(values, [20, 17, 13])
    a, b, done, lo, hi = cr.lanczos(lambda x: diag * x, None, v0, 8)
    ulp = np.spacing(1.75)
    print(f"three values: {done} steps, Ritz extremes off by {(lo - 1.0) / ulp:.1f} and {(hi - 1.75) / ulp:.1f} ulp")
    assert done == 3 and abs(lo - 1.0) <= 4 * ulp and abs(hi - 1.75) <= 4 * ulp


def test_sturm_bisection_against_numpy():
    rng = np.random.default_rng(19)
    a, b = rng.uniform(-1, 1, 12), rng.uniform(0.1, 1, 11)
    want = np.linalg.eigvalsh(np.diag(a) + np.diag(b, 1) + np.diag(b, -1))
    got = [cr.tridiagonal_eigenvalue(a, b, k) for k in range(12)]
    assert np.max(np.abs(np.array(got) - want)) <= 16 * np.spacing(np.max(np.abs(want)))


def test_iteration_counts_of_the_twins():
    """what tests/test_gpu_chebyshev.py compares the engine's iterations with; a preconditioned solve takes fewer than half the
    iterations of the plain one"""
    got_pre = {(name, d): cr.run_twin(name, d)[1] for name in cr.SYSTEMS for d in cr.DEGREES}
    got_plain = {name: cr.run_twin(name, 0)[1] for name in cr.SYSTEMS}
    print(got_pre, got_plain)
    assert got_pre == cr.TWIN_ITERATIONS and got_plain == cr.UNPRECONDITIONED_ITERATIONS
    for (name, d), k in got_pre.items():
        assert 2 * k < got_plain[name], (name, d)
