"""CPU-side checks of the LOBPCG twin (tests/lobpcg_ref.py) and of the outcome checks that tests/test_gpu_lobpcg.py holds spmv_lobpcg to:
the twin meets (a)-(d) on every problem of the GPU file within max_iter, and the checks reject wrong answers - a missed pair, an
unnormalised X, two theta swapped, a residual understated by a factor of 10.

The three preconditioned 64 x 64 problems run here with M = I: the engine's Chebyshev polynomial and AMG cycle need the device (the GPU
file hands them to the twin as its M^-1).  The problem, the block and the checks are the same."""
import os

import numpy as np
import pytest

import lobpcg_ref as lr


@pytest.fixture(scope="module")
def vec_uniform(pkg):
    return pkg.synth.vec_uniform


@pytest.mark.parametrize("name", list(lr.PROBLEMS))
def test_twin_meets_the_outcome_checks_on_every_problem(name, vec_uniform):
    E, lam, k, nev, largest, tol, max_iter, pre = lr.problem(name)
    if pre in ("chebyshev", "amg", "amg_sa"):
        theta, resid, it, X = lr.lobpcg(E.matvec, lr.start_block(name, vec_uniform), nev=nev, largest=largest, max_iter=800, tol=tol)
        max_iter = 800
    else:
        theta, resid, it, X = lr.twin(name, vec_uniform)
    print(f"{name}: {it} iterations, resid max {resid[:nev].max():.2e}")
    assert it < max_iter or np.all(resid[:nev] <= tol), (name, it, resid)
    assert lr.outcome_failures(E.matvec_ld, E.norm_inf(), X, theta, resid, nev, tol, lam, largest) == []
    if name == "diagonal_unit_start":
        assert it == 0


def test_sturm_bisection_agrees_with_a_dense_solver_on_a_small_matrix():
    d, e = 1.0 + np.arange(30), np.full(29, -0.25)
    T = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
    assert np.max(np.abs(lr.sturm_lowest(d, e, 6) - np.linalg.eigvalsh(T)[:6])) <= 1e-13


@pytest.fixture(scope="module")
def solved(vec_uniform):
    name = "lap16_k4"
    E, lam, k, nev, largest, tol, _, _ = lr.problem(name)
    theta, resid, it, X = lr.twin(name, vec_uniform)
    assert lr.outcome_failures(E.matvec_ld, E.norm_inf(), X, theta, resid, nev, tol, lam) == []
    # the mutations below are visible only against residuals well above the floor of (b)
    assert np.all(resid > 1e-10), resid
    return E, lam, nev, tol, theta.copy(), resid.copy(), X.copy()


def _failures(solved, X=None, theta=None, resid=None):
    E, lam, nev, tol, th0, r0, X0 = solved
    return lr.outcome_failures(E.matvec_ld, E.norm_inf(), X0 if X is None else X, th0 if theta is None else theta, r0 if resid is None else resid, nev,
                               tol, lam)


def test_a_missed_pair_is_rejected(solved):
    """column 2 replaced by the exact eigenvector of a LATER eigenvalue (the 6th), with that eigenvalue and an honest tiny residual:
    every column is an eigenpair and the block is orthonormal, but the 3rd value is not the 3rd eigenvalue"""
    E, lam, nev, tol, theta, resid, X = solved
    m = 16
    s = lambda i: np.sin(np.arange(1, m + 1) * i * np.pi / (m + 1))  # noqa: E731
    pairs = sorted(((4 - 2 * np.cos(i * np.pi / (m + 1)) - 2 * np.cos(j * np.pi / (m + 1)), i, j) for i in range(1, m + 1) for j in range(1, m + 1)))
    lam6, i, j = pairs[5]
    v = np.outer(s(i), s(j)).ravel()
    v /= np.linalg.norm(v)
    X2, th2, r2 = X.copy(), theta.copy(), resid.copy()
    X2[:, 2], th2[2] = v, lam6
    th2[3] = max(th2[3], lam6)  # (keep the order: the index alone must catch it)
    r2[2] = float(np.linalg.norm(E.matvec(v) - lam6 * v))
    fails = _failures(solved, X=X2, theta=th2, resid=r2)
    assert "d" in fails, fails


def test_an_unnormalised_block_is_rejected(solved):
    X2 = solved[6].copy()
    X2[:, 1] *= 1.0 + 1e-9
    assert "c" in _failures(solved, X=X2)
    X3 = solved[6].copy()
    X3[:, 0] *= 2.0
    fails = _failures(solved, X=X3)
    assert "c" in fails and "b" in fails, fails


def test_two_theta_swapped_are_rejected(solved):
    th2 = solved[4].copy()
    th2[[0, 1]] = th2[[1, 0]]
    assert "d" in _failures(solved, theta=th2)


def test_an_understated_residual_is_rejected(solved):
    r2 = solved[5].copy()
    r2[0] *= 0.1
    assert "b" in _failures(solved, resid=r2)


def test_a_residual_above_the_tolerance_is_rejected(solved):
    r2 = solved[5].copy()
    r2[1] = 2.0 * solved[3]
    assert "a" in _failures(solved, resid=r2)


# ---- the pairs family and the record of the twin's runs on it (tests/golden/lobpcg_pairs_twin.json) ---------------------------------
def test_pairs_eigenvalues_are_the_dense_matrix_s():
    for largest in (False, True):
        E, lam = lr.pairs(101, 16, largest)
        A = np.zeros((101, 101))
        A[E.row, E.col] = E.val
        assert np.array_equal(A, A.T) and E.norm_inf() == np.max(np.sum(np.abs(A), axis=1)) == np.max(np.diag(A)[:-1]) + 1.0
        assert np.max(np.abs(lam - np.linalg.eigvalsh(A))) <= 1e-13 * E.norm_inf()
        wanted = lam[::-1][:16] if largest else lam[:16]
        assert (39.5 - 1e-12 <= wanted.min() and wanted.max() <= 41.0) if largest else (wanted.min() == 2.0 and wanted.max() <= 3.5 + 1e-12)
        assert (lam[::-1][16] <= 39.0 + 1e-12) if largest else (lam[16] >= 4.0)
        # the products that use the structure are Entries' own, bit for bit, and take a block
        X = np.random.default_rng(3).standard_normal((101, 3))
        Xl = X.astype(np.longdouble)
        for j in range(3):
            assert np.array_equal(E.matvec(X[:, j]), lr.Entries.matvec(E, X[:, j]))
            assert np.array_equal(E.matvec_ld(Xl)[:, j], lr.Entries.matvec_ld(E, Xl[:, j]))
        assert np.max(np.abs(lr.gram_ld(X, X, rows=7) - Xl.T @ Xl)) <= 1e-17 * 101


def test_pairs_sizes_reach_what_they_are_there_for():
    """from the header constants: the grids of the four sizes, k at the solver's limit, and wanted vectors on the first and last rows, on
    both sides of workgroup 256's edge and of each trip edge"""
    B, G = lr.grid_constants()
    text = (lr.ROOT / "include" / "spmv_abi.h").read_text()
    assert f"#define SPMV_LOBPCG_MAX_K {lr.PAIRS_K}\n" in text
    z = lr.pairs_sizes()
    grid = lambda n: max(1, min(G, -(-n // B)))  # noqa: E731  (stream_grid of csrc/common.hpp)
    assert G > 258 and grid(z["n1"]) == 257 and grid(z["n2"]) == 258  # the last-ticket loop over g steps by B = 256
    assert grid(z["n3"]) == G and z["n3"] == G * B + 1
    assert grid(z["n4"]) == G and z["n4"] > 2 * G * B and z["n4"] % 2 == 1
    assert all(n % 32 != 0 for n in z.values())  # ld = padded(n) != n
    rows = lambda n: set(np.r_[2 * lr.pairs_low(n, lr.PAIRS_K), 2 * lr.pairs_low(n, lr.PAIRS_K) + 1].tolist())  # noqa: E731
    for n in z.values():
        assert len(lr.pairs_low(n, lr.PAIRS_K)) == lr.PAIRS_K and {0, 1, n - 3, n - 2} <= rows(n)
        assert {256 * B - 1} <= rows(n) and (n == z["n1"] or 256 * B in rows(n))  # (n1's row 256 B is the one that stands alone)
    assert G * B - 1 in rows(z["n3"]) and {G * B - 1, G * B} <= rows(z["n4"])  # (n3's row G B stands alone too)
    assert {2 * G * B - 1, 2 * G * B} <= rows(z["n4"])
    assert {s for s, _, _, _ in lr.PAIRS_CASES.values()} == set(z) and set(lr.PAIRS_QUICK) | set(lr.PAIRS_EARLY) <= set(lr.PAIRS_CASES)


def test_pairs_records_are_the_twin_s(vec_uniform):
    """The two Jacobi cases at n1 and n2 are recomputed and compared bit for bit every time; SPMV_LOBPCG_RECORD_ALL=1 recomputes all
    seven (some minutes).  Every recorded pivot is a factor 10 above its threshold, so that no compared iterate hangs on a
    threshold decision."""
    records = lr.load_records()
    assert set(records) == set(lr.PAIRS_CASES)
    for name, rec in records.items():
        assert float.fromhex(rec["rank_pivot"]) >= 10 * lr.RANK_PIVOT and float.fromhex(rec["basis_pivot"]) >= 10 * lr.BASIS_PIVOT, (name, rec)
        th = lr.recorded_theta(rec)
        assert th.shape == (len(lr.EARLY), lr.PAIRS_K) and np.all(np.isfinite(th))
    for name in (lr.PAIRS_CASES if os.environ.get("SPMV_LOBPCG_RECORD_ALL") == "1" else lr.PAIRS_QUICK):
        assert lr.pairs_record(name, vec_uniform) == records[name], name
    assert all(isinstance(rec["iterations"], int) and 0 < rec["iterations"] < lr.PAIRS_MAX_ITER for rec in records.values())


def test_dependent_residual_columns_are_left_out():
    """first_dependent_column names the first column that depends on those before it; and a solve whose residual block loses rank (a
    start block with two columns that share their residual direction) goes on without that column instead of stopping"""
    rng = np.random.default_rng(4)
    B = np.linalg.qr(rng.standard_normal((50, 5)))[0]
    assert lr.first_dependent_column(B.T @ B) is None
    B[:, 3] = B[:, 1] + 1e-4 * B[:, 3]  # an angle of 1e-4: a pivot of about 1e-8
    assert lr.first_dependent_column(B.T @ B) == 3
    B[:, 0] = 0.0
    assert lr.first_dependent_column(B.T @ B) == 0
    # diag(1 .. 40): from x_0 = e_0 + e_5 and x_1 = e_1 + e_5 both residuals are along e_5 once X is projected out
    E, lam = lr.diagonal(40)
    d = E.diagonal()
    order = np.argsort(d)
    X0 = np.zeros((40, 2))
    X0[order[0], 0] = X0[order[1], 1] = 1.0
    X0[order[5], :] = 1e-3
    theta, resid, it, X = lr.lobpcg(E.matvec, X0, tol=1e-10, max_iter=50)
    assert lr.outcome_failures(E.matvec_ld, E.norm_inf(), X, theta, resid, 2, 1e-10, lam) == [], (theta, resid, it)
