"""CPU-side checks of the LOBPCG twin (tests/lobpcg_ref.py) and of the outcome checks that tests/test_gpu_lobpcg.py holds spmv_lobpcg to:
the twin meets (a)-(d) on every problem of the GPU file within max_iter, and the checks reject wrong answers - a missed pair, an
unnormalised X, two theta swapped, a residual understated by a factor of 10.

The three preconditioned 64 x 64 problems run here with M = I: the engine's Chebyshev polynomial and AMG cycle need the device (the GPU
file hands them to the twin as its M^-1).  The problem, the block and the checks are the same."""
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
