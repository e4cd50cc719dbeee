"""NumPy twin of spmv_lobpcg (csrc/solver_lobpcg.hip) - TEST INFRASTRUCTURE ONLY (no GPU needed): the same algorithm in float64 with the
same thresholds, the small problems through numpy.linalg instead of the engine's Jacobi rotations; the outcome checks (a)-(d) that
every solve is held to; and the problems of tests/test_gpu_lobpcg.py with their exact eigenvalues.  The last section is the pairs
family (k = 16 at sizes past 256 workgroups and past one and two trips of the grid) and the record of the twin's runs on it:

    python tests/lobpcg_ref.py --record     writes tests/golden/lobpcg_pairs_twin.json (some minutes: one BLAS thread)
    python tests/lobpcg_ref.py --one-ulp    how far theta of the early iterates moves when the start block moves by one ulp

    start      orthonormalise X (rank loss: ValueError "start block");  AX = A X;  Rayleigh-Ritz on X^T AX
    iteration  R = AX - X diag(theta), resid_j = ||R_j||;  active = resid > tol;  none among the first nev, or max_iter: stop
               W = M^-1 R_active;  W -= X (X^T W) twice;  orthonormalise W (rank loss: without the first dependent column, and so on);  AW = A W
               P: orthonormalised with AP alike; rank loss drops it for this iteration
               S = [X P W];  GB = S^T S, GA = S^T AS symmetrised;  GB's smallest pivot (unit-diagonal scaling) < BASIS_PIVOT with P: without P
               the k lowest (largest: highest) pairs of GA c = theta GB c;  X = S C, AX = AS C, P = S C0[:, active], AP likewise
"""
from __future__ import annotations

import contextlib
import json
import math
import os
import re
import sys
import time
from pathlib import Path

import numpy as np

RANK_PIVOT = 1e-6   # kLobpcgRankPivot
BASIS_PIVOT = 1e-4  # kLobpcgBasisPivot


# ---- the small problems ----------------------------------------------------------------------------------------------------------
def _unit_diagonal_factor(G):
    """(s, L, smallest pivot) with diag(s) G diag(s) = L L^T of unit diagonal, the pivot before its square root; None at rank loss"""
    d = np.diag(G)
    if not (np.all(np.isfinite(G)) and np.all(d > 0)):
        return None
    s = 1.0 / np.sqrt(d)
    Gs = s[:, None] * G * s[None, :]
    np.fill_diagonal(Gs, 1.0)
    try:
        L = np.linalg.cholesky(Gs)
    except np.linalg.LinAlgError:
        return None
    return s, L, float(np.min(np.diag(L) ** 2))


def first_dependent_column(G):
    """the first column of a block with Gram matrix G whose pivot in the unit-diagonal factorisation is below RANK_PIVOT (or whose
    diagonal entry is not positive and finite); None: the block has full rank"""
    d = np.diag(G)
    for i in range(len(d)):
        if not (d[i] > 0 and np.isfinite(d[i])):
            return i
    s = 1.0 / np.sqrt(d)
    Gs = s[:, None] * G * s[None, :]
    np.fill_diagonal(Gs, 1.0)
    L = np.zeros_like(Gs)
    for j in range(len(d)):
        p = Gs[j, j] - L[j, :j] @ L[j, :j]
        if not p >= RANK_PIVOT:
            return j
        L[j, j] = np.sqrt(p)
        L[j + 1:, j] = (Gs[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return None


def orthonormalise(B, AB=None, seen=None):
    """(B T, AB T) with T = diag(s) L^-T, or None at rank loss (a pivot below RANK_PIVOT); the smallest pivot is appended to `seen`"""
    f = _unit_diagonal_factor(B.T @ B)
    if seen is not None:
        seen.append(0.0 if f is None else f[2])
    if f is None or f[2] < RANK_PIVOT:
        return None
    s, L, _ = f
    T = s[:, None] * np.linalg.inv(L).T
    return B @ T, (None if AB is None else AB @ T)


def generalised(GA, GB):
    """(theta ascending, C with C^T GB C = I, smallest pivot of the scaled GB) or None"""
    f = _unit_diagonal_factor(GB)
    if f is None:
        return None
    s, L, piv = f
    Li = np.linalg.inv(L)
    M = Li @ (s[:, None] * GA * s[None, :]) @ Li.T
    th, Z = np.linalg.eigh(0.5 * (M + M.T))
    return th, s[:, None] * (Li.T @ Z), piv


# ---- the solver ------------------------------------------------------------------------------------------------------------------
def lobpcg(matvec, X0, nev=None, largest=False, max_iter=500, tol=1e-8, precond=None, stats=None):
    """matvec(v) = A v and precond(r) = M^-1 r (None: the identity) on vectors.  Returns (theta[k], resid[k], iterations, X).
    stats (a dict, optional) receives three lists indexed by the iteration count t: "theta" (theta after t iterations), "rank_pivot" and
    "basis_pivot" (the smallest orthonormalisation pivot - the start block's counts for t = 0 - and the smallest pivot of the scaled GB
    that iteration t + 1 saw on its way, whatever it decided on them)"""
    X = np.array(X0, dtype=np.float64, order="F")
    n, k = X.shape
    nev = k if nev is None else nev
    mv = lambda B: np.column_stack([matvec(np.ascontiguousarray(B[:, j])) for j in range(B.shape[1])])  # noqa: E731
    rank_seen, basis_seen = [], []
    o = orthonormalise(X, seen=rank_seen)
    if o is None:
        raise ValueError("start block")
    X = o[0]
    AX = mv(X)
    G = X.T @ AX
    th, Z = np.linalg.eigh(0.5 * (G + G.T))
    if largest:
        th, Z = th[::-1], Z[:, ::-1]
    X, AX, theta = X @ Z, AX @ Z, th.copy()
    P = AP = None
    it = 0
    while True:
        R = AX - X * theta[None, :]
        resid = np.sqrt(np.sum(R * R, axis=0))
        if not (np.all(np.isfinite(theta)) and np.all(np.isfinite(resid))):
            raise ValueError("theta or a residual is not finite")
        if stats is not None:
            stats.setdefault("theta", []).append(theta.copy())
            if it > 0:
                stats.setdefault("rank_pivot", []).append(min(rank_seen))
                stats.setdefault("basis_pivot", []).append(min(basis_seen))
                rank_seen, basis_seen = [], []
        active = np.flatnonzero(resid > tol)
        if not np.any(active < nev) or it >= max_iter:
            return theta, resid, it, X
        W = R[:, active] if precond is None else np.column_stack([precond(np.ascontiguousarray(R[:, j])) for j in active])
        for _ in range(2):
            W = W - X @ (X.T @ W)
        o = orthonormalise(W, seen=rank_seen)
        if o is None:
            # rank loss among the residuals: the first column that depends on those before it is left out of this iteration, and so on
            G = W.T @ W
            keep = list(range(len(active)))
            while keep:
                bad = first_dependent_column(G[np.ix_(keep, keep)])
                if bad is None:
                    break
                del keep[bad]
            o = orthonormalise(W[:, keep]) if keep else None
            if o is None:
                raise ValueError(f"the preconditioned residuals lost rank at iteration {it}")
            active = active[keep]
        W = o[0]
        AW = mv(W)
        use_p = P is not None
        if use_p:
            o = orthonormalise(P, AP, seen=rank_seen)
            if o is None:
                use_p = False
            else:
                P, AP = o
        while True:
            S = np.column_stack([X, P, W] if use_p else [X, W])
            AS = np.column_stack([AX, AP, AW] if use_p else [AX, AW])
            GA = S.T @ AS
            g = generalised(0.5 * (GA + GA.T), S.T @ S)
            basis_seen.append(0.0 if g is None else g[2])
            if (g is None or g[2] < BASIS_PIVOT) and use_p:
                use_p = False
                continue
            break
        if g is None:
            raise ValueError(f"the basis [X W] lost rank at iteration {it}")
        th, C, _ = g
        if largest:
            th, C = th[::-1], C[:, ::-1]
        C = C[:, :k]
        C0 = C.copy()
        C0[:k, :] = 0.0
        X, AX, P, AP, theta = S @ C, AS @ C, S @ C0[:, active], AS @ C0[:, active], th[:k].copy()
        it += 1


# ---- the outcome checks: what every solve is held to, for the first nev columns -------------------------------------------------------
def outcome_failures(apply_ld, anorm, X, theta, resid, nev, tol, lam, largest=False):
    """The names of the checks a result misses (empty: it passes).  apply_ld(v) = A v in np.longdouble, anorm = ||A||_inf, lam = the
    exact eigenvalues in the order asked for (ascending; largest: descending), at least nev of them.
      (a) resid_j <= tol
      (b) | ||A x_j - theta_j x_j|| recomputed in long double - resid_j | <= 1e-12 ||A||_inf
      (c) ||X^T X - I||_max <= 1e-12 over all k columns
      (d) theta in order, and |theta_j - lam_j| <= max(resid_j, 1e-12 ||A||_inf): some eigenvalue of a symmetric matrix lies within the
          residual of theta_j, and the j-th index catches a missed pair"""
    X = np.asarray(X, dtype=np.float64)
    theta, resid = np.asarray(theta, dtype=np.float64), np.asarray(resid, dtype=np.float64)
    k = X.shape[1]
    fails = []
    if not np.all(resid[:nev] <= tol):
        fails.append("a")
    for j in range(nev):
        x = X[:, j].astype(np.longdouble)
        r = apply_ld(x) - np.longdouble(theta[j]) * x
        true = float(np.sqrt(np.sum(r * r)))
        if not abs(true - resid[j]) <= 1e-12 * anorm:
            fails.append("b")
            break
    if not float(np.max(np.abs(gram_ld(X, X) - np.eye(k, dtype=np.longdouble)))) <= 1e-12:
        fails.append("c")
    d = np.diff(theta)
    in_order = np.all(d <= 0) if largest else np.all(d >= 0)
    close = all(abs(theta[j] - lam[j]) <= max(resid[j], 1e-12 * anorm) for j in range(nev))
    if not (in_order and close):
        fails.append("d")
    return fails


# ---- matrices as entry lists (row, column, value), their products and norms ----------------------------------------------------------
class Entries:
    def __init__(self, n, row, col, val):
        order = np.lexsort((col, row))
        self.n = int(n)
        self.row, self.col, self.val = np.asarray(row, np.int64)[order], np.asarray(col, np.int64)[order], np.asarray(val, np.float64)[order]
        self.val_ld = self.val.astype(np.longdouble)

    def matvec(self, x):
        return np.bincount(self.row, weights=self.val * x[self.col], minlength=self.n)

    def matvec_ld(self, x):
        y = np.zeros(self.n, dtype=np.longdouble)
        np.add.at(y, self.row, self.val_ld * x[self.col])
        return y

    def norm_inf(self):
        return float(np.max(np.bincount(self.row, weights=np.abs(self.val), minlength=self.n)))

    def csr(self):
        rp = np.zeros(self.n + 1, dtype=np.int32)
        np.cumsum(np.bincount(self.row, minlength=self.n), out=rp[1:])
        return rp, self.col.astype(np.int32), self.val.copy()

    def diagonal(self):
        d = np.zeros(self.n)
        m = self.row == self.col
        np.add.at(d, self.row[m], self.val[m])
        return d


def laplacian(m):
    """the 5-point Laplacian on an m x m grid (Dirichlet) and its eigenvalues 4 - 2 cos(i pi / (m+1)) - 2 cos(j pi / (m+1)), ascending"""
    idx = np.arange(m * m).reshape(m, m)
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [np.full(m * m, 4.0)]
    for a, b in ((idx[:, :-1], idx[:, 1:]), (idx[:-1, :], idx[1:, :])):
        rows += [a.ravel(), b.ravel()]
        cols += [b.ravel(), a.ravel()]
        vals += [np.full(a.size, -1.0)] * 2
    c = 2.0 * np.cos(np.arange(1, m + 1) * math.pi / (m + 1))
    lam = np.sort((4.0 - c[:, None] - c[None, :]).ravel())
    return Entries(m * m, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)), lam


def dense12():
    rng = np.random.default_rng(12)
    B = rng.standard_normal((12, 12))
    B = 0.5 * (B + B.T)
    r, c = np.indices((12, 12))
    return Entries(12, r.ravel(), c.ravel(), B.ravel()), np.linalg.eigvalsh(B)


def diagonal(n=40):
    d = 1.0 + ((np.arange(n) * 17) % n).astype(np.float64)  # 1 .. n, shuffled
    return Entries(n, np.arange(n), np.arange(n), d), np.sort(d)


def tridiagonal(n=4099):
    i = np.arange(n)
    E = Entries(n, np.r_[i, i[:-1], i[1:]], np.r_[i, i[1:], i[:-1]], np.r_[1.0 + i, np.full(2 * (n - 1), -0.25)])
    return E, sturm_lowest(1.0 + i, np.full(n - 1, -0.25), 8)


def sturm_lowest(d, e, count):
    """the `count` lowest eigenvalues of the symmetric tridiagonal matrix (d, e) by bisection on the Sturm count (the number of negative
    pivots of T - x I), all of them at once"""
    d, e2 = np.asarray(d, np.float64), np.asarray(e, np.float64) ** 2
    r = np.r_[0.0, np.abs(e)] + np.r_[np.abs(e), 0.0]
    lo, hi = np.full(count, float(np.min(d - r))), np.full(count, float(np.max(d + r)))
    want = np.arange(1, count + 1)
    tiny = np.finfo(np.float64).tiny
    for _ in range(120):
        mid = 0.5 * (lo + hi)
        q = d[0] - mid
        neg = (q < 0).astype(np.int64)
        for i in range(1, len(d)):
            q = d[i] - mid - e2[i - 1] / np.where(q == 0.0, tiny, q)
            neg += q < 0
        below = neg >= want
        hi = np.where(below, mid, hi)
        lo = np.where(below, lo, mid)
    return 0.5 * (lo + hi)


# ---- the problems of tests/test_gpu_lobpcg.py ----------------------------------------------------------------------------------------
# name -> (matrix maker, k, nev, largest, tol, max_iter, preconditioner: None, "jacobi", "chebyshev", "amg", "amg_sa")
PROBLEMS = {
    "dense12_smallest": (dense12, 4, 4, False, 1e-8, 50, None),
    "dense12_largest": (dense12, 4, 4, True, 1e-8, 50, None),
    "diagonal_unit_start": (diagonal, 3, 3, False, 1e-8, 50, None),
    "lap16_k1": (lambda: laplacian(16), 1, 1, False, 1e-8, 400, None),
    "lap16_k4": (lambda: laplacian(16), 4, 4, False, 1e-8, 400, None),
    "lap32_k8": (lambda: laplacian(32), 8, 8, False, 1e-8, 500, None),
    "lap32_k8_nev6": (lambda: laplacian(32), 8, 6, False, 1e-8, 500, None),
    "lap32_k8_largest": (lambda: laplacian(32), 8, 8, True, 1e-8, 500, None),
    "lap33_k5_multiple": (lambda: laplacian(33), 5, 5, False, 1e-8, 500, None),
    "tri4099_jacobi": (tridiagonal, 6, 6, False, 1e-9, 100, "jacobi"),
    "lap64_chebyshev": (lambda: laplacian(64), 8, 6, False, 1e-8, 200, "chebyshev"),
    "lap64_amg": (lambda: laplacian(64), 8, 6, False, 1e-8, 200, "amg"),
    "lap64_amg_sa": (lambda: laplacian(64), 8, 6, False, 1e-8, 200, "amg_sa"),
}
LAPLACIANS = ("lap16_k1", "lap16_k4", "lap32_k8", "lap32_k8_nev6", "lap32_k8_largest", "lap33_k5_multiple")

_made = {}


def problem(name):
    """(Entries, eigenvalues in the order asked for, k, nev, largest, tol, max_iter, preconditioner), made once"""
    if name not in _made:
        make, k, nev, largest, tol, max_iter, pre = PROBLEMS[name]
        E, lam = make()
        lam = np.asarray(lam)
        _made[name] = (E, lam[::-1].copy() if largest else lam, k, nev, largest, tol, max_iter, pre)  # (the makers of these give the whole spectrum)
    return _made[name]


def start_block(name, vec_uniform):
    """the start block of a problem, (n, k): spmv_gen_vec_uniform's twin over n * k entries with seed 1, column-major; unit vectors at
    the k smallest diagonal entries for the diagonal problem"""
    E, _, k = problem(name)[:3]
    if name == "diagonal_unit_start":
        X = np.zeros((E.n, k))
        X[np.argsort(E.diagonal())[:k], np.arange(k)] = 1.0
        return X
    return np.asfortranarray(vec_uniform(E.n * k, seed=1).reshape(k, E.n).T)


_twin = {}


def twin(name, vec_uniform, precond=None):
    """the twin's (theta, resid, iterations, X) on a problem, run once (precond: the callable M^-1 of a preconditioned problem)"""
    if name not in _twin:
        E, _, k, nev, largest, tol, max_iter, pre = problem(name)
        if pre == "jacobi":
            dinv = 1.0 / E.diagonal()
            precond = lambda r: dinv * r  # noqa: E731
        _twin[name] = lobpcg(E.matvec, start_block(name, vec_uniform), nev=nev, largest=largest, max_iter=max_iter, tol=tol, precond=precond)
    return _twin[name]


# ---- the pairs family: an exact spectrum at any size, wanted vectors on chosen rows ---------------------------------------------------
# Kept out of PROBLEMS: at these sizes the twin takes from seconds to a minute, so the GPU tests read what they need from it out of
# tests/golden/lobpcg_pairs_twin.json (`python tests/lobpcg_ref.py --record` writes it; tests/test_lobpcg_ref.py holds it to the twin).
ROOT = Path(__file__).resolve().parent.parent
RECORD_PATH = ROOT / "tests" / "golden" / "lobpcg_pairs_twin.json"
PAIRS_K = 16
PAIRS_TOL = 1e-8
PAIRS_MAX_ITER = 200
EARLY = (0, 1, 2, 3)  # the max_iter values whose theta the record holds


def grid_constants():
    """kBlock and kMaxGrid as csrc/common.hpp defines them"""
    text = (ROOT / "arm-spmv_amd" / "csrc" / "common.hpp").read_text()
    vals = {}
    for name, expr in re.findall(r"constexpr int (k\w+)\s*=\s*([^;]+);", text):
        try:
            vals[name] = int(eval(expr, {"__builtins__": {}}, dict(vals)))
        except Exception:
            pass
    return vals["kBlock"], vals["kMaxGrid"]


def pairs_sizes():
    """n1: 257 workgroups (the last-ticket sum's second step);  n2: 258;  n3: a full grid and one row on the second trip;  n4: a third
    trip and an odd tail"""
    B, G = grid_constants()
    return {"n1": 256 * B + 1, "n2": 257 * B + 1, "n3": G * B + 1, "n4": 2 * G * B + 2051}


class PairsEntries(Entries):
    """Entries of a pairs() matrix with products that use its structure (the same sums in the same order as Entries', see
    tests/test_lobpcg_ref.py); matvec_ld also takes a block of columns"""

    def matvec(self, x):
        return self._apply(self.diagonal_values, x)

    def matvec_ld(self, x):
        return self._apply(self.diagonal_values.astype(np.longdouble), x)

    def _apply(self, d, x):
        y = (d * x.T).T
        m = self.n - 1
        y[0:m:2] -= x[1:m:2]
        y[1:m:2] -= x[0:m:2]
        return y


def pairs_low(n, k):
    """the pairs whose eigenvalues are wanted, sorted: on the first and last rows, on both sides of workgroup 256's edge, on both sides
    of each trip edge, and spread evenly where the size has no such rows"""
    B, G = grid_constants()
    npairs = (n - 1) // 2
    low = []
    for r in (0, n - 3, G * B - 2, G * B, 2 * G * B - 2, 2 * G * B, 256 * B - 2, 256 * B, 254, G * B + 2, 2 * G * B + 2, 256 * B + 254):
        if 0 <= r // 2 < npairs and r // 2 not in low:
            low.append(r // 2)
    for p in np.linspace(0, npairs - 1, 2 * k + 1).astype(np.int64)[1::2]:
        if int(p) not in low:
            low.append(int(p))
    return np.array(sorted(low[:k]), dtype=np.int64)


def pairs(n, k, largest=False):
    """Rows 2p and 2p+1 form the block [[a_p, -1], [-1, a_p]] (p < (n-1)/2), row n-1 stands alone with 20: the eigenvalues are exactly
    a_p - 1, a_p + 1 and 20, and ||A||_inf = max(a) + 1.  a is 10 + 10 u (u uniform: a continuous unwanted spectrum; a constant one makes
    the residuals lose rank within three iterations) except on the k pairs of pairs_low, where it is 3.0 .. 3 + 0.1 (k-1) shuffled
    (largest: 40 - that).  Returns (PairsEntries, every eigenvalue ascending)"""
    assert n % 2 == 1 and (n - 1) // 2 >= k
    npairs = (n - 1) // 2
    a = 10.0 + 10.0 * np.random.default_rng(7).random(npairs)
    shuffled = 0.1 * np.random.default_rng(0).permutation(k)
    a[pairs_low(n, k)] = 40.0 - shuffled if largest else 3.0 + shuffled
    d = np.r_[np.repeat(a, 2), 20.0]
    i, p = np.arange(n), 2 * np.arange(npairs)
    E = PairsEntries(n, np.r_[i, p, p + 1], np.r_[i, p + 1, p], np.r_[d, np.full(2 * npairs, -1.0)])
    E.diagonal_values = d
    return E, np.sort(np.r_[a - 1.0, a + 1.0, 20.0])


# name -> (size, nev, largest, preconditioner); k = PAIRS_K, tol = PAIRS_TOL, max_iter = PAIRS_MAX_ITER
PAIRS_CASES = {
    "pairs_n1_nev16_jacobi": ("n1", 16, False, "jacobi"),
    "pairs_n1_nev12": ("n1", 12, False, None),
    "pairs_n2_nev12_jacobi": ("n2", 12, False, "jacobi"),
    "pairs_n2_nev12_largest": ("n2", 12, True, None),
    "pairs_n3_nev12_jacobi": ("n3", 12, False, "jacobi"),
    "pairs_n4_nev12_jacobi": ("n4", 12, False, "jacobi"),
    "pairs_n4_nev16_jacobi": ("n4", 16, False, "jacobi"),
}
PAIRS_QUICK = ("pairs_n1_nev16_jacobi", "pairs_n2_nev12_jacobi")  # the records that tests/test_lobpcg_ref.py recomputes every time
# the cases whose early iterates are compared.  n1's is there for its last workgroup: it holds the row that stands alone and nothing else, a
# row whose residual vanishes at convergence, so only an iterate on the way shows whether that workgroup's partial sum is added
PAIRS_EARLY = ("pairs_n1_nev16_jacobi", "pairs_n2_nev12_jacobi", "pairs_n3_nev12_jacobi", "pairs_n4_nev12_jacobi")

_pairs_made = {}


def pairs_problem(name):
    """(PairsEntries, eigenvalues in the order asked for, k, nev, largest, tol, max_iter, preconditioner); a matrix is made once"""
    size, nev, largest, pre = PAIRS_CASES[name]
    n = pairs_sizes()[size]
    if (n, largest) not in _pairs_made:
        E, lam = pairs(n, PAIRS_K, largest)
        _pairs_made[(n, largest)] = (E, lam[::-1].copy() if largest else lam)
    E, lam = _pairs_made[(n, largest)]
    return E, lam, PAIRS_K, nev, largest, PAIRS_TOL, PAIRS_MAX_ITER, pre


def pairs_start(n, vec_uniform):
    """the start block (n, PAIRS_K): spmv_gen_vec_uniform's twin over n * k entries with seed 1, column-major"""
    return np.asfortranarray(vec_uniform(n * PAIRS_K, seed=1).reshape(PAIRS_K, n).T)


def pairs_twin(name, vec_uniform, max_iter=None, X0=None, stats=None):
    """the twin on a pairs case: (theta, resid, iterations, X)"""
    E, _, k, nev, largest, tol, limit, pre = pairs_problem(name)
    dinv = 1.0 / E.diagonal_values
    return lobpcg(E.matvec, pairs_start(E.n, vec_uniform) if X0 is None else X0, nev=nev, largest=largest, max_iter=limit if max_iter is None else max_iter,
                  tol=tol, precond=(lambda r: dinv * r) if pre == "jacobi" else None, stats=stats)


def _one_blas_thread():
    """a record is compared bit for bit, and the order in which a threaded BLAS adds up B^T B depends on its thread count: threadpoolctl
    holds it to one, or, where that is not installed, the process was started with OMP_NUM_THREADS=1 (tests/conftest.py sets it); with
    neither no record is made"""
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:
        if os.environ.get("OMP_NUM_THREADS") != "1":
            raise RuntimeError("a twin record needs a one-thread BLAS: install threadpoolctl or start python with OMP_NUM_THREADS=1")
        return contextlib.nullcontext()
    return threadpool_limits(limits=1, user_api="blas")


def pairs_record(name, vec_uniform):
    """what the GPU tests need from the twin on one case: its iteration count, theta (all k, float.hex) after 0 .. 3 iterations and the
    smallest pivots those three iterations saw.  From the twin alone, never from the GPU; a twin that refuses the case raises"""
    E, _, k, nev, largest, tol, limit, pre = pairs_problem(name)
    stats = {}
    with _one_blas_thread():
        _, resid, it, _ = pairs_twin(name, vec_uniform, stats=stats)
    t = len(EARLY)
    assert it < limit and np.all(resid[:nev] <= tol) and len(stats["basis_pivot"]) >= t - 1, (name, it, resid)
    return {"n": E.n, "k": k, "nev": nev, "largest": largest, "precond": pre or "none", "iterations": int(it),
            "theta": [[float(v).hex() for v in stats["theta"][i]] for i in EARLY],
            "rank_pivot": float(min(stats["rank_pivot"][:t - 1])).hex(), "basis_pivot": float(min(stats["basis_pivot"][:t - 1])).hex()}


def load_records():
    with open(RECORD_PATH) as f:
        return json.load(f)


def recorded_theta(rec):
    """theta of a record as an array (len(EARLY), k)"""
    return np.array([[float.fromhex(v) for v in row] for row in rec["theta"]])


def gram_ld(U, V, rows=2048):
    """U^T V in long double, added up over chunks of rows (NumPy has no fast long-double product: a chunk stays in the cache)"""
    G = np.zeros((U.shape[1], V.shape[1]), dtype=np.longdouble)
    for lo in range(0, U.shape[0], rows):
        G += np.ascontiguousarray(U[lo:lo + rows].T, dtype=np.longdouble) @ np.asarray(V[lo:lo + rows], dtype=np.longdouble)
    return G


def ritz_failure(E, X, theta):
    """check (e), over all k columns in long double: max |X^T A X - diag(theta)| <= 1e-12 ||A||_inf.  Returns the excess as text, or None"""
    Xl = np.asarray(X, dtype=np.longdouble)
    err = float(np.max(np.abs(gram_ld(Xl, E.matvec_ld(Xl)) - np.diag(np.asarray(theta, dtype=np.longdouble)))))
    return None if err <= 1e-12 * E.norm_inf() else f"e: max |X^T A X - diag(theta)| = {err:.3e} > 1e-12 ||A||_inf = {1e-12 * E.norm_inf():.3e}"


def _vec_uniform():
    sys.path.insert(0, str(ROOT))
    from __graft_entry__ import load_package

    return load_package().synth.vec_uniform


def main(argv):
    vec_uniform = _vec_uniform()
    if argv == ["--record"]:
        records = {}
        for name in PAIRS_CASES:
            t0 = time.perf_counter()
            records[name] = pairs_record(name, vec_uniform)
            print(f"{name}: {records[name]['iterations']} iterations, {time.perf_counter() - t0:.1f} s", flush=True)
        with open(RECORD_PATH, "w") as f:
            json.dump(records, f, indent=1)
            f.write("\n")
    elif argv == ["--one-ulp"]:
        # how far theta after 0 .. 3 iterations moves when every entry of the start block moves by one ulp: the yardstick of the
        # early-iterate gate of tests/test_gpu_lobpcg.py
        for name in PAIRS_EARLY:
            E = pairs_problem(name)[0]
            X0 = pairs_start(E.n, vec_uniform)
            a, b = {}, {}
            pairs_twin(name, vec_uniform, max_iter=EARLY[-1], X0=X0, stats=a)
            pairs_twin(name, vec_uniform, max_iter=EARLY[-1], X0=np.nextafter(X0, np.inf), stats=b)
            a, b = a["theta"], b["theta"]
            moved = [float(np.max(np.abs(u - v))) for u, v in zip(a, b)]
            print(f"{name}: ||A||_inf = {E.norm_inf()}, theta moved by " + ", ".join(f"{m:.2e}" for m in moved), flush=True)
    else:
        raise SystemExit("usage: python tests/lobpcg_ref.py --record | --one-ulp")


if __name__ == "__main__":
    main(sys.argv[1:])
