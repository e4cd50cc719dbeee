"""NumPy twin of spmv_lobpcg (csrc/solver_lobpcg.hip) - TEST INFRASTRUCTURE ONLY (no GPU needed): the same algorithm in float64 with the
same thresholds, the small problems through numpy.linalg instead of the engine's Jacobi rotations; the outcome checks (a)-(d) that
every solve is held to; and the problems of tests/test_gpu_lobpcg.py with their exact eigenvalues.

    start      orthonormalise X (rank loss: ValueError "start block");  AX = A X;  Rayleigh-Ritz on X^T AX
    iteration  R = AX - X diag(theta), resid_j = ||R_j||;  active = resid > tol;  none among the first nev, or max_iter: stop
               W = M^-1 R_active;  W -= X (X^T W) twice;  orthonormalise W;  AW = A W
               P: orthonormalised with AP alike; rank loss drops it for this iteration
               S = [X P W];  GB = S^T S, GA = S^T AS symmetrised;  GB's smallest pivot (unit-diagonal scaling) < BASIS_PIVOT with P: without P
               the k lowest (largest: highest) pairs of GA c = theta GB c;  X = S C, AX = AS C, P = S C0[:, active], AP likewise
"""
from __future__ import annotations

import math

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


def orthonormalise(B, AB=None):
    """(B T, AB T) with T = diag(s) L^-T, or None at rank loss (a pivot below RANK_PIVOT)"""
    f = _unit_diagonal_factor(B.T @ B)
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
def lobpcg(matvec, X0, nev=None, largest=False, max_iter=500, tol=1e-8, precond=None):
    """matvec(v) = A v and precond(r) = M^-1 r (None: the identity) on vectors.  Returns (theta[k], resid[k], iterations, X)"""
    X = np.array(X0, dtype=np.float64, order="F")
    n, k = X.shape
    nev = k if nev is None else nev
    mv = lambda B: np.column_stack([matvec(np.ascontiguousarray(B[:, j])) for j in range(B.shape[1])])  # noqa: E731
    o = orthonormalise(X)
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
        active = np.flatnonzero(resid > tol)
        if not np.any(active < nev) or it >= max_iter:
            return theta, resid, it, X
        W = R[:, active] if precond is None else np.column_stack([precond(np.ascontiguousarray(R[:, j])) for j in active])
        for _ in range(2):
            W = W - X @ (X.T @ W)
        o = orthonormalise(W)
        if o is None:
            raise ValueError(f"the preconditioned residuals lost rank at iteration {it}")
        W = o[0]
        AW = mv(W)
        use_p = P is not None
        if use_p:
            o = orthonormalise(P, AP)
            if o is None:
                use_p = False
            else:
                P, AP = o
        while True:
            S = np.column_stack([X, P, W] if use_p else [X, W])
            AS = np.column_stack([AX, AP, AW] if use_p else [AX, AW])
            GA = S.T @ AS
            g = generalised(0.5 * (GA + GA.T), S.T @ S)
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
    Xl = X.astype(np.longdouble)
    if not float(np.max(np.abs(Xl.T @ Xl - np.eye(k, dtype=np.longdouble)))) <= 1e-12:
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
