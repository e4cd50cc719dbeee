"""NumPy twin of the Chebyshev polynomial preconditioner and of the Lanczos spectrum estimate (csrc/chebyshev.hip): the definition
that include/spmv_abi.h states, restated.  tests/test_chebyshev_ref.py holds it to facts of its own on the CPU (a closed form, a
contraction bound, definiteness, mutations); tests/test_gpu_chebyshev.py holds the engine to it.

The operator.  s_i = 1 / a_ii (scaled: duplicates summed) or 1; B = diag(s) A; 0 < lmin < lmax.
    theta = (lmax + lmin) / 2;  delta = (lmax - lmin) / 2;  sigma = theta / delta;  rho_0 = 1 / sigma;  c0 = 1 / theta
    for k = 1..d:  rho_k = 1 / (2 sigma - rho_{k-1});  c1_k = rho_k rho_{k-1};  c2_k = 2 rho_k / delta
    d = c0 (s .* r);  z = d;  t = r;      for k = 1..d:  w = A d;  t = t - w;  d = c1_k d + c2_k (s .* t);  z = z + d
z = p_d(B) diag(s) r.  The start and the d terms are d + 1 corrections of the Chebyshev iteration, so p_d has degree d and the
residual polynomial is the Chebyshev polynomial of degree d + 1:  1 - lambda p_d(lambda) = T_{d+1}((theta - lambda) / delta) /
T_{d+1}(sigma)  (with T_d in its place the closed form is off by O(1): tests/test_chebyshev_ref.py checks both).

Lanczos: m steps without reorthogonalisation on C = diag(sqrt s) A diag(sqrt s) from a given v_0 (normalised here):
    w = C v_j;  alpha_j = v_j . w;  w -= alpha_j v_j + beta_j v_{j-1};  beta_{j+1} = ||w||;  v_{j+1} = w / beta_{j+1}
beta_{j+1} <= 2^-44 max(|alpha|, beta seen so far) ends the run.  The extreme Ritz values by bisection on the Sturm count."""
import numpy as np

import ilu0_ref as ir
import solver_ref as sr

LD = np.longdouble
MUTATIONS = ("rho", "c2", "t", "s_on_w")
BREAKDOWN = 2.0**-44
# float64 twin against the closed form in longdouble on diagonal matrices (tests/test_chebyshev_ref.py measures and asserts these):
# the largest relative deviation of z_i / r_i over 257 values across [lmin, lmax] and 16 below lmin, bounds DIAGONAL_BOUNDS,
# with r = default_rng(5).uniform(0.5, 1.5).  The yardstick of the GPU gate: the engine is held to 8 E_d
DIAGONAL_BOUNDS = (0.05, 1.97)
E_D = {1: 5.3e-15, 2: 2.1e-15, 5: 2.5e-15, 9: 1.5e-15, 16: 1.5e-15}


# ---- the coefficient table --------------------------------------------------------------------------------------------------------
def coefficients(degree, lmin, lmax, kind=np.float64, mutate=None):
    """(c0, c1[degree], c2[degree]); every line one rounded operation in `kind`"""
    f = kind
    lmin, lmax, two, one = f(lmin), f(lmax), f(2.0), f(1.0)
    total = lmax + lmin
    theta = total / two
    diff = lmax - lmin
    delta = diff / two
    sigma = theta / delta
    rho = one / sigma
    c0 = one / theta
    c1, c2 = np.zeros(degree, dtype=kind), np.zeros(degree, dtype=kind)
    for k in range(degree):
        twice = two * sigma
        den = twice - rho
        nxt = one / den
        c1[k] = nxt * rho
        num = (one if mutate == "c2" else two) * nxt
        c2[k] = num / delta
        if mutate != "rho":
            rho = nxt
    return c0, c1, c2


def apply(mv, s, r, c0, c1, c2, mutate=None):
    """z = M^-1 r; mv: the product with A; s: the scaling vector or None"""
    one = s if s is not None else 1.0
    d = c0 * (one * r)
    z = d.copy()
    t = r.copy()
    for k in range(len(c1)):
        w = mv(d)
        if mutate == "s_on_w":
            t = t - one * w
            d = c1[k] * d + c2[k] * t
        else:
            if mutate != "t":
                t = t - w
            d = c1[k] * d + c2[k] * (one * t)
        z = z + d
    return z


def smooth(mv, s, b, x, c0, c1, c2):
    """x + M^-1 (b - A x): one smoothing step"""
    return x + apply(mv, s, b - mv(x), c0, c1, c2)


# ---- diagonal, row bound ------------------------------------------------------------------------------------------------------------
def inverse_diagonal(n, rp, cc, cv):
    """s_i = 1 / a_ii, duplicates summed; a zero or missing entry raises"""
    rows = np.repeat(np.arange(n), np.diff(rp))
    d = np.zeros(n)
    on = rows == np.asarray(cc)
    np.add.at(d, rows[on], np.asarray(cv)[on])
    if np.any(d == 0.0):
        raise ValueError("a zero or missing diagonal entry")
    return 1.0 / d


def row_bound(n, rp, cc, cv, s=None):
    """max_i |s_i| sum_j |a_ij| over every stored entry: the infinity norm of B"""
    sums = np.zeros(n)
    np.add.at(sums, np.repeat(np.arange(n), np.diff(rp)), np.abs(cv))
    if s is not None:
        sums = np.abs(s) * sums
    return float(sums.max()) if n else 0.0


# ---- the closed form on a diagonal matrix -----------------------------------------------------------------------------------------
def chebyshev_t(d, x):
    """T_d(x) by the three-term recurrence, in x's precision"""
    t0, t1 = np.ones_like(x), x
    if d == 0:
        return t0
    for _ in range(d - 1):
        t0, t1 = t1, 2 * x * t1 - t0
    return t1


def closed_form(lam, d, lmin, lmax):
    """p_d(lambda) = (1 - T_{d+1}((theta - lambda) / delta) / T_{d+1}(sigma)) / lambda in longdouble: z_i / r_i on diag(lambda),
    unscaled, after d products"""
    lam, lmin, lmax = np.asarray(lam, dtype=LD), LD(lmin), LD(lmax)
    theta, delta = (lmax + lmin) / 2, (lmax - lmin) / 2
    sigma = theta / delta
    return (1 - chebyshev_t(d + 1, (theta - lam) / delta) / chebyshev_t(d + 1, np.asarray(sigma))) / lam


def contraction(d, lmin, lmax):
    """1 / T_{d+1}(sigma): what one application contracts the error by, at most, in the 2-norm (symmetric A, exact bounds)"""
    theta, delta = (LD(lmax) + LD(lmin)) / 2, (LD(lmax) - LD(lmin)) / 2
    return float(1 / chebyshev_t(d + 1, np.asarray(theta / delta)))


def diagonal_family(lmin, lmax):
    """257 values across [lmin, lmax] and 16 below lmin (down to lmin / 64)"""
    return np.concatenate([np.linspace(lmin, lmax, 257), lmin * np.linspace(1.0 / 64, 1.0, 16, endpoint=False)])


# ---- Lanczos ------------------------------------------------------------------------------------------------------------------------
def sturm_count(a, b, x, tiny):
    """eigenvalues below x of the symmetric tridiagonal matrix (a; b off the diagonal)"""
    count, q = 0, 1.0
    for i in range(len(a)):
        q = (a[i] - x) - (b[i - 1] * b[i - 1] / q if i > 0 else 0.0)
        if q == 0.0:
            q = -tiny
        if q < 0.0:
            count += 1
    return count


def tridiagonal_eigenvalue(a, b, k):
    """the k-th eigenvalue from below by bisection, to 2 ulp of the largest |value| the Gershgorin discs allow (the engine's steps)"""
    a, b = [float(v) for v in a], [float(v) for v in b]
    m = len(a)
    if m == 1:
        return a[0]
    lo, hi = a[0], a[0]
    for i in range(m):
        r = (abs(b[i - 1]) if i > 0 else 0.0) + (abs(b[i]) if i + 1 < m else 0.0)
        lo, hi = min(lo, a[i] - r), max(hi, a[i] + r)
    big = max(abs(lo), abs(hi))
    tol, tiny = 2.0 * 2.0**-52 * big, 2.0**-104 * max(big, 2.0**-900)
    it = 0
    while it < 200 and hi - lo > tol:
        mid = lo + 0.5 * (hi - lo)
        if sturm_count(a, b, mid, tiny) > k:
            hi = mid
        else:
            lo = mid
        it += 1
    return lo + 0.5 * (hi - lo)


def lanczos(mv, s, v0, m, kind=np.float64):
    """(alpha, beta, steps_done, ritz_min, ritz_max): alpha_j and beta_{j+1} for j < steps_done; mv in float64 or longdouble as
    `kind` asks (the caller's product must keep the precision); s: the Jacobi scaling or None"""
    v0 = np.asarray(v0, dtype=kind)
    rt = np.sqrt(np.asarray(s, dtype=kind)) if s is not None else None
    if s is not None and not np.all(np.asarray(s) > 0):
        raise ValueError("a diagonal entry is not positive")
    cv = (lambda v: rt * mv(rt * v)) if rt is not None else mv
    v = v0 / np.sqrt(np.dot(v0, v0))
    prev = np.zeros_like(v)
    alpha, beta = [], []
    scale, b_j = kind(0.0), kind(0.0)
    for _ in range(m):
        w = cv(v)
        a = np.dot(v, w)
        w = w - a * v - b_j * prev
        b_next = np.sqrt(np.dot(w, w))
        alpha.append(a)
        beta.append(b_next)
        scale = max(scale, abs(a))
        if not b_next > kind(BREAKDOWN) * scale:
            break
        scale = max(scale, b_next)
        prev, v, b_j = v, w / b_next, b_next
    done = len(alpha)
    off = beta[: done - 1]
    return (np.array(alpha, dtype=kind), np.array(beta, dtype=kind), done, tridiagonal_eigenvalue(alpha, off, 0),
            tridiagonal_eigenvalue(alpha, off, done - 1))


# ---- systems --------------------------------------------------------------------------------------------------------------------------
def laplacian_2d_csr(m):
    n, r, c, v = sr.laplacian_2d(m)
    return (n,) + sr.csr_arrays(n, r, c, v)


def laplacian_2d_bounds(m):
    """(smallest, largest) eigenvalue of the unscaled 5-point Laplacian on an m x m grid"""
    c = np.cos(np.pi / (m + 1))
    return 4.0 - 4.0 * c, 4.0 + 4.0 * c


def tridiagonal(n, lower=-1.0, diag=2.0, upper=-1.0):
    """CSR of the n x n tridiagonal matrix with constant diagonals"""
    i = np.arange(n)
    row = np.concatenate([i[1:], i, i[:-1]])
    col = np.concatenate([i[:-1], i, i[1:]])
    val = np.concatenate([np.full(max(n - 1, 0), lower), np.full(n, diag), np.full(max(n - 1, 0), upper)])
    o = np.lexsort((col, row))
    return (n,) + sr.csr_arrays(n, row[o], col[o], val[o])


def diagonal(values):
    n = len(values)
    return n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.asarray(values, dtype=np.float64)


SYSTEMS = {  # name: (solver, builder)
    "cg_laplacian12": ("cg", lambda: ir.laplacian_3d(12)),
    "cg_laplacian24": ("cg", lambda: ir.laplacian_3d(24)),
    "bicgstab_convdiff40": ("bicgstab", lambda: ir.convection_diffusion_2d(40)),
    "bicgstab_laplacian64": ("bicgstab", lambda: laplacian_2d_csr(64)),
    "gmres_convdiff40": ("gmres", lambda: ir.convection_diffusion_2d(40)),
    "gmres_laplacian64": ("gmres", lambda: laplacian_2d_csr(64)),
}
REL_TOL = 1e-9
GMRES_RESTART = 30
DEGREES = (4, 8)
# Iterations of the float64 twins (pairwise dots) to REL_TOL from x0 = 0 with the default set-up - Jacobi scaling, lmax the row
# bound, lmin = lmax / 30 - and without a preconditioner, as tests/test_chebyshev_ref.py::test_iteration_counts_of_the_twins measures
# them on the CPU (it fails when they move).  tests/test_gpu_chebyshev.py allows the engine one iteration either side.
TWIN_ITERATIONS = {  # (system, degree): iterations
    ("cg_laplacian12", 4): 14, ("cg_laplacian12", 8): 8,
    ("cg_laplacian24", 4): 23, ("cg_laplacian24", 8): 14,
    ("bicgstab_convdiff40", 4): 15, ("bicgstab_convdiff40", 8): 9,
    ("bicgstab_laplacian64", 4): 35, ("bicgstab_laplacian64", 8): 22,
    ("gmres_convdiff40", 4): 22, ("gmres_convdiff40", 8): 13,
    ("gmres_laplacian64", 4): 60, ("gmres_laplacian64", 8): 31,
}
UNPRECONDITIONED_ITERATIONS = {"cg_laplacian12": 53, "cg_laplacian24": 101, "bicgstab_convdiff40": 66, "bicgstab_laplacian64": 153,
                               "gmres_convdiff40": 207, "gmres_laplacian64": 590}


def solver_system(name):
    """(solver, n, rp, cc, cv, b)"""
    solver, build = SYSTEMS[name]
    n, rp, cc, cv = build()
    b = np.random.default_rng(4000 + list(SYSTEMS).index(name)).uniform(-1, 1, n)
    return solver, n, rp, cc, cv, b


def default_preconditioner(n, rp, cc, cv, degree, ratio=30.0):
    """M^-1 as a solver's own set-up builds it: Jacobi scaling, lmax the row bound, lmin = lmax / ratio"""
    s = inverse_diagonal(n, rp, cc, cv)
    lmax = row_bound(n, rp, cc, cv, s)
    c0, c1, c2 = coefficients(degree, lmax / ratio, lmax)
    mv = lambda x: ir.csr_mv(n, rp, cc, cv, x)
    return lambda r: apply(mv, s, r, c0, c1, c2)


def run_twin(name, degree, max_iter=2000):
    """(x, iterations) of the float64 twin of the system's solver; degree 0: no preconditioner"""
    solver, n, rp, cc, cv, b = solver_system(name)
    mv = lambda x: ir.csr_mv(n, rp, cc, cv, x)
    minv = default_preconditioner(n, rp, cc, cv, degree) if degree else None
    if solver == "gmres":
        import gmres_ref as gr

        rows = np.repeat(np.arange(n), np.diff(rp))
        return gr.run_to_tolerance((rows, cc, cv), n, b, np.zeros(n), GMRES_RESTART, minv, REL_TOL, max_iter)
    run = ir.run_bicgstab if solver == "bicgstab" else ir.run_cg
    return run(mv, minv if minv else (lambda r: r.copy()), b, REL_TOL, max_iter)
