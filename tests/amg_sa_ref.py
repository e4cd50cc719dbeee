"""NumPy twin of smoothed-aggregation AMG (spmv_amg_setup_smoothed, csrc/amg.hip): the definition that
include/spmv_abi.h states, restated number for number on top of amg_ref (aggregates, stop rules, the dense inverse), spgemm_ref (every
product and the transpose) and chebyshev_ref (the row bound, the smoother).  tests/test_amg_sa_ref.py holds it to facts of its own on
the CPU; tests/test_gpu_amg_sa.py holds the engine to it.

On level l, with agg from amg_ref.aggregate and its strength mask:
  A^F   theta <= 0: the level's own arrays.  theta > 0: row i holds, in stored order, every stored diagonal entry and every entry
        the mask calls a neighbour; if the row has a weak off-diagonal entry, one more entry (i, i) comes last, the sum of the weak
        values from 0.0 left to right.
  d_i   the sum of the diagonal entries of row i of A^F in stored order (zero: an error).
  lam   chebyshev_ref.row_bound of A^F with s_i = 1 / d_i.
  T     n x nc, one entry 1.0 at (i, agg(i)).
  P     AT = spgemm(A^F, T); g = prolong_damping / lam; c_i = g / d_i; P[i, J] = e - c_i AT[i, J], e = 1.0 where J = agg(i), else
        0.0: the product rounded once, then a plain subtraction.
  R     transpose(P).
  A_c   spgemm(R, spgemm(A_l, P)), with the full A_l.
Cycle: as amg_ref's, with b_c = R (b - A x) and x += omega P x_c."""
import numpy as np

import amg_ref as ar
import chebyshev_ref as cr
import ilu0_ref as ir
import spgemm_ref as sg

DEFAULTS = dict(ar.DEFAULTS, overcorrection=1.0, prolong_damping=4.0 / 3.0)
MUTATIONS = ("tentative", "unlumped", "galerkin_filtered", "restrict_tentative", "omega_dropped")


def filtered(n, rp, cc, cv, theta, mutate=None):
    """(row_ptr, col, val) of A^F; theta <= 0: the arrays themselves"""
    rp, cc, cv = np.asarray(rp), np.asarray(cc), np.asarray(cv, dtype=np.float64)
    if not theta > 0.0:
        return rp, cc, cv
    rows, mask = ar.neighbour_mask(n, rp, cc, cv, theta)
    keep = mask | (rows == cc)
    weak = ~keep
    lump = np.zeros(n)
    np.add.at(lump, rows[weak], cv[weak])  # from 0.0, in stored order
    has = np.zeros(n, dtype=bool)
    has[rows[weak]] = True
    if mutate == "unlumped":  # the mutation: the weak entries are dropped, not lumped
        has[:] = False
    kept = np.bincount(rows[keep], minlength=n)
    rp_f = np.concatenate([[0], np.cumsum(kept + has)]).astype(np.int64)
    cc_f, cv_f = np.zeros(rp_f[-1], dtype=np.int32), np.zeros(rp_f[-1])
    first = np.cumsum(kept) - kept
    at = rp_f[rows[keep]] + (np.arange(int(keep.sum())) - first[rows[keep]])
    cc_f[at], cv_f[at] = cc[keep], cv[keep]
    last = rp_f[1:][has] - 1
    cc_f[last], cv_f[last] = np.flatnonzero(has), lump[has]
    return rp_f.astype(np.int32), cc_f, cv_f


def filtered_diagonal(n, rp_f, cc_f, cv_f, level=0):
    rows = np.repeat(np.arange(n), np.diff(rp_f))
    d = np.zeros(n)
    on = rows == cc_f
    np.add.at(d, rows[on], cv_f[on])
    if np.any(d == 0.0):
        raise ValueError(f"the filtered operator of level {level} has a zero diagonal")
    return d


def tentative(n, agg):
    return np.arange(n + 1, dtype=np.int32), np.asarray(agg, dtype=np.int32), np.ones(n)


def prolongator(n, rp, cc, cv, agg, nc, theta, damping, level=0, mutate=None):
    """((row_ptr, col, val) of P, lam)"""
    AF = filtered(n, rp, cc, cv, theta, mutate)
    d = filtered_diagonal(n, *AF, level=level)
    lam = cr.row_bound(n, AF[0], AF[1], AF[2], 1.0 / d)
    T = tentative(n, agg)
    if mutate == "tentative":  # the mutation: P = T
        return T, lam
    rp_p, cc_p, at = sg.spgemm_twin(n, n, nc, AF, T)[:3]
    g = damping / lam
    c = g / d
    rows = np.repeat(np.arange(n), np.diff(rp_p))
    scaled = c[rows] * at  # rounded once
    e = np.where(cc_p == np.asarray(agg)[rows], 1.0, 0.0)
    return (rp_p, cc_p, e - scaled), lam


class Level(ar.Level):
    def __init__(self, n, rp, cc, cv, degree):
        super().__init__(n, rp, cc, cv, degree)
        self.P = self.R = None
        self.lam = 0.0


def _csr_mv(nrow, M, x):
    rp, cc, cv = M
    return np.bincount(np.repeat(np.arange(nrow), np.diff(rp)), weights=cv * x[cc], minlength=nrow)


class Hierarchy:
    """the twin of spmv_amg_setup_smoothed; 0 or None for an argument: its default"""

    def __init__(self, n, rp, cc, cv, max_levels=0, coarse_max=0, smooth_degree=0, strength=0.0, overcorrection=0.0, prolong_damping=0.0,
                 mutate=None):
        assert mutate is None or mutate in MUTATIONS
        self.max_levels = max_levels or DEFAULTS["max_levels"]
        self.coarse_max = coarse_max or DEFAULTS["coarse_max"]
        self.degree = smooth_degree or DEFAULTS["smooth_degree"]
        self.theta = strength if strength > 0.0 else 0.0
        self.omega = overcorrection or DEFAULTS["overcorrection"]
        self.damping = prolong_damping or DEFAULTS["prolong_damping"]
        self.mutate = mutate
        self.levels = [Level(n, rp, cc, cv, self.degree)]
        self.mis_rounds = 0
        self.inv = None
        if n == 0:
            return
        while True:
            L = self.levels[-1]
            if L.n <= self.coarse_max or len(self.levels) == self.max_levels:
                break
            agg, nc, rounds, _ = ar.aggregate(L.n, L.rp, L.cc, L.cv, self.theta)
            self.mis_rounds += rounds
            if 5 * nc > 4 * L.n:
                break
            L.agg, L.nc = agg, nc
            l = len(self.levels) - 1
            L.P, L.lam = prolongator(L.n, L.rp, L.cc, L.cv, agg, nc, self.theta, self.damping, l, mutate)
            L.R = sg.transpose_twin(L.n, nc, L.P)
            A = (L.rp, L.cc, L.cv)
            if mutate == "galerkin_filtered":  # the mutation: R A^F P
                A = filtered(L.n, L.rp, L.cc, L.cv, self.theta)
            AP = sg.spgemm_twin(L.n, L.n, nc, A, L.P)[:3]
            rp_c, cc_c, cv_c = sg.spgemm_twin(nc, L.n, nc, L.R, AP)[:3]
            self.levels.append(Level(nc, rp_c, cc_c, cv_c, self.degree))
        last = self.levels[-1]
        if last.n <= ar.DENSE_MAX:
            self.inv = ar.dense_inverse(last.n, last.rp, last.cc, last.cv)

    @property
    def rows(self):
        return [L.n for L in self.levels]

    @property
    def nnz(self):
        return [L.nnz for L in self.levels]

    def launches(self):
        if self.levels[0].n == 0:
            return 0
        degrees = [L.degree for L in self.levels]
        return sum(4 * d + 7 for d in degrees[:-1]) + (1 if self.inv is not None else 2 * degrees[-1] + 1)

    def state_bytes(self):
        """a lower bound of "amg_bytes": the aggregates, the arrays of P and R and the vectors (beside them it counts the coarse
        handles' device_bytes, what the analysis of P and R keeps, and the inverse)"""
        pad = lambda k: (k + 31) & ~31
        total = 0
        for l, L in enumerate(self.levels):
            total += 8 * pad(L.n) * (1 if l == 0 else 3)
            if L.agg is not None:
                total += 4 * L.n
                total += 4 * (L.n + 1) + 12 * len(L.P[1]) + 4 * (L.nc + 1) + 12 * len(L.R[1])
        return total

    def apply(self, r, level=0):
        """z = B r"""
        L = self.levels[level]
        if L.n == 0:
            return np.zeros(0)
        if level + 1 == len(self.levels) and self.inv is not None:
            return self.inv @ r
        s, c0, c1, c2 = L.cheby()
        if level + 1 == len(self.levels):
            return cr.apply(L.mv, s, r, c0, c1, c2)
        x = cr.apply(L.mv, s, r, c0, c1, c2)
        residual = r - L.mv(x)
        if self.mutate == "restrict_tentative":  # the mutation: restriction through T^T
            bc = np.bincount(L.agg, weights=residual, minlength=L.nc)
        else:
            bc = _csr_mv(L.nc, L.R, residual)
        xc = self.apply(bc, level + 1)
        step = _csr_mv(L.n, L.P, xc)
        x = x + (step if self.mutate == "omega_dropped" else self.omega * step)
        return cr.smooth(L.mv, s, r, x, c0, c1, c2)

    def dense_operator(self):
        n = self.levels[0].n
        return np.stack([self.apply(e) for e in np.eye(n)], axis=1)

    def dense_prolongator(self, level=0):
        L = self.levels[level]
        return dense_rect(L.n, L.nc, *L.P)


def dense_rect(nrow, ncol, rp, cc, cv):
    out = np.zeros((nrow, ncol))
    np.add.at(out, (np.repeat(np.arange(nrow), np.diff(rp)), np.asarray(cc)), cv)
    return out


def cannot_move(H, mutation):
    """why `mutation` leaves every application of the hierarchy H unchanged, or None where it must move them"""
    if len(H.levels) == 1:
        return "a single level: no prolongator is built"
    if mutation in ("unlumped", "galerkin_filtered"):
        if not H.theta > 0.0:
            return "theta <= 0: A^F is the level's own arrays"
        weak = False
        for L in H.levels[:-1]:
            rows, mask = ar.neighbour_mask(L.n, L.rp, L.cc, L.cv, H.theta)
            lump = np.zeros(L.n)
            off = ~mask & (rows != L.cc)
            np.add.at(lump, rows[off], L.cv[off])
            weak = weak or bool(np.any(lump != 0.0))
        if not weak:
            return "no row of any level lumps anything but 0.0"
    if mutation in ("tentative", "restrict_tentative"):
        if all(len(L.P[1]) == L.n and np.all(L.P[2] == 1.0) for L in H.levels[:-1]):
            return "P = T already"
    if mutation == "tentative" and len(H.levels) == 2 and H.inv is not None:
        L = H.levels[0]
        if len(L.P[1]) == L.n:
            low, high = np.full(L.nc, np.inf), np.full(L.nc, -np.inf)
            np.minimum.at(low, L.P[1], L.P[2])
            np.maximum.at(high, L.P[1], L.P[2])
            if np.all(low == high) and np.all(low != 0.0):
                return "P = T D with a diagonal D, and the coarse level is solved exactly: the correction P (P^T A P)^-1 P^T does not see D"
    if mutation == "omega_dropped" and H.omega == 1.0:
        return "omega = 1.0: the product by omega is exact"
    return None


# ---- the exact family: the 2-D Laplacian, prolong_damping = 1.0, max_levels = 2 -------------------------------------------------------
def _stencil(G):
    """the 5-point Laplacian applied along the two grid axes of G (m x m x k), in G's integer type"""
    out = 4 * G
    out[1:] -= G[:-1]
    out[:-1] -= G[1:]
    out[:, 1:] -= G[:, :-1]
    out[:, :-1] -= G[:, 1:]
    return out


def _reach(G):
    """the pattern of the stencil's product with a boolean G"""
    out = G.copy()
    out[1:] |= G[:-1]
    out[:-1] |= G[1:]
    out[:, 1:] |= G[:, :-1]
    out[:, :-1] |= G[:, 1:]
    return out


def exact_family_int64(m, agg, nc):
    """(8 P, 64 A_1, pattern of P, pattern of A_1) as dense arrays (int64, int64, bool, bool) for the m x m Laplacian with the given
    aggregates under prolong_damping = 1.0: lam = 2, d = 4 and c = 1/8, so 8 P = 8 T - A T and 64 A_1 = (8 P)^T A (8 P).  Integer
    arithmetic on the grid - shifted slices and an int64 matrix product: it shares no ordering code with the twin"""
    n = m * m
    T = np.zeros((n, nc), dtype=np.int64)
    T[np.arange(n), agg] = 1
    G = T.reshape(m, m, nc)
    P8 = 8 * G - _stencil(G)
    pattern_p = _reach(G != 0)
    AP8 = _stencil(P8).reshape(n, nc)
    pattern_ap = _reach(pattern_p).reshape(n, nc)
    P8, pattern_p = P8.reshape(n, nc), pattern_p.reshape(n, nc)
    # (8 P)^T (A 8 P) row by row of the fine grid: the outer product of the row's stored entries of P and of A P, scattered in int64
    ip, vp, sp = _padded_rows(P8, pattern_p)
    ia, va, sa_ = _padded_rows(AP8, pattern_ap)
    I = np.broadcast_to(ip[:, :, None], ip.shape + ia.shape[1:]).ravel()
    J = np.broadcast_to(ia[:, None, :], ip.shape + ia.shape[1:]).ravel()
    A64 = np.zeros((nc, nc), dtype=np.int64)
    np.add.at(A64, (I, J), (vp[:, :, None] * va[:, None, :]).ravel())
    pattern_c = np.zeros((nc, nc), dtype=bool)
    both = (sp[:, :, None] & sa_[:, None, :]).ravel()
    pattern_c[I[both], J[both]] = True
    return P8, A64, pattern_p, pattern_c


def _padded_rows(values, pattern):
    """(columns, values, stored) of every row's stored entries, padded to the longest row with (0, 0, False)"""
    rows, cols = np.nonzero(pattern)
    count = np.bincount(rows, minlength=pattern.shape[0])
    pos = np.arange(len(rows)) - (np.cumsum(count) - count)[rows]
    shape = (pattern.shape[0], int(count.max()))
    idx, val, stored = np.zeros(shape, dtype=np.int64), np.zeros(shape, dtype=np.int64), np.zeros(shape, dtype=bool)
    idx[rows, pos], val[rows, pos], stored[rows, pos] = cols, values[rows, cols], True
    return idx, val, stored


def csr_of_dense(values, pattern, scale):
    """(row_ptr, col, val) of values / scale over the stored pattern, columns ascending"""
    rows, cols = np.nonzero(pattern)
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=pattern.shape[0]))]).astype(np.int32)
    return rp, cols.astype(np.int32), values[rows, cols].astype(np.float64) / scale


# ---- the systems the GPU tests compare -------------------------------------------------------------------------------------------------
BIG = 2 * 2048 * 256 + 3
ARROWS = (63, 64, 65, 127, 129, 257, 300)
COARSEST_N = {1024: 3734, 1025: 3737}  # the tridiagonal sizes whose second level holds 1024 rows (a dense inverse) and 1025 (Chebyshev)
CASES = {  # name: (builder, arguments of Hierarchy)
    "tridiagonal1": (lambda: cr.tridiagonal(1), dict(coarse_max=1)),
    "tridiagonal2": (lambda: cr.tridiagonal(2), dict(coarse_max=1)),
    "tridiagonal3": (lambda: cr.tridiagonal(3), dict(coarse_max=1)),
    "tridiagonal257": (lambda: cr.tridiagonal(257), dict(coarse_max=1)),
    "diagonal1": (lambda: cr.diagonal(np.full(1, 3.0)), dict(coarse_max=1)),
    "diagonal2": (lambda: cr.diagonal(np.linspace(1.0, 2.0, 2)), dict(coarse_max=1)),
    "diagonal3": (lambda: cr.diagonal(np.linspace(1.0, 2.0, 3)), dict(coarse_max=1)),
    "diagonal257": (lambda: cr.diagonal(np.linspace(1.0, 2.0, 257)), dict(coarse_max=1)),
    "laplacian32x32": (lambda: cr.laplacian_2d_csr(32), dict(coarse_max=8)),
    "laplacian12^3": (lambda: ir.laplacian_3d(12), dict(coarse_max=8)),
    "convdiff40": (lambda: ir.convection_diffusion_2d(40), dict(coarse_max=8)),
    "nonsymmetric500": (lambda: ar.random_nonsymmetric(500), dict(coarse_max=8)),
    "anisotropic16x16": (lambda: ar.anisotropic_2d(16), dict(coarse_max=8, strength=0.5)),
    "anisotropic16x16_quarter": (lambda: ar.anisotropic_2d(16), dict(coarse_max=8, strength=0.25)),
}
CASES.update({f"fuzz{seed:02d}": ((lambda seed=seed: ar.fuzz_system(seed)), ar.fuzz_setup(seed)) for seed in ar.FUZZ_SEEDS})
CASES.update({f"arrow{n}": ((lambda n=n: ar.arrow(n)), dict(coarse_max=8)) for n in ARROWS})
SMALL = tuple(CASES)
CASES["tridiagonal_big"] = (lambda: cr.tridiagonal(BIG), dict(max_levels=2))
# what the application is run under beside each case's own arguments
CONFIGS = (dict(smooth_degree=1, overcorrection=1.0, prolong_damping=1.0), dict(smooth_degree=3, overcorrection=1.5),
           dict(max_levels=2, overcorrection=1.5, prolong_damping=1.0), dict(coarse_max=1))
CONFIG_SYSTEMS = ("laplacian32x32", "laplacian12^3", "convdiff40", "anisotropic16x16_quarter")


def case_rhs(name, n):
    return np.random.default_rng(12000 + list(CASES).index(name)).uniform(-1, 1, n)


def coarsest_rows_case(rows):
    """(n, rp, cc, cv) of the tridiagonal system whose two-level hierarchy (max_levels = 2) has `rows` rows on the coarsest level"""
    return cr.tridiagonal(COARSEST_N[rows])


# Iterations of the float64 twins to amg_ref.REL_TOL from x0 = 0 under the smoothed defaults, as
# tests/test_amg_sa_ref.py::test_iteration_counts_of_the_twins measures them on the CPU (it fails when they move).
# tests/test_gpu_amg_sa.py allows the engine one iteration either side.
TWIN_ITERATIONS = {"cg_laplacian64": 11, "cg_laplacian24": 10, "bicgstab_convdiff40": 14, "bicgstab_laplacian64": 7, "gmres_convdiff40": 21,
                   "gmres_laplacian64": 11}


def run_twin(name, max_iter=2000, **setup):
    """(x, iterations) of the float64 twin of the system's solver under the smoothed hierarchy"""
    solver, n, rp, cc, cv, b = ar.solver_system(name)
    mv = lambda x: ir.csr_mv(n, rp, cc, cv, x)
    minv = Hierarchy(n, rp, cc, cv, **setup).apply
    if solver == "gmres":
        import gmres_ref as gr

        rows = np.repeat(np.arange(n), np.diff(rp))
        return gr.run_to_tolerance((rows, cc, cv), n, b, np.zeros(n), ar.GMRES_RESTART, minv, ar.REL_TOL, max_iter)
    return (ir.run_bicgstab if solver == "bicgstab" else ir.run_cg)(mv, minv, b, ar.REL_TOL, max_iter)
