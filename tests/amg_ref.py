"""NumPy twin of aggregation AMG (csrc/amg.hip; SPMV_PRECOND_AMG): the definition that include/spmv_abi.h states, restated number
for number.  tests/test_amg_ref.py holds it to facts of its own on the CPU; tests/test_gpu_amg.py and
tests/test_gpu_amg_edges.py hold the engine to it.

Level 0 is the matrix; level l + 1 is built from level l until level l is the coarsest: n_l <= coarse_max, l + 1 == max_levels, or
5 n_c > 4 n_l (stalled).

Strength.  theta <= 0: every stored a_ij with j != i makes j a neighbour of i; theta > 0: iff a_ij^2 >= theta^2 |a_ii a_jj|.  The
graph is what the row lists give.

MIS(2).  The priority of row i is ((h(i) << 32) | i) + 1 with the 32-bit finaliser h; 0 is below all of them.  A round: t = the
priority of an undecided row, else 0; twice t_i <- max(t_i, max over neighbours t_j); an undecided row with t_i = its priority is
a root; the root flag is spread twice the same way and removes the undecided rows it reaches.  Roots take ids in ascending row
order.  Pass 1: a non-root joins the smallest root id among its neighbours.  Pass 2: a row still free joins the smallest id among
its neighbours as pass 1 left them.

Coarse operator.  A_c[I, J] = sum of a_ij over all stored entries, added from 0.0 in ascending (I, J, entry) order.

Cycle (V(1,1)), smoother M_l the Chebyshev polynomial of chebyshev_ref with the default set-up (Jacobi scaling, lmax the row bound,
lmin = lmax / 30) and degree smooth_degree:
    x = M^-1 b;  b_c[I] = sum over i in I, ascending, of (b - A x)[i];  x_c = cycle(l + 1);  x[i] += omega x_c[agg(i)];
    x += M^-1 (b - A x)
and at the coarsest level x = inverse b (n <= 1024: LU with partial pivoting) or x = M^-1 b."""
import numpy as np

import chebyshev_ref as cr
import ilu0_ref as ir
import solver_ref as sr

DEFAULTS = dict(max_levels=16, coarse_max=256, smooth_degree=2, strength=0.0, overcorrection=1.5)
DENSE_MAX = 1024
SINGULAR = 2.0**-44
MUTATIONS = ("tie", "strong_sum", "post_degree", "restrict_drop", "prolong_tail")
_U32 = np.uint32
_U64 = np.uint64


def hash32(i):
    h = np.asarray(i).astype(_U32)
    h = h ^ (h >> _U32(16))
    h = h * _U32(0x85EBCA6B)
    h = h ^ (h >> _U32(13))
    h = h * _U32(0xC2B2AE35)
    h = h ^ (h >> _U32(16))
    return h


def priorities(n):
    i = np.arange(n, dtype=_U64)
    return ((hash32(i).astype(_U64) << _U64(32)) | i) + _U64(1)


def diagonal_of(n, rp, cc, cv):
    """a_ii, duplicates summed; a zero or missing entry raises"""
    rows = np.repeat(np.arange(n), np.diff(rp))
    d = np.zeros(n)
    on = rows == np.asarray(cc)
    np.add.at(d, rows[on], np.asarray(cv)[on])
    if np.any(d == 0.0):
        raise ValueError("a zero or missing diagonal entry")
    return d


def neighbour_mask(n, rp, cc, cv, theta):
    """per stored entry: is its column a neighbour of its row"""
    rows = np.repeat(np.arange(n), np.diff(rp))
    cc = np.asarray(cc)
    d = diagonal_of(n, rp, cc, cv)
    off = rows != cc
    if theta > 0.0:
        theta2 = theta * theta
        off &= np.asarray(cv) * np.asarray(cv) >= theta2 * np.abs(d[rows] * d[cc])
    return rows, off


def _spread(values, rows, cols, mask, n, rp):
    """out_i = max(v_i, max over the neighbours j of v_j)"""
    out = values.copy()
    if len(rows):
        contrib = np.where(mask, values[cols], values.dtype.type(0))
        filled = np.flatnonzero(np.diff(rp) > 0)
        best = np.maximum.reduceat(contrib, np.asarray(rp)[filled])  # (a maximum does not depend on the order)
        out[filled] = np.maximum(out[filled], best)
    return out


def _min_over(values, rows, cols, take, n, rp, none):
    """min over the entries with take of values[col], per row; `none` where there is no such entry"""
    out = np.full(n, none, dtype=np.int64)
    if len(rows):
        contrib = np.where(take, values[cols], none)
        filled = np.flatnonzero(np.diff(rp) > 0)
        out[filled] = np.minimum.reduceat(contrib, np.asarray(rp)[filled])
    return out


def aggregate(n, rp, cc, cv, theta=0.0, mutate=None):
    """(agg, number of aggregates, rounds, roots): the aggregate of every row"""
    cc = np.asarray(cc)
    rows, mask = neighbour_mask(n, rp, cc, cv, theta)
    prio = priorities(n)
    state = np.zeros(n, dtype=np.int8)  # 0 undecided, 1 root, 2 removed
    rounds = 0
    while np.any(state == 0):
        t = np.where(state == 0, prio, _U64(0))
        t = _spread(_spread(t, rows, cc, mask, n, rp), rows, cc, mask, n, rp)
        state[(state == 0) & (t == prio)] = 1
        flag = (state == 1).astype(_U64)
        flag = _spread(_spread(flag, rows, cc, mask, n, rp), rows, cc, mask, n, rp)
        state[(state == 0) & (flag != 0)] = 2
        rounds += 1
    root = state == 1
    root_id = np.cumsum(root) - root  # exclusive scan
    none = np.int64(2**31 - 1)
    if mutate != "tie":
        best = _min_over(root_id, rows, cc, mask & root[cc], n, rp, none)
    else:  # the mutation: the LARGEST root id among the neighbours
        best = -_min_over(-root_id, rows, cc, mask & root[cc], n, rp, none)
        best = np.where(best == -none, none, best)
    agg1 = np.where(root, root_id, np.where(best == none, -1, best))
    best2 = _min_over(agg1, rows, cc, mask & (agg1[cc] >= 0), n, rp, none)
    agg = np.where(agg1 >= 0, agg1, np.where(best2 == none, -1, best2))
    assert np.all(agg >= 0), "a row was left without an aggregate"
    return agg.astype(np.int32), int(root.sum()), rounds, np.flatnonzero(root)


def coarse_operator(n, rp, cc, cv, agg, nc, theta=0.0, mutate=None):
    """(row_ptr, col, val) of A_c: sums over every stored entry from 0.0 in (I, J, entry) order"""
    rows = np.repeat(np.arange(n), np.diff(rp))
    cc, cv = np.asarray(cc), np.asarray(cv, dtype=np.float64)
    ki, kj = agg[rows].astype(np.int64), agg[cc].astype(np.int64)
    if mutate == "strong_sum":  # the mutation: the strong entries (and the diagonal) alone
        keep = neighbour_mask(n, rp, cc, cv, theta)[1] | (rows == cc)
        ki, kj, cv = ki[keep], kj[keep], cv[keep]
    order = np.lexsort((kj, ki))  # stable: entry ids ascending within equal keys
    ki, kj, v = ki[order], kj[order], cv[order]
    head = np.ones(len(ki), dtype=bool)
    head[1:] = (ki[1:] != ki[:-1]) | (kj[1:] != kj[:-1])
    run = np.cumsum(head) - 1
    val = np.zeros(int(head.sum()))
    np.add.at(val, run, v)  # unbuffered, in index order: 0.0 + v_1 + v_2 + ...
    rp_c = np.zeros(nc + 1, dtype=np.int32)
    np.add.at(rp_c, ki[head] + 1, 1)
    return np.cumsum(rp_c).astype(np.int32), kj[head].astype(np.int32), val


def dense_inverse(n, rp, cc, cv):
    """the inverse by LU with partial pivoting (the first of the largest), row operations in the engine's order"""
    lu = np.zeros((n, n))
    np.add.at(lu, (np.repeat(np.arange(n), np.diff(rp)), np.asarray(cc)), np.asarray(cv, dtype=np.float64))
    largest = np.max(np.abs(lu)) if n else 0.0
    perm = np.arange(n)
    for k in range(n):
        p = k + int(np.argmax(np.abs(lu[k:, k])))
        pivot = lu[p, k]
        if not abs(pivot) >= SINGULAR * largest or pivot == 0.0:
            raise ValueError("singular coarsest operator")
        if p != k:
            lu[[p, k]] = lu[[k, p]]
            perm[[p, k]] = perm[[k, p]]
        m = lu[k + 1:, k] / pivot
        lu[k + 1:, k] = m
        lu[k + 1:, k + 1:] -= np.outer(m, lu[k, k + 1:])
    inv = np.zeros((n, n))
    inv[np.arange(n), perm] = 1.0
    for i in range(n):
        inv[i] -= lu[i, :i] @ inv[:i]
    for i in range(n - 1, -1, -1):
        inv[i] -= lu[i, i + 1:] @ inv[i + 1:]
        inv[i] /= lu[i, i]
    return inv


class Level:
    def __init__(self, n, rp, cc, cv, degree):
        self.n, self.rp, self.cc, self.cv = n, np.asarray(rp), np.asarray(cc), np.asarray(cv, dtype=np.float64)
        self.nnz = len(self.cc)
        self.agg, self.nc = None, 0
        self.degree = degree
        self._rows = np.repeat(np.arange(n), np.diff(self.rp))
        self._cheby = None
        self.smoother = None  # (scaled, lmin, lmax) in place of the default set-up: what a later spmv_chebyshev_setup left on the handle

    def mv(self, x):
        return np.bincount(self._rows, weights=self.cv * x[self.cc], minlength=self.n)

    def cheby(self, degree=None):
        """(s, c0, c1, c2) of the default set-up, or of `smoother` (s None: unscaled)"""
        degree = degree or self.degree
        if self._cheby is None or self._cheby[0] != degree:
            if self.smoother is None:
                s = cr.inverse_diagonal(self.n, self.rp, self.cc, self.cv)
                lmax = cr.row_bound(self.n, self.rp, self.cc, self.cv, s)
                lmin = lmax / 30.0
            else:
                scaled, lmin, lmax = self.smoother
                s = cr.inverse_diagonal(self.n, self.rp, self.cc, self.cv) if scaled else None
            self._cheby = (degree, s) + cr.coefficients(degree, lmin, lmax)
        return self._cheby[1:]


class Hierarchy:
    """the twin of spmv_amg_setup; 0 or None for an argument: its default.  level0_smoother = (degree, scaled, lmin, lmax): level 0
    smooths with that polynomial instead (the handle's own Chebyshev state after a later spmv_chebyshev_setup: the cycle reads it
    as it stands; the hierarchy and the coarse levels' smoothers are what the set-up built)"""

    def __init__(self, n, rp, cc, cv, max_levels=0, coarse_max=0, smooth_degree=0, strength=0.0, overcorrection=0.0, mutate=None,
                 level0_smoother=None):
        self.max_levels = max_levels or DEFAULTS["max_levels"]
        self.coarse_max = coarse_max or DEFAULTS["coarse_max"]
        self.degree = smooth_degree or DEFAULTS["smooth_degree"]
        self.theta = strength if strength > 0.0 else 0.0
        self.omega = overcorrection or DEFAULTS["overcorrection"]
        self.mutate = mutate
        self.levels = [Level(n, rp, cc, cv, self.degree)]
        self.mis_rounds = 0
        self.roots = []
        self.inv = None
        if n == 0:
            return
        while True:
            L = self.levels[-1]
            if L.n <= self.coarse_max or len(self.levels) == self.max_levels:
                break
            agg, nc, rounds, roots = aggregate(L.n, L.rp, L.cc, L.cv, self.theta, mutate)
            self.mis_rounds += rounds
            if 5 * nc > 4 * L.n:
                break
            L.agg, L.nc = agg, nc
            self.roots.append(roots)
            rp_c, cc_c, cv_c = coarse_operator(L.n, L.rp, L.cc, L.cv, agg, nc, self.theta, mutate)
            self.levels.append(Level(nc, rp_c, cc_c, cv_c, self.degree))
        last = self.levels[-1]
        if last.n <= DENSE_MAX:
            self.inv = dense_inverse(last.n, last.rp, last.cc, last.cv)
        if level0_smoother is not None:
            self.levels[0].degree = int(level0_smoother[0])
            self.levels[0].smoother = (bool(level0_smoother[1]), float(level0_smoother[2]), float(level0_smoother[3]))

    @property
    def rows(self):
        return [L.n for L in self.levels]

    @property
    def nnz(self):
        return [L.nnz for L in self.levels]

    def launches(self):
        if self.levels[0].n == 0:
            return 0
        degrees = [L.degree for L in self.levels]  # (level 0's may have been replaced: level0_smoother)
        return sum(4 * d + 7 for d in degrees[:-1]) + (1 if self.inv is not None else 2 * degrees[-1] + 1)

    def apply(self, r, level=0):
        """z = B r"""
        L = self.levels[level]
        if L.n == 0:
            return np.zeros(0)
        if level + 1 == len(self.levels):
            if self.inv is not None:
                return self.inv @ r
            s, c0, c1, c2 = L.cheby()
            return cr.apply(L.mv, s, r, c0, c1, c2)
        s, c0, c1, c2 = L.cheby()
        x = cr.apply(L.mv, s, r, c0, c1, c2)
        bc = np.zeros(L.nc)
        residual = r - L.mv(x)
        if self.mutate == "restrict_drop":  # the mutation: the last member of every aggregate of two and more is left out
            last = np.zeros(L.nc, dtype=np.int64)
            np.maximum.at(last, L.agg, np.arange(L.n))
            residual[last[np.bincount(L.agg, minlength=L.nc) > 1]] = 0.0
        np.add.at(bc, L.agg, residual)  # in ascending row order from 0.0
        xc = self.apply(bc, level + 1)
        x = x + self.omega * xc[L.agg]
        if self.mutate == "prolong_tail":  # the mutation: the last row's correction is added twice
            x[-1] += self.omega * xc[L.agg[-1]]
        if self.mutate == "post_degree":  # the mutation: another polynomial behind the correction
            s, c0, c1, c2 = L.cheby(L.degree + 1)
        return cr.smooth(L.mv, s, r, x, c0, c1, c2)

    def dense_operator(self):
        """B column by column"""
        n = self.levels[0].n
        return np.stack([self.apply(e) for e in np.eye(n)], axis=1)

    def prolongator(self, level=0):
        L = self.levels[level]
        P = np.zeros((L.n, L.nc))
        P[np.arange(L.n), L.agg] = 1.0
        return P


# ---- systems ----------------------------------------------------------------------------------------------------------------------
def dense_of(n, rp, cc, cv):
    dense = np.zeros((n, n))
    np.add.at(dense, (np.repeat(np.arange(n), np.diff(rp)), np.asarray(cc)), cv)
    return dense


def anisotropic_2d(m, ax=1.0, ay=0.01):
    """the 5-point stencil -ax u_xx - ay u_yy on an m x m grid, row i = y * m + x"""
    y, x = np.divmod(np.arange(m * m), m)
    row, col, val = [np.arange(m * m)], [np.arange(m * m)], [np.full(m * m, 2.0 * (ax + ay))]
    for ok, step, a in ((x > 0, -1, ax), (x < m - 1, 1, ax), (y > 0, -m, ay), (y < m - 1, m, ay)):
        i = np.flatnonzero(ok)
        row.append(i)
        col.append(i + step)
        val.append(np.full(len(i), -a))
    row, col, val = np.concatenate(row), np.concatenate(col), np.concatenate(val)
    o = np.lexsort((col, row))
    return (m * m,) + sr.csr_arrays(m * m, row[o], col[o], val[o])


def arrow(n):
    """row and column 0 full, a diagonal of n + 1: one row wider than a wavefront"""
    i = np.arange(1, n)
    row = np.concatenate([np.zeros(n, dtype=np.int64), i, i])
    col = np.concatenate([np.arange(n), np.zeros(n - 1, dtype=np.int64), i])
    val = np.concatenate([[n + 1.0], np.full(n - 1, -1.0), np.full(n - 1, -1.0), np.full(n - 1, n + 1.0)])
    o = np.lexsort((col, row))
    return (n,) + sr.csr_arrays(n, row[o], col[o], val[o])


def random_nonsymmetric(n, k=4, seed=11):
    """a structurally nonsymmetric pattern: k random off-diagonal columns a row, a full dominant diagonal"""
    rng = np.random.default_rng(seed)
    row, col, val = [], [], []
    for i in range(n):
        others = np.setdiff1d(rng.choice(n, size=k, replace=False), [i])
        cols = np.sort(np.concatenate([others, [i]]))
        vals = np.where(cols == i, float(k + 1), -rng.uniform(0.25, 1.0, len(cols)))
        row.append(np.full(len(cols), i))
        col.append(cols)
        val.append(vals)
    return (n,) + sr.csr_arrays(n, np.concatenate(row), np.concatenate(col), np.concatenate(val))


def periodic_tridiagonal(n):
    """2.5 on the diagonal, -1 at (i, i +- 1 mod n), columns ascending: rows 0 and n - 1 reach across the whole matrix, and so does
    the first or last row of some block of rows on every coarse level"""
    i = np.arange(n)
    row = np.concatenate([i, i, i])
    col = np.concatenate([(i - 1) % n, i, (i + 1) % n])
    val = np.concatenate([np.full(n, -1.0), np.full(n, 2.5), np.full(n, -1.0)])
    o = np.lexsort((col, row))
    return (n,) + sr.csr_arrays(n, row[o], col[o], val[o])


FUZZ_SIZES = (1, 2, 3, 5, 17, 64, 65, 130, 300, 700)
FUZZ_BASE = 7031  # (of the bases 7000 .. 7059 the one whose seeds 0 .. 23 draw all ten sizes and most often n > coarse_max)
FUZZ_E = 10  # every stored value of fuzz_system is an integer multiple of 2^-FUZZ_E (exact.scaled(cv, FUZZ_E))


def fuzz_system(seed):
    """(n, rp, cc, cv): a strictly row-dominant matrix with a positive diagonal on a structurally nonsymmetric pattern, as untidy as
    CSR allows.  0 .. 6 random off-diagonal columns a row, values exact.dyadic (at most 10 bits, exponents -10 .. 0); about 15 % of
    those entries stored twice, as two dyadic parts, about 10 % stored as 0.0; the diagonal = the row's sum of stored |off-diagonal
    values| + 1 + one more |dyadic| (all on the grid 2^-10), in half the rows split into two stored parts; the entries of a row in
    random order.  Row dominance with a positive diagonal survives the coarse operator's sums: no coarse diagonal is zero, no
    coarsest operator singular."""
    import exact

    rng = np.random.default_rng(FUZZ_BASE + seed)
    n = int(FUZZ_SIZES[rng.integers(len(FUZZ_SIZES))])
    grid = 2**FUZZ_E
    row, col, val = [], [], []
    for i in range(n):
        k = int(min(rng.integers(0, 7), n - 1))
        others = rng.choice(n - 1, size=k, replace=False) if k else np.zeros(0, dtype=np.int64)
        others = others + (others >= i)  # (skips i)
        cols, vals = [], []
        for j in others:
            kind = rng.random()
            if kind < 0.10:
                parts = [0.0]
            else:
                parts = list(exact.dyadic(rng, 2 if kind < 0.25 else 1, 10, 0, -FUZZ_E))
            cols += [int(j)] * len(parts)
            vals += parts
        weight = int(sum(abs(v) for v in vals) * grid) + grid + int(abs(exact.dyadic(rng, 1, 10, 0, -FUZZ_E)[0]) * grid)
        if rng.random() < 0.5:
            first = int(rng.integers(1, weight))  # (weight >= 2^10 + 1)
            parts = [first / grid, (weight - first) / grid]
        else:
            parts = [weight / grid]
        cols += [i] * len(parts)
        vals += parts
        o = rng.permutation(len(cols))
        row.append(np.full(len(cols), i))
        col.append(np.asarray(cols, dtype=np.int64)[o])
        val.append(np.asarray(vals, dtype=np.float64)[o])
    return (n,) + sr.csr_arrays(n, np.concatenate(row), np.concatenate(col), np.concatenate(val))


FUZZ_SEEDS = tuple(range(24))


def fuzz_setup(seed):
    """the set-up arguments that go with fuzz_system(seed): theta cycles through 0, 0.1, 0.5; coarse_max is drawn from 1, 8, 256"""
    return dict(strength=(0.0, 0.1, 0.5)[seed % 3], coarse_max=int(np.random.default_rng(FUZZ_BASE + 100 + seed).choice((1, 8, 256))))


def galerkin_int64(n, rp, cc, cv, agg, nc, e=FUZZ_E):
    """P^T A P in int64 on the grid 2^-e, dense (nc x nc), and the pattern (which (I, J) hold a stored entry): arithmetic that
    shares no ordering code with coarse_operator"""
    import exact

    rows = np.repeat(np.arange(n), np.diff(rp))
    dense = np.zeros((nc, nc), dtype=np.int64)
    stored = np.zeros((nc, nc), dtype=bool)
    I, J = np.asarray(agg)[rows], np.asarray(agg)[np.asarray(cc)]
    np.add.at(dense, (I, J), exact.scaled(cv, e))
    stored[I, J] = True
    return dense, stored


PERIODIC = 100000
_DEGREE1 = dict(smooth_degree=1, overcorrection=1.0)
# The applications tests/test_gpu_amg_edges.py compares with the twin, name: (builder, arguments of Hierarchy).
# tests/test_amg_ref.py::test_every_mutation_moves_every_application holds each to the five mutations.
EDGE_CASES = {
    "arrow300": (lambda: arrow(300), dict(coarse_max=8)),
    "nonsymmetric500": (lambda: random_nonsymmetric(500), dict(coarse_max=8)),
    "anisotropic16x16": (lambda: anisotropic_2d(16), dict(coarse_max=8, strength=0.5)),
    "anisotropic16x16_quarter": (lambda: anisotropic_2d(16), dict(coarse_max=8, strength=0.25)),
    "tridiagonal257": (lambda: cr.tridiagonal(257), dict(coarse_max=1)),
    "diagonal257": (lambda: cr.diagonal(np.linspace(1.0, 2.0, 257)), dict(coarse_max=1)),
}
IRREGULAR = tuple(EDGE_CASES)
EDGE_CASES.update({name + "_degree1": (EDGE_CASES[name][0], dict(EDGE_CASES[name][1], **_DEGREE1)) for name in IRREGULAR})
EDGE_CASES.update({f"fuzz{seed:02d}": ((lambda seed=seed: fuzz_system(seed)), fuzz_setup(seed)) for seed in FUZZ_SEEDS})
EDGE_CASES.update({
    "laplacian32x32": (lambda: cr.laplacian_2d_csr(32), dict(coarse_max=8)),
    "laplacian32x32_unscaled3": (lambda: cr.laplacian_2d_csr(32), dict(coarse_max=8, level0_smoother=(3, False) + cr.laplacian_2d_bounds(32))),
    "periodic100000": (lambda: periodic_tridiagonal(PERIODIC), dict()),
    "tridiagonal1024": (lambda: cr.tridiagonal(1024), dict(max_levels=1)),
    "tridiagonal1025": (lambda: cr.tridiagonal(1025), dict(max_levels=1)),
})


def edge_rhs(name, n):
    """the right-hand side the case is applied to"""
    return np.random.default_rng(9000 + list(EDGE_CASES).index(name)).uniform(-1, 1, n)


SYSTEMS = {  # name: (solver, builder)
    "cg_laplacian64": ("cg", lambda: cr.laplacian_2d_csr(64)),
    "cg_laplacian24": ("cg", lambda: ir.laplacian_3d(24)),
    "bicgstab_convdiff40": ("bicgstab", lambda: ir.convection_diffusion_2d(40)),
    "bicgstab_laplacian64": ("bicgstab", lambda: cr.laplacian_2d_csr(64)),
    "gmres_convdiff40": ("gmres", lambda: ir.convection_diffusion_2d(40)),
    "gmres_laplacian64": ("gmres", lambda: cr.laplacian_2d_csr(64)),
}
REL_TOL = 1e-8
GMRES_RESTART = 30
# Iterations of the float64 twins to REL_TOL from x0 = 0 with the default hierarchy and without a preconditioner, as
# tests/test_amg_ref.py::test_iteration_counts_of_the_twins measures them on the CPU (it fails when they move).
# tests/test_gpu_amg.py allows the engine one iteration either side.
TWIN_ITERATIONS = {"cg_laplacian64": 19, "cg_laplacian24": 14, "bicgstab_convdiff40": 14, "bicgstab_laplacian64": 12, "gmres_convdiff40": 23,
                   "gmres_laplacian64": 19}
UNPRECONDITIONED_ITERATIONS = {"cg_laplacian64": 200, "cg_laplacian24": 93, "bicgstab_convdiff40": 62, "bicgstab_laplacian64": 148,
                               "gmres_convdiff40": 195, "gmres_laplacian64": 523}


def solver_system(name):
    """(solver, n, rp, cc, cv, b)"""
    solver, build = SYSTEMS[name]
    n, rp, cc, cv = build()
    b = np.random.default_rng(5000 + list(SYSTEMS).index(name)).uniform(-1, 1, n)
    return solver, n, rp, cc, cv, b


def run_twin(name, amg=True, max_iter=2000, **setup):
    """(x, iterations) of the float64 twin of the system's solver; amg False: no preconditioner"""
    solver, n, rp, cc, cv, b = solver_system(name)
    mv = lambda x: ir.csr_mv(n, rp, cc, cv, x)
    minv = Hierarchy(n, rp, cc, cv, **setup).apply if amg else None
    if solver == "gmres":
        import gmres_ref as gr

        rows = np.repeat(np.arange(n), np.diff(rp))
        return gr.run_to_tolerance((rows, cc, cv), n, b, np.zeros(n), GMRES_RESTART, minv, REL_TOL, max_iter)
    run = ir.run_bicgstab if solver == "bicgstab" else ir.run_cg
    return run(mv, minv if minv else (lambda r: r.copy()), b, REL_TOL, max_iter)
