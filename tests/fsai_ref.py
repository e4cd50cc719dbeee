"""NumPy twin of FSAI (spmv_fsai_*; SPMV_PRECOND_FSAI) - TEST INFRASTRUCTURE ONLY (no GPU needed).

The definition the engine is held to (include/spmv_abi.h states it as the contract, csrc/fsai.hip the same):

  pattern   S = the lower triangle, diagonal included, of the structural pattern of A^level (level 1, 2 or 3): every stored entry
            counts, zeros included; a row holds distinct columns in ascending order and its last column is the row itself (a row
            without a stored diagonal entry: ValueError naming the row).  More than MAX_ROW columns in a row: RowTooLong.
  row i     J = S_i, m = |J|.  M = A[J, J] from the LOWER triangle of A alone: entry (p, q), q <= p, is the sum of the stored
            entries (J_p, J_q) of row J_p, from 0.0 in stored order.  M = C C^T right-looking (c_kk = sqrt(m_kk), c_pk = m_pk / c_kk,
            m_pq -= c_pk c_qk); C^T g = e_m from the last unknown up (g_p = t_p / c_pp, t_a -= c_pa g_p).  A pivot that is not
            positive or not finite: ZeroDivisionError naming the row.  (The engine fuses every update into one fma: one rounding
            fewer, 1e-16 relative, six decades below the parity tolerance the values are compared at.)
  apply     z = G^T (G r)

Fsai holds G as CSR (rp, cc, values).  residuals() evaluates the two facts that define G in np.longdouble from ANY G on the
pattern - the twin's or the engine's.  Two switches exist for the mutation check of tests/test_fsai_ref.py only: mutate="upper" takes
the upper triangle as the pattern, mutate="last_wins" stores the last duplicate instead of the sum.
"""
from __future__ import annotations

import math

import numpy as np

import ilu0_ref
import solver_ref
from ilu0_ref import csr_mv, laplacian_3d, run_cg, tridiagonal_8  # noqa: F401  (shared with the ILU(0) tests)

MAX_ROW = 64  # SPMV_FSAI_MAX_ROW
LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


class RowTooLong(Exception):
    def __init__(self, row, m):
        super().__init__(f"row {row} has {m} pattern columns, the cap is {MAX_ROW}")
        self.row, self.m = row, m


# ---- the pattern -----------------------------------------------------------------------------------------------------------------
def _distinct(n, rows, cols):
    code = np.unique(rows.astype(np.int64) * max(n, 1) + cols.astype(np.int64))
    r, c = code // max(n, 1), code % max(n, 1)
    return np.searchsorted(r, np.arange(n + 1)).astype(np.int64), c


def _times(n, prp, pcc, arp, acc):
    """the structural pattern of P A: distinct ascending columns per row"""
    rows = np.repeat(np.arange(n), np.diff(prp))
    lens = (arp[1:] - arp[:-1])[pcc]
    total = int(lens.sum())
    start = np.repeat(arp[:-1][pcc], lens)
    within = np.arange(total) - np.repeat(np.cumsum(lens) - lens, lens)
    return _distinct(n, np.repeat(rows, lens), acc[start + within])


def pattern(n, rp, cc, level, upper=False):
    """(row_ptr, col) of S: tril of the structural pattern of A^level (triu with upper=True, the mutation)"""
    if level not in (1, 2, 3):
        raise ValueError(f"level={level}, must be 1 .. 3")
    rp, cc = np.asarray(rp, np.int64), np.asarray(cc, np.int64)
    prp, pcc = _distinct(n, np.repeat(np.arange(n), np.diff(rp)), cc)
    arp, acc = prp, pcc
    for _ in range(level - 1):
        prp, pcc = _times(n, prp, pcc, arp, acc)
    rows = np.repeat(np.arange(n), np.diff(prp))
    keep = pcc >= rows if upper else pcc <= rows
    rows, pcc = rows[keep], pcc[keep]
    srp = np.searchsorted(rows, np.arange(n + 1)).astype(np.int64)
    on = np.zeros(n, bool)
    on[rows[rows == pcc]] = True
    if not on.all():
        raise ValueError(f"row {int(np.flatnonzero(~on)[0])} has no stored diagonal entry")
    return srp, pcc


def gather(rp, cc, cv, Jr, Jc, lower=False, dtype=np.float64, last_wins=False):
    """A[Jr, Jc] as a dense array (Jc ascending): cell (p, q) the sum of the stored entries (Jr_p, Jc_q) of row Jr_p from 0.0 in
    stored order; lower: only the cells q <= p (the rest stay 0)"""
    m = len(Jc)
    lens = rp[Jr + 1] - rp[Jr]
    total = int(lens.sum())
    p = np.repeat(np.arange(len(Jr)), lens)
    e = np.repeat(rp[Jr], lens) + (np.arange(total) - np.repeat(np.cumsum(lens) - lens, lens))
    c = cc[e]
    q = np.minimum(np.searchsorted(Jc, c), m - 1)
    ok = Jc[q] == c
    if lower:
        ok &= q <= p
    M = np.zeros((len(Jr), m), dtype)
    if last_wins:
        M[p[ok], q[ok]] = cv[e[ok]]
    else:
        np.add.at(M, (p[ok], q[ok]), cv[e[ok]].astype(dtype))  # (unbuffered: in the order given, which is the stored one)
    return M


def local_matrix(rp, cc, cv, J, last_wins=False):
    """M = A[J, J] from the lower triangle of A alone"""
    return gather(rp, cc, cv, J, J, lower=True, last_wins=last_wins)


def solve_row(M, row):
    """g of C^T g = e_m with M = C C^T (the lower triangle of M is read and overwritten)"""
    m = M.shape[0]
    for k in range(m):
        d = M[k, k]
        if not (d > 0.0) or not math.isfinite(d):
            raise ZeroDivisionError(f"a pivot of row {row} is not positive or not finite")
        c = math.sqrt(d)
        M[k, k] = c
        if k + 1 < m:
            M[k + 1:, k] /= c
            M[k + 1:, k + 1:] -= np.outer(M[k + 1:, k], M[k + 1:, k])
    t = np.zeros(m)
    t[m - 1] = 1.0
    g = np.zeros(m)
    for p in range(m - 1, -1, -1):
        g[p] = t[p] / M[p, p]
        if p:
            t[:p] -= M[p, :p] * g[p]
    return g


class Fsai:
    def __init__(self, n, rp, cc, cv, level=1, mutate=None):
        rp, cc, cv = np.asarray(rp, np.int64), np.asarray(cc, np.int64), np.asarray(cv, np.float64)
        self.n, self.level = n, level
        self.rp, self.cc = pattern(n, rp, cc, level, upper=mutate == "upper")
        lens = np.diff(self.rp)
        self.max_row = int(lens.max()) if n else 0
        if self.max_row > MAX_ROW:
            first = int(np.flatnonzero(lens > MAX_ROW)[0])
            raise RowTooLong(first, int(lens[first]))
        self.values = np.zeros(len(self.cc))
        for i in range(n):
            a, b = self.rp[i], self.rp[i + 1]
            J = self.cc[a:b]
            if mutate == "upper":  # (the same system, read from the upper triangle and solved for the row's own unknown, the first)
                M = gather(rp, cc, cv, J, J)[::-1, ::-1].copy()
                self.values[a:b] = solve_row(M, i)[::-1]
            else:
                self.values[a:b] = solve_row(local_matrix(rp, cc, cv, J, last_wins=mutate == "last_wins"), i)
        self.rows = np.repeat(np.arange(n), lens)

    @property
    def nnz(self):
        return len(self.cc)

    def apply(self, r):
        """z = G^T (G r)"""
        return apply_factor(self.n, self.rp, self.cc, self.values, r)


def apply_factor(n, g_rp, g_cc, g_val, r):
    rows = np.repeat(np.arange(n), np.diff(g_rp))
    w = np.bincount(rows, weights=g_val * np.asarray(r)[g_cc], minlength=n)
    return np.bincount(g_cc, weights=g_val * w[rows], minlength=n)


def residuals(n, rp, cc, cv, g_rp, g_cc, g_val, s_rp=None, s_cc=None):
    """In np.longdouble, from A as stored (both triangles, duplicates summed) and any G, in units of the float64 eps:
    (max_i |(G A G^T)_ii - 1| / (|G||A||G^T|)_ii,  max over i and j in S_i, j < i, of |(G A)_ij| / (|G||A|)_ij); S: the pattern given
    (tests/test_fsai_ref.py's mutation check), else G's own"""
    rp, cc = np.asarray(rp, np.int64), np.asarray(cc, np.int64)
    cvl = np.asarray(cv, np.float64).astype(LD)
    g_rp, g_cc = np.asarray(g_rp, np.int64), np.asarray(g_cc, np.int64)
    if s_rp is None:
        s_rp, s_cc = g_rp, g_cc
    worst_diag = worst_off = 0.0
    for i in range(n):
        a, b = g_rp[i], g_rp[i + 1]
        J = g_cc[a:b]
        g = np.asarray(g_val[a:b], np.float64).astype(LD)
        M = gather(rp, cc, cvl, J, J, dtype=LD)
        worst_diag = max(worst_diag, float(abs(g @ M @ g - 1) / (np.abs(g) @ np.abs(M) @ np.abs(g))))
        S = s_cc[s_rp[i]:s_rp[i + 1]]
        S = S[S < i]
        if len(S):
            M = gather(rp, cc, cvl, J, S, dtype=LD)
            scale = np.abs(g) @ np.abs(M)
            worst_off = max(worst_off, float(np.max(np.abs(g @ M) / np.where(scale > 0, scale, 1))))
    return worst_diag / EPS, worst_off / EPS


# What residuals() gives for the twin's own G on every problem below, as tests/test_fsai_ref.py measures and prints it (it fails where
# a problem exceeds a bound): 8 eps on the diagonal, measured 2.9 (dense_blocks); 8 eps off it, measured 2.5 (dense_blocks).  The GPU
# test holds the engine's G to solver_ref.F times these bounds.
DIAG_BOUND_EPS, OFF_BOUND_EPS = 8.0, 8.0


# ---- matrices (CSR: n, row_ptr, col, val) ----------------------------------------------------------------------------------------
def laplacian_2d(m):
    n, r, c, v = solver_ref.laplacian_2d(m)
    return (n,) + solver_ref.csr_arrays(n, r, c, v)


def stencil27(m):
    """27-point stencil on an m^3 grid: faces -1, edges -1/2, corners -1/4, the diagonal 15 (the interior row sum is 1): symmetric,
    strictly diagonally dominant, columns ascending"""
    n = m * m * m
    idx = np.arange(n).reshape(m, m, m)
    rows, cols, vals = [], [], []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                w = 15.0 if (dz, dy, dx) == (0, 0, 0) else -(2.0 ** (1 - abs(dz) - abs(dy) - abs(dx)))
                src = idx[max(0, -dz):m - max(0, dz), max(0, -dy):m - max(0, dy), max(0, -dx):m - max(0, dx)]
                dst = idx[max(0, dz):m - max(0, -dz), max(0, dy):m - max(0, -dy), max(0, dx):m - max(0, -dx)]
                rows.append(src.ravel())
                cols.append(dst.ravel())
                vals.append(np.full(src.size, w))
    r, c, v = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    o = np.lexsort((c, r))
    return (n,) + solver_ref.csr_arrays(n, r[o], c[o], v[o])


def dense_blocks(sizes=(64, 64, 64), seed=41):
    """(n, rp, cc, cv, owner, rank): a block-diagonal matrix of dense SPD blocks B B^T + 64 I, B from multiples of 1/4 in [-1, 1]
    (every entry a multiple of 1/16 below 2^8: exact), the blocks' rows interleaved over the matrix by a random permutation, a
    block's rows in ascending index (ilu0_ref.clique_rank), columns ascending.  Row `rank` of a block has rank + 1 pattern columns."""
    owner, rank = ilu0_ref.clique_rank(sizes, seed)
    n = len(owner)
    by_block = np.argsort(owner, kind="stable")
    rng = np.random.default_rng([seed, 1])
    rows, cols, vals, start = [], [], [], 0
    for s in sizes:
        idx = by_block[start:start + s]
        start += s
        B = rng.integers(-4, 5, (s, s)) / 4.0
        a = B @ B.T + 64.0 * np.eye(s)
        rows.append(np.repeat(idx, s))
        cols.append(np.tile(idx, s))
        vals.append(a.ravel())
    r, c, v = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    o = np.lexsort((c, r))
    return (n,) + solver_ref.csr_arrays(n, r[o], c[o], v[o]) + (owner, rank)


def block_of(n, rp, cc, cv, owner, b):
    """the dense block b of dense_blocks and the indices of its rows"""
    idx = np.flatnonzero(owner == b)
    dense = np.zeros((n, len(idx)))
    where = np.full(n, -1)
    where[idx] = np.arange(len(idx))
    rows = np.repeat(np.arange(n), np.diff(rp))
    sel = where[cc] >= 0
    np.add.at(dense, (rows[sel], where[cc[sel]]), cv[sel])
    return dense[idx], idx


def random_symmetric(n=30_000, k=3, seed=43):
    """B + B^T, k random off-diagonal entries per row of B with dyadic values (one in eight a stored zero), the diagonal
    sum |off| + 1 stored twice (3/4 and 1/4 of it), every row's columns in random order: symmetric, strictly diagonally dominant"""
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(n), k)
    c = rng.integers(0, n, n * k)
    v = rng.integers(-(2**10) + 1, 2**10, n * k) / 2.0**10
    v[rng.random(n * k) < 0.125] = 0.0
    keep = r != c
    r, c, v = r[keep], c[keep], v[keep]
    rr, cc, vv = np.concatenate([r, c]), np.concatenate([c, r]), np.concatenate([v, v])
    dom = np.zeros(n)
    np.add.at(dom, rr, np.abs(vv))
    dom += 1.0
    rr = np.concatenate([rr, np.arange(n), np.arange(n)])
    cc = np.concatenate([cc, np.arange(n), np.arange(n)])
    vv = np.concatenate([vv, 0.75 * dom, 0.25 * dom])
    o = np.lexsort((rng.random(len(rr)), rr))
    return (n,) + solver_ref.csr_arrays(n, rr[o], cc[o], vv[o])


def diagonal_powers_of_four(n=37):
    """diag(4^k), k = -8 .. : G = diag(2^-k) and z = r / d, bit for bit"""
    d = np.ldexp(1.0, 2 * (np.arange(n) % 17 - 8))
    return n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), d


# ---- rows that take a later trip over the grid (tests/tiled.py) ---------------------------------------------------------------------
# per lane class of fsai_rows_kernel the smallest base with rows of that class, and its level: the 5-point Laplacian on 3 x 3
# (m = 1 .. 3), on 8 x 8 at level 2 (m up to 7) and 3 (m up to 13), dense blocks with every m up to 64
GRID_LOOP_BASES = {
    4: (lambda: laplacian_2d(3), 1),
    8: (lambda: laplacian_2d(8), 2),
    16: (lambda: laplacian_2d(8), 3),
    32: (lambda: dense_blocks((64, 47, 27))[:4], 1),
    64: (lambda: dense_blocks((64, 47, 27))[:4], 1),
}


def grid_loop_case(lanes):
    """The base of GRID_LOOP_BASES[lanes] in as many block-diagonal copies as take the groups of `lanes` lanes past kMaxGrid
    workgroups: a dict of the base matrix, its twin, the copies, the rows of the class a copy, the groups a workgroup, and
    where(copy, row) for tiled.tiled_mismatch.  Every threshold comes from the settings headers."""
    import tiled

    build, level = GRID_LOOP_BASES[lanes]
    n, rp, cc, cv = build()
    ref = Fsai(n, rp, cc, cv, level)
    m = np.diff(ref.rp)
    all_lanes = tiled.fsai_lanes()
    cls = np.array([tiled.fsai_class_of(x) for x in m])
    groups = {c: tiled.fsai_groups_per_block(L) for c, L in enumerate(all_lanes)}
    mine = all_lanes.index(lanes)
    rows, grid = int(np.sum(cls == mine)), tiled.max_grid()
    assert rows > 0, f"no row of {lanes} lanes in the base"
    trips = tiled.describe_trips(cls, groups, grid, {c: f"of {L} lanes" for c, L in enumerate(all_lanes)})
    return dict(n=n, rp=rp, cc=cc, cv=cv, level=level, ref=ref, m=m, rows=rows, groups=groups[mine], grid=grid,
                copies=groups[mine] * grid // rows + 1, where=lambda copy, row: f"m = {int(m[row])}, {trips(copy, row)}")


# ---- the two systems whose iteration counts the GPU test compares with --------------------------------------------------------------
REL_TOL = 1e-9
SOLVER_SYSTEMS = ("laplacian_2d_33", "laplacian_3d_12")
# Iterations of the float64 twins (ilu0_ref.run_cg over Fsai.apply) to REL_TOL from x0 = 0, (smallest, largest) over
# solver_ref.DOT_ORDERS, as tests/test_fsai_ref.py::test_iteration_counts_of_the_twins measures them on the CPU (it fails when they
# move).  tests/test_gpu_fsai.py allows the engine one iteration either side of these.
TWIN_ITERATIONS = {
    ("laplacian_2d_33", 1): (64, 64),
    ("laplacian_2d_33", 2): (47, 47),
    ("laplacian_2d_33", 3): (36, 36),
    ("laplacian_3d_12", 1): (30, 30),
    ("laplacian_3d_12", 2): (23, 23),
    ("laplacian_3d_12", 3): (17, 17),
}
UNPRECONDITIONED_ITERATIONS = {"laplacian_2d_33": 111, "laplacian_3d_12": 52}


def solver_system(name):
    """(n, rp, cc, cv, b)"""
    n, rp, cc, cv = laplacian_2d(33) if name == "laplacian_2d_33" else laplacian_3d(12)
    b = np.random.default_rng(5000 + SOLVER_SYSTEMS.index(name)).uniform(-1, 1, n)
    return n, rp, cc, cv, b


def twin_iterations(name, level, max_iter=500):
    """{dot order: iterations to REL_TOL} of the float64 twins; level 0: no preconditioner"""
    n, rp, cc, cv, b = solver_system(name)
    mv = lambda x: csr_mv(n, rp, cc, cv, x)
    apply_m = Fsai(n, rp, cc, cv, level).apply if level else (lambda r: r.copy())
    return {o: run_cg(mv, apply_m, b, REL_TOL, max_iter, dot_order=o)[1] for o in solver_ref.DOT_ORDERS}
