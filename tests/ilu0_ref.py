"""NumPy reference for ILU(0) in sweep order (spmv_ilu0_*; SPMV_PRECOND_ILU0) - TEST INFRASTRUCTURE ONLY (no GPU needed).

The definition the engine is held to (csrc/ilu0.hip states the same): pos[i] is the position of row i in the sweep `order`; the
pattern P is the set of (i, j) with at least one stored entry, duplicates summed first in stored order; the factors are those of
the IKJ elimination restricted to P,

    for i in sweep order:
        for k in row i with pos[k] < pos[i], ascending pos[k]:
            l_ik = a_ik / u_kk
            for j in row k with pos[j] > pos[k]:
                if (i, j) in P:  a_ij = fma(-l_ik, u_kj, a_ij)
        u_ii = a_ii;  u_ij = a_ij for pos[j] > pos[i]

and the application is z = U^-1 L^-1 r: forward through the sweep order with the unit lower triangle, backward with the upper one.
Vectors stay in the matrix's own numbering.

Ilu0 holds the factor values aligned to the CSR entries they came from, as an in-place csrilu0 would leave them (of a set of
duplicates the first stored one carries the value, the others hold 0.0), and applies them.  run_cg and run_bicgstab are the float64
recurrences csrc/solver.hip (three-launch arrangement) and csrc/solver_bicgstab.hip state, with a callable M^-1 and the dot
products summed in one of solver_ref.DOT_ORDERS; they run to the engine's stopping rule and return the iteration count.

One switch exists for the mutation check of tests/test_ilu0_ref.py only: restrict=False eliminates without the pattern
restriction (fill takes part in the elimination and is dropped at the end).
"""
from __future__ import annotations

import math

import numpy as np

from solver_ref import DOT_ORDERS, _dot  # noqa: F401  (the dot orders of the float64 twins)

_fma = getattr(math, "fma", None) or (lambda a, b, c: a * b + c)  # (one rounding more without it: 1e-16, far below any gate here)


class Ilu0:
    def __init__(self, n, rp, cc, cv, order, restrict=True):
        rp, cc, cv = np.asarray(rp, np.int64), np.asarray(cc, np.int64), np.asarray(cv, np.float64)
        order = np.asarray(order, np.int64)
        assert np.array_equal(np.sort(order), np.arange(n)), "the order is not a permutation of the rows"
        pos = np.empty(n, np.int64)
        pos[order] = np.arange(n)
        self.n, self.rp, self.cc, self.order, self.pos = n, rp, cc, order, pos
        kl = pos.tolist()  # (the key of a column: its sweep position)
        # rows as {key of column: value}, duplicates summed in stored order; first[i][key] = the stored entry that carries the value
        rows, first = [None] * n, [None] * n
        cl, vl = cc.tolist(), cv.tolist()
        for i in range(n):
            d, f = {}, {}
            for e in range(rp[i], rp[i + 1]):
                k = kl[cl[e]]
                if k in d:
                    d[k] += vl[e]
                else:
                    d[k] = 0.0 + vl[e]
                    f[k] = e
            if kl[i] not in d:
                raise ValueError(f"row {i} has no diagonal entry")
            rows[i], first[i] = d, f
        upper = [None] * n  # by key of the row: [(key of column, u)] of the finished row, ascending
        for i in order.tolist():
            d, ki = rows[i], kl[i]
            todo = sorted(k for k in d if k < ki)
            seen = 0
            while seen < len(todo):  # (without the restriction fill may add lower entries while the row is eliminated)
                k = todo[seen]
                seen += 1
                uk = upper[k]
                if uk is None:
                    raise ValueError(f"row {i} reads row {int(order[k])}, which the sweep has not finished: not a valid order")
                l = d[k] / rows[int(order[k])][k]
                d[k] = l
                for kj, u in uk:
                    if kj in d:
                        d[kj] = _fma(-l, u, d[kj])
                    elif not restrict:
                        d[kj] = -l * u
                        if kj < ki:
                            todo = sorted(set(todo) | {kj})
            piv = d[ki]
            if piv == 0.0 or not math.isfinite(piv):
                raise ZeroDivisionError(f"the pivot of row {i} is zero or not finite")
            upper[ki] = sorted((k, v) for k, v in d.items() if k > ki)
        self.values = np.zeros(len(cc))
        for i in range(n):
            for k, e in first[i].items():
                self.values[e] = rows[i][k]
        # the triangles for the application: every stored entry takes part (later duplicates hold 0.0)
        r = np.repeat(np.arange(n), np.diff(rp))
        kr, kc = pos[r], pos[cc]
        self._tri = []
        for sel in (kc < kr, kc > kr):
            ptr = np.concatenate([[0], np.cumsum(np.bincount(r[sel], minlength=n))])
            self._tri.append((ptr.tolist(), cc[sel], self.values[sel]))
        self.diag = np.zeros(n)
        np.add.at(self.diag, r[kc == kr], self.values[kc == kr])

    def apply(self, rhs):
        """z = U^-1 L^-1 rhs"""
        z = np.array(rhs, dtype=np.float64)
        (lp, lc, lv), (up, uc, uv) = self._tri
        for i in self.order.tolist():
            a, b = lp[i], lp[i + 1]
            if b > a:
                z[i] -= np.dot(lv[a:b], z[lc[a:b]])
        d = self.diag
        for i in self.order[::-1].tolist():
            a, b = up[i], up[i + 1]
            z[i] = (z[i] - (np.dot(uv[a:b], z[uc[a:b]]) if b > a else 0.0)) / d[i]
        return z

    def product_on_pattern(self):
        """(L U)_ij for every stored entry (i, j), aligned to the CSR entries, from the factor values alone"""
        n, rp, cc, pos = self.n, self.rp, self.cc, self.pos
        r = np.repeat(np.arange(n), np.diff(rp))
        rows = [dict() for _ in range(n)]  # row -> {column: value}, later duplicates add 0.0
        for i, c, v in zip(r.tolist(), cc.tolist(), self.values.tolist()):
            rows[i][c] = rows[i].get(c, 0.0) + v
        out = np.zeros(len(cc))
        for e, (i, j) in enumerate(zip(r.tolist(), cc.tolist())):
            ri, t = rows[i], 0.0
            for k, lik in ri.items():  # sum over k with pos[k] < pos[i] and pos[k] <= pos[j] of l_ik u_kj, plus u_ij where pos[j] >= pos[i]
                if pos[k] < pos[i] and pos[k] < pos[j] and j in rows[k]:
                    t += lik * rows[k][j]
                elif pos[k] < pos[i] and k == j:
                    t += lik * rows[k][k]
            if pos[j] >= pos[i]:
                t += ri[j]
            out[e] = t
        return out


def merged_entries(n, rp, cc, cv):
    """a_ij for every stored entry with its duplicates summed (every duplicate shows the sum), aligned to the CSR entries"""
    r = np.repeat(np.arange(n), np.diff(rp))
    code = r.astype(np.int64) * n + np.asarray(cc, np.int64)
    u, inv = np.unique(code, return_inverse=True)
    s = np.zeros(len(u))
    np.add.at(s, inv, cv)
    return s[inv]


def csr_mv(n, rp, cc, cv, x):
    t = np.asarray(cv) * x[np.asarray(cc)]
    out = np.zeros(n)
    np.add.at(out, np.repeat(np.arange(n), np.diff(rp)), t)
    return out


# ---- the two solvers with a callable M^-1, run to the engine's stopping rule --------------------------------------------------
def run_cg(mv, apply_m, b, rel_tol, max_iter, dot_order="pairwise"):
    """(x, iterations) of csrc/solver.hip's three-launch arrangement from x0 = 0: q = A p; alpha = rz / p.q; x += alpha p;
    r -= alpha q; z = M^-1 r; beta = rz' / rz; p = z + beta p; stops once r.r <= rel_tol^2 b.b, looked at every iteration"""
    dot = lambda a, c: float(_dot(a, c, dot_order))
    x = np.zeros_like(b)
    r = b - mv(x)
    z = apply_m(r)
    p = z.copy()
    rz, bb = dot(r, z), dot(b, b)
    limit = rel_tol * rel_tol * bb
    k = 0
    if dot(r, r) <= limit:
        return x, 0
    while k < max_iter:
        q = mv(p)
        alpha = rz / dot(p, q)
        x = x + alpha * p
        r = r - alpha * q
        k += 1
        if dot(r, r) <= limit:
            break
        z = apply_m(r)
        rz_next = dot(r, z)
        p = z + (rz_next / rz) * p
        rz = rz_next
    return x, k


def run_bicgstab(mv, apply_m, b, rel_tol, max_iter, dot_order="pairwise"):
    """(x, iterations) of csrc/solver_bicgstab.hip from x0 = 0: phat = M^-1 p; v = A phat; alpha = rho / rhat.v; s = r - alpha v;
    shat = M^-1 s; t = A shat; omega = t.s / t.t (0 where t.t = 0); x += alpha phat + omega shat; r = s - omega t; rho' = rhat.r;
    beta = (rho' / rho)(alpha / omega); p = r + beta (p - omega v); stops once r.r <= rel_tol^2 b.b, looked at every iteration"""
    dot = lambda a, c: float(_dot(a, c, dot_order))
    x = np.zeros_like(b)
    r = b - mv(x)
    rhat, p = r.copy(), r.copy()
    bb = dot(b, b)
    rho = dot(r, r)
    limit = rel_tol * rel_tol * bb
    k = 0
    if rho <= limit:
        return x, 0
    while k < max_iter:
        phat = apply_m(p)
        v = mv(phat)
        alpha = rho / dot(rhat, v)
        s = r - alpha * v
        shat = apply_m(s)
        t = mv(shat)
        tt = dot(t, t)
        omega = dot(t, s) / tt if tt != 0.0 else 0.0
        x = x + alpha * phat + omega * shat
        r = s - omega * t
        k += 1
        if dot(r, r) <= limit or omega == 0.0:
            break
        rho_new = dot(rhat, r)
        p = r + (rho_new / rho) * (alpha / omega) * (p - omega * v)
        rho = rho_new
    return x, k


# ---- orders -------------------------------------------------------------------------------------------------------------
def greedy_colour_order(n, rp, cc):
    """the sequential greedy colouring the engine's relaxation ends at: colour(i) = the smallest colour no coupled row j < i has;
    returns (colours, colour, sequence: colour by colour, ascending row index inside a colour)"""
    colour = np.zeros(n, np.int64)
    cl, rl = np.asarray(cc).tolist(), np.asarray(rp).tolist()
    col_l = [0] * n
    for i in range(n):
        used = {col_l[c] for c in cl[rl[i]:rl[i + 1]] if c < i}
        m = 0
        while m in used:
            m += 1
        col_l[i] = m
    colour[:] = col_l
    return int(colour.max()) + 1 if n else 0, colour, np.argsort(colour, kind="stable")


# ---- matrices (CSR: n, row_ptr, col, val) ----------------------------------------------------------------------------------
def from_dense(dense):
    n = dense.shape[0]
    r, c = np.nonzero(dense)
    rp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int32)
    return n, rp, c.astype(np.int32), dense[r, c].astype(np.float64)


def tridiagonal_8():
    n = 8
    return from_dense(2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1))


def tridiagonal_nonsym(n=33):
    """diagonal 3, -1.5 below it, -0.5 above: a nonsymmetric M-matrix"""
    return from_dense(3.0 * np.eye(n) - 1.5 * np.eye(n, k=-1) - 0.5 * np.eye(n, k=1))


def laplacian_3d(m):
    """7-point Laplacian on an m^3 grid, CSR, columns ascending (tests/test_gpu_solver.py: _laplacian_3d)"""
    n = m * m * m
    idx = np.arange(n).reshape(m, m, m)
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [np.full(n, 6.0)]
    for a, b in ((idx[:, :, :-1], idx[:, :, 1:]), (idx[:, :-1, :], idx[:, 1:, :]), (idx[:-1, :, :], idx[1:, :, :])):
        rows += [a.ravel(), b.ravel()]
        cols += [b.ravel(), a.ravel()]
        vals += [np.full(a.size, -1.0)] * 2
    r, c, v = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    o = np.lexsort((c, r))
    r, c, v = r[o], c[o], v[o]
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, r + 1, 1)
    return n, np.cumsum(rp).astype(np.int32), c.astype(np.int32), v


def dominant_random(n, k, seed, unsorted=True):
    """NON-symmetric pattern, k random off-diagonal entries per row in random order, the diagonal entry given twice (duplicates
    are summed), strictly diagonally dominant (tests/test_gpu_solver.py: _dominant_random)"""
    rng = np.random.default_rng(seed)
    cols = rng.integers(0, n, (n, k))
    vals = rng.uniform(-1, 1, (n, k))
    rows = np.repeat(np.arange(n), k).reshape(n, k)
    vals[cols == rows] = 0.0  # an accidental diagonal hit: keep the slot, drop its weight
    dom = np.abs(vals).sum(axis=1) + 1.0
    cc = np.concatenate([cols, rows[:, :1], rows[:, :1]], axis=1)
    cv = np.concatenate([vals, (0.75 * dom)[:, None], (0.25 * dom)[:, None]], axis=1)
    if unsorted:
        perm = np.argsort(rng.uniform(size=cc.shape), axis=1)
        cc, cv = np.take_along_axis(cc, perm, 1), np.take_along_axis(cv, perm, 1)
    rp = (np.arange(n + 1) * (k + 2)).astype(np.int32)
    return n, rp, cc.ravel().astype(np.int32), cv.ravel()


def lower_triangular_cut(n, k, seed):
    """the entries of dominant_random(n, k, seed) on and below the diagonal"""
    n, rp, cc, cv = dominant_random(n, k, seed)
    rows = np.repeat(np.arange(n), np.diff(rp))
    keep = cc <= rows
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int32)
    return n, rp, cc[keep], cv[keep]


def band33(n=4099, seed=7):
    """33 diagonals (offsets -16 .. 16) of an n x n matrix, values as cgls_ref.band draws them (multiples of 2^-20 in (-1, 1)), the
    main one 32 + 2^-10: strictly diagonally dominant, 33 entries per interior row, 16 in either triangle"""
    offs = np.arange(-16, 17)
    rng = np.random.default_rng(seed)
    i = np.repeat(np.arange(n), len(offs))
    off = np.tile(offs, n)
    v = rng.integers(-(2**20) + 1, 2**20, len(i)) / 2.0**20
    v[off == 0] = 32.0 + 2.0**-10
    j = i + off
    keep = (j >= 0) & (j < n) & (v != 0)
    i, j, v = i[keep], j[keep], v[keep]
    rp = np.searchsorted(i, np.arange(n + 1)).astype(np.int32)
    return n, rp, j.astype(np.int32), v


def convection_diffusion_2d(m, cx=1.5, cy=0.5):
    """5-point diffusion plus first-order upwind convection with the velocity (cx, cy) > 0 on an m x m grid, Dirichlet boundary:
    diagonal 4 + cx + cy everywhere (constant: Jacobi is a scaling), west -(1 + cx), east -1, south -(1 + cy), north -1.  A
    nonsymmetric M-matrix, columns ascending"""
    n = m * m
    idx = np.arange(n).reshape(m, m)
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [np.full(n, 4.0 + cx + cy)]
    for lo, hi, w_lo, w_hi in ((idx[:, :-1], idx[:, 1:], -(1.0 + cx), -1.0), (idx[:-1, :], idx[1:, :], -(1.0 + cy), -1.0)):
        rows += [hi.ravel(), lo.ravel()]  # the later point sees the earlier one upwind
        cols += [lo.ravel(), hi.ravel()]
        vals += [np.full(lo.size, w_lo), np.full(lo.size, w_hi)]
    r, c, v = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    o = np.lexsort((c, r))
    r, c, v = r[o], c[o], v[o]
    return n, np.searchsorted(r, np.arange(n + 1)).astype(np.int32), c.astype(np.int32), v


# ---- the two systems whose iteration counts the GPU test compares with ------------------------------------------------------------
REL_TOL = 1e-9
SOLVER_SYSTEMS = ("bicgstab_convdiff40", "cg_laplacian12")
# Iterations of the float64 twins to REL_TOL from x0 = 0, (smallest, largest) over solver_ref.DOT_ORDERS, as
# tests/test_ilu0_ref.py::test_iteration_counts_of_the_twins measures and prints them on the CPU (it fails when they move).
# Order 0 is the matrix's own row order, 1 the multicolour order.  Without a preconditioner and with Jacobi (a constant diagonal)
# both systems take 67 and 53 iterations.  tests/test_gpu_ilu0.py allows the engine one iteration either side of these.
TWIN_ITERATIONS = {
    ("bicgstab_convdiff40", 0): (15, 15),
    ("bicgstab_convdiff40", 1): (33, 33),
    ("cg_laplacian12", 0): (20, 20),
    ("cg_laplacian12", 1): (26, 26),
}
UNPRECONDITIONED_ITERATIONS = {"bicgstab_convdiff40": 67, "cg_laplacian12": 53}


def solver_system(name):
    """(solver, n, rp, cc, cv, b)"""
    if name == "bicgstab_convdiff40":
        n, rp, cc, cv = convection_diffusion_2d(40)
        solver = "bicgstab"
    elif name == "cg_laplacian12":
        n, rp, cc, cv = laplacian_3d(12)
        solver = "cg"
    else:
        raise KeyError(name)
    b = np.random.default_rng(3000 + SOLVER_SYSTEMS.index(name)).uniform(-1, 1, n)
    return solver, n, rp, cc, cv, b


def twin_iterations(name, order, precond="ilu0", max_iter=500):
    """{dot order: iterations to REL_TOL} of the float64 twins on one of SOLVER_SYSTEMS; order: the sweep order (array), ignored
    unless precond is "ilu0"; precond "none" and "jacobi" for the table of the CPU test"""
    solver, n, rp, cc, cv, b = solver_system(name)
    mv = lambda x: csr_mv(n, rp, cc, cv, x)
    if precond == "ilu0":
        apply_m = Ilu0(n, rp, cc, cv, order).apply
    elif precond == "jacobi":
        d = np.zeros(n)
        rows = np.repeat(np.arange(n), np.diff(rp))
        np.add.at(d, rows[rows == cc], cv[rows == cc])
        apply_m = lambda r: r / d
    else:
        apply_m = lambda r: r.copy()
    run = run_bicgstab if solver == "bicgstab" else run_cg
    return {o: run(mv, apply_m, b, REL_TOL, max_iter, dot_order=o)[1] for o in DOT_ORDERS}


# ---- matrices ILU(0) factorises EXACTLY: A = (I + L) U from small dyadic numbers on a pattern that takes no fill ------------------
# L: multiples of 1/4 in [-3/4, 3/4]; U off its diagonal: integers in [-3, 3]; U's diagonal: +-{1/2, 1, 2, 4}, so every division
# of the elimination and of the backward solve is by a power of two.  Every term l_ik u_kj is a multiple of 2^-2, A's entries are
# sums of a handful of them, and a split entry is stored as two multiples of 2^-4 that sum to it: all of it on the grid 2^-EXACT_G,
# orders of magnitude below the 2^53 budget (assert_exact_budget counts, in integers).  ILU(0) of such a matrix must return L and U
# themselves and its application to r = A z, z integers, z itself - whatever the lanes, the tree or the order of a sum.
EXACT_G, EXACT_G_L, EXACT_G_U = 4, 2, 0
EXACT_G_DIAG = 1  # (U's diagonal alone is on the grid 2^-1)


def _dyadic_lu_values(rng, shape_l, shape_u, shape_d):
    l = rng.integers(-3, 4, shape_l) / 4.0
    u = rng.integers(-3, 4, shape_u).astype(np.float64)
    d = np.where(rng.random(shape_d) < 0.5, -1.0, 1.0) * np.ldexp(1.0, rng.integers(-1, 3, shape_d))
    return l, u, d


def _store_exact(rng, n, r, c, a, f, split=0.2):
    """CSR of the entries (r, c, a) with their factor values f: about `split` of them stored as two duplicates whose dyadic parts sum
    exactly, the entries of a row in random order; expected[e] = f for the first stored entry of a position, 0.0 for a later one"""
    two = np.flatnonzero(rng.random(len(r)) < split)
    part = rng.integers(-64, 65, len(two)) / 16.0  # (a zero part, and a zero rest, are stored zeros like any other)
    v = a.copy()
    v[two] = part
    r, c, v, f = np.concatenate([r, r[two]]), np.concatenate([c, c[two]]), np.concatenate([v, a[two] - part]), np.concatenate([f, f[two]])
    o = np.lexsort((rng.random(len(r)), r))
    r, c, v, f = r[o], c[o], v[o], f[o]
    firsts = np.zeros(len(r), bool)
    firsts[np.unique(r.astype(np.int64) * n + c, return_index=True)[1]] = True
    rp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int32)
    return n, rp, c.astype(np.int32), v, np.where(firsts, f, 0.0)


def clique_rank(sizes, seed):
    """(block of every row, its rank inside the block) of clique_blocks(sizes, seed): a random permutation deals the rows 0 .. n-1 out
    to the blocks, a block's rows in ascending index.  Greedy colouring in row order gives a row its rank as colour."""
    sizes = np.asarray(sizes, np.int64)
    owner = np.random.default_rng(seed).permutation(np.repeat(np.arange(len(sizes)), sizes))
    by_block = np.argsort(owner, kind="stable")
    rank = np.empty(len(owner), np.int64)
    rank[by_block] = np.arange(len(owner)) - np.repeat(np.cumsum(sizes) - sizes, sizes)
    return owner, rank


def clique_blocks(sizes, seed, split=0.2):
    """(n, rp, cc, cv, expected factors): a block-diagonal matrix of dense blocks A_b = (I + L_b) U_b, the blocks' rows interleaved
    (clique_rank), every position of a block stored, zeros included.  A dense block takes no fill in any order, and both sweep orders
    eliminate a block in its construction order: exact in both."""
    owner, rank = clique_rank(sizes, seed)
    n = len(owner)
    by_block = np.argsort(owner, kind="stable")
    rng = np.random.default_rng([seed, 1])
    rs, cs, vs, fs = [], [], [], []
    start = 0
    for s in np.asarray(sizes, np.int64).tolist():
        idx = by_block[start:start + s]
        start += s
        l, u, d = _dyadic_lu_values(rng, (s, s), (s, s), s)
        l, u = np.tril(l, -1), np.triu(u, 1) + np.diag(d)
        a = (np.eye(s) + l) @ u  # (exact: every partial sum is a small multiple of 2^-3)
        rs.append(np.repeat(idx, s))
        cs.append(np.tile(idx, s))
        vs.append(a.ravel())
        fs.append((l + u).ravel())
    cat = lambda x, t: np.concatenate(x).astype(t) if x else np.zeros(0, t)
    return _store_exact(rng, n, cat(rs, np.int64), cat(cs, np.int64), cat(vs, np.float64), cat(fs, np.float64), split)


def band_lu(n, p, q, seed, split=0.2):
    """(n, rp, cc, cv, expected factors): A = (I + L) U with p sub-diagonals in L and q super-diagonals in U, the whole band
    -p .. q stored (products that happen to be zero included): no fill in ROW ORDER, where ILU(0) is the LU factorisation.  Not
    diagonally dominant: not for the multicolour order."""
    rng = np.random.default_rng([seed, 2])
    l, u, d = _dyadic_lu_values(rng, (p + 1, n), (q + 1, n), n)  # l[k][i] = L[i, i - k], u[e][i] = U[i, i + e]
    l[0], u[0] = 1.0, d
    i = np.arange(n)
    for k in range(1, p + 1):
        l[k][i < k] = 0.0
    for e in range(1, q + 1):
        u[e][i + e >= n] = 0.0
    rs, cs, vs, fs = [], [], [], []
    for off in range(-p, q + 1):
        a = np.zeros(n)
        for k in range(max(0, -off), p + 1):  # A[i, i + off] = sum_k L[i, i - k] U[i - k, i + off]
            e = off + k
            if e > q:
                break
            src = i - k
            ok = src >= 0
            a[ok] += l[k][ok] * u[e][src[ok]]
        keep = (i + off >= 0) & (i + off < n)
        rs.append(i[keep])
        cs.append(i[keep] + off)
        vs.append(a[keep])
        fs.append((l[-off] if off < 0 else u[off])[keep])
    return _store_exact(rng, n, np.concatenate(rs), np.concatenate(cs), np.concatenate(vs), np.concatenate(fs), split)


def integer_vector(n, seed):
    """z: integers in [-8, 8]"""
    return np.random.default_rng([seed, 3]).integers(-8, 9, n).astype(np.float64)


def _scaled(a, g, what):
    s = np.ldexp(np.asarray(a, np.float64), g)
    if not (np.all(np.isfinite(s)) and np.array_equal(s, np.round(s)) and (s.size == 0 or np.max(np.abs(s)) < 2.0**53)):
        raise AssertionError(f"{what}: not on the grid 2^-{g}")
    return s.astype(np.int64)


def assert_exact_budget(n, rp, cc, cv, expected, order, z, g=EXACT_G, g_l=EXACT_G_L, g_u=EXACT_G_U, g_d=EXACT_G_DIAG):
    """The conditions under which the elimination and both solves are exact in any order of any sum, checked in INTEGER arithmetic
    (values scaled by 2^g; tests/exact.py does the same for the products): with the expected factors L (grid 2^-g_l), U (2^-g_u off
    the diagonal, +- a power of two on it, grid 2^-g_d) and the stored values (2^-g),
      - no fill: wherever (i, k) and (k, j) are in the pattern with k before i and j in the sweep, (i, j) is;
      - the matrix is the product: sum of the stored duplicates of (i, j) = sum_k l_ik u_kj (+ u_ij), as integers, so the
        elimination - which subtracts exactly these terms from exactly these sums, and divides by powers of two - ends at L and U;
      - every term of it is a multiple of 2^-g and |stored parts| + sum |l_ik u_kj| stays below 2^(53 - g), so every partial sum is
        a float64, whatever came first;
      - the same for r = A z, the forward solve (r_i and the terms l_ik y_k, y = U z) and the backward one (y_i and u_ij z_j).
    Returns the largest of those magnitudes as a number of bits (53 is the budget)."""
    assert g >= g_l + max(g_u, g_d)
    rp, cc, cv = np.asarray(rp, np.int64), np.asarray(cc, np.int64), np.asarray(cv, np.float64)
    order = np.asarray(order, np.int64)
    pos = np.empty(n, np.int64)
    pos[order] = np.arange(n)
    rows = np.repeat(np.arange(n), np.diff(rp))
    code, ia = rows * n + cc, _scaled(cv, g, "a stored value")
    u_code, first, inv = np.unique(code, return_index=True, return_inverse=True)
    firsts = np.zeros(len(cc), bool)
    firsts[first] = True
    assert np.all(np.asarray(expected)[~firsts] == 0.0), "a later duplicate carries a factor value"
    a_sum, a_mag = np.zeros(len(u_code), np.int64), np.zeros(len(u_code), np.int64)
    np.add.at(a_sum, inv, ia)
    np.add.at(a_mag, inv, np.abs(ia))
    mr, mc, f = u_code // n, u_code % n, np.asarray(expected, np.float64)[first]  # the merged pattern, row by row
    kr, kc = pos[mr], pos[mc]
    il = _scaled(np.where(kc < kr, f, 0.0), g_l, "an entry of L") << (g - g_l)  # on the grid 2^-g ...
    iu = _scaled(np.where(kc > kr, f, 0.0), g_u, "an entry of U") << (g - g_l - g_u)  # ... and 2^-(g - g_l): l u is on 2^-g again
    idg = _scaled(np.where(kc == kr, f, 0.0), g_d, "a pivot") << (g - g_l - g_d)
    piv = np.abs(idg[kc == kr])
    assert len(piv) == n and np.all(piv > 0) and np.all(piv & (piv - 1) == 0), "a pivot is not +- a power of two"
    iu = iu + idg  # U with its diagonal, grid 2^-(g - g_l)
    mptr = np.searchsorted(mr, np.arange(n + 1))
    up_of = [None] * n  # row k: (columns, values) of its part on and after the diagonal
    for k in range(n):
        sel = np.arange(mptr[k], mptr[k + 1])
        sel = sel[kc[sel] >= kr[sel]]
        up_of[k] = (mc[sel], iu[sel])
    slot = np.full(n, -1, np.int64)
    worst = 1
    for i in range(n):
        b, e = mptr[i], mptr[i + 1]
        slot[mc[b:e]] = np.arange(e - b)
        acc = np.where(kc[b:e] >= kr[b:e], iu[b:e] << g_l, 0)  # the row of I times U
        mag = a_mag[b:e] + 0
        for t in np.flatnonzero(kc[b:e] < kr[b:e]).tolist():
            cols, vals = up_of[mc[b + t]]
            s = slot[cols]
            assert np.all(s >= 0), f"fill: row {i} through row {int(mc[b + t])}"
            term = (il[b + t] >> (g - g_l)) * vals  # l (grid 2^-g_l) times u (grid 2^-(g - g_l)): grid 2^-g
            acc[s] += term
            mag[s] += np.abs(term)
        assert np.array_equal(acc, a_sum[b:e]), f"row {i}: the stored values are not those of (I + L) U"
        worst = max(worst, int(mag.max()))
        slot[mc[b:e]] = -1
    # the solves: r = A z; L y = r with y = U z; U z = y
    iz = _scaled(z, 0, "z")
    t = np.abs(ia * iz[cc])
    r_mag = np.zeros(n, np.int64)
    np.add.at(r_mag, rows, t)
    iy = np.zeros(n, np.int64)  # y = U z on the grid 2^-(g - g_l)
    np.add.at(iy, mr, iu * iz[mc])
    ir = np.zeros(n, np.int64)
    np.add.at(ir, rows, ia * iz[cc])
    fwd, bwd = np.abs(ir), np.abs(iy) << g_l
    ly = np.zeros(n, np.int64)
    np.add.at(ly, mr, (il >> (g - g_l)) * iy[mc])
    np.add.at(fwd, mr, np.abs((il >> (g - g_l)) * iy[mc]))
    np.add.at(bwd, mr, np.abs(np.where(kc > kr, iu, 0) * iz[mc]) << g_l)
    assert np.array_equal(ir, ly + (iy << g_l)), "r = A z is not (I + L) (U z)"
    worst = max(worst, int(r_mag.max(initial=0)), int(fwd.max(initial=0)), int(bwd.max(initial=0)))
    assert worst < 2**53, f"a sum needs {math.log2(worst):.1f} bits on the grid 2^-{g} (budget 53)"
    return math.log2(worst)


# ---- the levels and launches tri_levels.hpp must find ------------------------------------------------------------------------------
SMALL_LEVEL, LANE_STEPS = 4096, ((2.5, 1), (12.0, 4))  # csrc/tri_levels.hpp: kSmallLevel; lanes 1 / 4 / 16 by entries per row


def level_sizes(n, rp, cc, order, merged=True):
    """The dependency levels of both triangles in a sweep order and the schedule csrc/tri_levels.hpp's rule makes of them:
    level(i) = 1 + the largest level among the rows that row i's triangle names (0 without any); lanes per row 1, 4 or 16 for up to
    2.5, up to 12 and more entries per row on average (merged: duplicates counted once, as ILU(0) stores its triangles; the
    Gauss-Seidel sweep keeps them); levels of up to 4096 lanes are folded, run by run, into one launch, every other level is a launch
    of its own.  Returns {"lower" / "upper": rows per level, "lanes": (lower, upper), "schedule": ([(first level, levels)], same),
    "launches": of one application}"""
    rp, cc, order = np.asarray(rp, np.int64), np.asarray(cc, np.int64), np.asarray(order, np.int64)
    pos = np.empty(n, np.int64)
    pos[order] = np.arange(n)
    rows = np.repeat(np.arange(n), np.diff(rp))
    if merged:
        code = np.unique(rows * max(n, 1) + cc)
        rows, cc = code // max(n, 1), code % max(n, 1)
    out = {"lanes": [], "schedule": [], "launches": 0}
    for name, sel, sweep in (("lower", pos[cc] < pos[rows], order), ("upper", pos[cc] > pos[rows], order[::-1])):
        r, c = rows[sel], cc[sel]
        ptr = np.searchsorted(r, np.arange(n + 1)).tolist()  # (rows ascends)
        cl, lev = c.tolist(), [0] * n
        for i in sweep.tolist():
            a, b = ptr[i], ptr[i + 1]
            if b > a:
                lev[i] = 1 + max(lev[j] for j in cl[a:b])
        hist = np.bincount(np.asarray(lev, np.int64), minlength=1) if n else np.zeros(0, np.int64)
        avg = len(r) / n if n else 0.0
        lanes = next((w for bound, w in LANE_STEPS if avg <= bound), 16)
        sched, lv = [], 0
        while lv < len(hist):
            end = lv
            while end < len(hist) and hist[end] * lanes <= SMALL_LEVEL:
                end += 1
            end = max(end, lv + 1)  # (a level above the bound: alone)
            sched.append((lv, end - lv))
            lv = end
        out[name] = hist
        out["lanes"].append(lanes)
        out["schedule"].append(sched)
        out["launches"] += len(sched)
    out["lanes"] = tuple(out["lanes"])
    return out


# ---- the exact cases tests/test_gpu_ilu0_exact.py runs on the GPU and tests/test_ilu0_ref.py checks on the CPU --------------------
def _mixed_sizes(count, top, seed, extra=()):
    return np.random.default_rng([seed, 4]).integers(1, top + 1, count).tolist() + list(extra)


EXACT_CLIQUES = {  # name: (block sizes, seed)
    "cliques_130": ([1, 2, 27, 65, 130], 130),
    "cliques_mixed": (_mixed_sizes(1500, 6, 131, [130, 70]), 131),
    "cliques_12": ([12] * 60 + [1] * 5, 132),
    "cliques_tiny": (_mixed_sizes(6000, 3, 133), 133),
}
EXACT_BANDS = {  # name: (n, sub-diagonals of L, super-diagonals of U, seed); row order only
    "band_1_20": (5000, 1, 20, 140),
    "band_20_1": (5000, 20, 1, 141),
    "band_3_3": (3000, 3, 3, 142),
}
EXACT_CASES = [(name, order) for name in EXACT_CLIQUES for order in (0, 1)] + [(name, 0) for name in EXACT_BANDS]


def exact_case(name):
    """(n, rp, cc, cv, expected factors, z)"""
    if name in EXACT_CLIQUES:
        sizes, seed = EXACT_CLIQUES[name]
        m = clique_blocks(sizes, seed)
    else:
        n, p, q, seed = EXACT_BANDS[name]
        m = band_lu(n, p, q, seed)
    return m + (integer_vector(m[0], seed),)
