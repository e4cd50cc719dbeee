"""References for the least-squares solver (spmv_cgls) - TEST INFRASTRUCTURE ONLY (no GPU needed).  The CGLS twin of
tests/solver_ref.py, whose arithmetic helpers, gate factor and floor it takes over unchanged.

cgls_reference is textbook CGLS for min ||b - A x||^2 + damp^2 ||x||^2 over an entry list (any shape, duplicates allowed: every
entry is one product of the sums, as the engine's products take them) in extended precision - np.longdouble, mpmath where
solver_ref.available says so - written as csrc/solver_cgls.hip states it:

    r = b - A x;  s = A^T r - damp^2 x;  p = s;  gamma = s.s
    loop:  q = A p;  delta = q.q + damp^2 p.p;  alpha = gamma / delta;  x += alpha p;  r -= alpha q;  s = A^T r - damp^2 x;
           gamma' = s.s;  beta = gamma' / gamma;  p = s + beta p;  gamma = gamma'

It returns x_k, sqrt(gamma_k / ||A^T b||^2) and sqrt(r_k.r_k / b.b) after exactly k iterations, for every k asked for.

The float64 TWINS are the same recurrence in numpy float64 with two things varied: the order of the dot products (forward,
reversed, pairwise) and the order in which the products of a row of A (of a column, for A^T) are added - as stored and reversed -
because the engine's product kernels add in other orders than numpy does.  Envelope.gate(k) = F * max(FLOOR, the largest deviation
of a twin's x_k from the extended-precision x_k), with F = 8 and FLOOR = 2^-50 from solver_ref.py.  It is measured on this file's
arithmetic and never on the engine: an engine iterate beyond it is a finding to explain, not a reason to raise F.
"""
from __future__ import annotations

import numpy as np

from solver_ref import DOT_ORDERS, F, FLOOR, _conv, _dot, _hp_kind, _sqrt, _xdev, available  # noqa: F401

ROW_ORDERS = ("stored", "reversed")
KS = (1, 2, 3, 4, 5, 8, 9, 13)


def _segment_sums(t, ptr):
    """sums of t[ptr[i] : ptr[i + 1]], empty segments 0"""
    out = np.zeros(len(ptr) - 1, dtype=t.dtype) if t.dtype != object else _conv(np.zeros(len(ptr) - 1), "mp")
    has = ptr[1:] > ptr[:-1]
    if has.any():
        out[has] = np.add.reduceat(t, ptr[:-1][has])
    return out


class Operator:
    """A (m x n) of an entry list in one arithmetic: mv(x) = A x with a row's products added in stored or reversed order,
    rmv(y) = A^T y with a column's products added in row order or reversed"""

    def __init__(self, entries, shape, kind, row_order="stored"):
        row, col, val = (np.asarray(a) for a in entries)
        row, col = row.astype(np.int64), col.astype(np.int64)
        m, n = shape
        assert len(row) == 0 or (row.min() >= 0 and row.max() < m and col.min() >= 0 and col.max() < n)
        self.shape, self.kind, self.row_order = (m, n), kind, row_order
        v = _conv(val, kind)
        idx = np.arange(len(row))
        if row_order == "reversed":
            idx = idx[::-1]
        by_row = idx[np.argsort(row[idx], kind="stable")]
        by_col = idx[np.argsort(col[idx], kind="stable")]
        self.f_col, self.f_val, self.f_ptr = col[by_row], v[by_row], np.searchsorted(row[by_row], np.arange(m + 1))
        self.t_row, self.t_val, self.t_ptr = row[by_col], v[by_col], np.searchsorted(col[by_col], np.arange(n + 1))

    def mv(self, x):
        return _segment_sums(self.f_val * x[self.f_col], self.f_ptr)

    def rmv(self, y):
        return _segment_sums(self.t_val * y[self.t_row], self.t_ptr)


MUTATIONS = ("beta", "nodamp", "stale_s", "tail")


def run_cgls(Op: Operator, b, x0, ks, damp, dot_order="pairwise", mutate=None):
    """({k: (x_k, sqrt(gamma_k / ||A^T b||^2), sqrt(r_k.r_k / b.b))}, the two residual histories for every k up to max(ks)).
    mutate (the mutation check): "beta" gamma / gamma' instead of gamma' / gamma; "nodamp" delta without damp^2 p.p; "stale_s" the
    transposed product added on top of the previous s instead of -damp^2 x; "tail" the last element of x never updated"""
    kind = Op.kind
    dot = lambda a, c: _dot(a, c, dot_order)
    b, x = _conv(b, kind), _conv(x0, kind)
    d2 = _conv(np.array([damp]), kind)[0] ** 2
    ks = set(ks)
    atb = Op.rmv(b)
    atb2, bb = dot(atb, atb), dot(b, b)
    r = b - Op.mv(x)
    s = Op.rmv(r) - d2 * x
    p = s.copy()
    gamma = dot(s, s)
    out, nhist, rhist = {}, [], []

    def record(k):
        nres, res = float(_sqrt(gamma / atb2, kind)), float(_sqrt(dot(r, r) / bb, kind))
        nhist.append(nres)
        rhist.append(res)
        if k in ks:
            out[k] = (x.copy(), nres, res)

    record(0)
    for k in range(max(ks)):
        q = Op.mv(p)
        delta = dot(q, q) if mutate == "nodamp" else dot(q, q) + d2 * dot(p, p)
        alpha = gamma / delta
        xn = x + alpha * p
        if mutate == "tail":
            xn[-1] = x[-1]
        x = xn
        r = r - alpha * q
        s = (s if mutate == "stale_s" else -d2 * x) + Op.rmv(r)
        gamma_new = dot(s, s)
        beta = gamma / gamma_new if mutate == "beta" else gamma_new / gamma
        p = s + beta * p
        gamma = gamma_new
        record(k + 1)
    return out, nhist, rhist


def cgls_reference(entries, shape, b, x0, ks, damp=0.0, force_mp=False):
    """{k: (x_k in the reference's precision, sqrt(gamma_k / ||A^T b||^2), sqrt(r_k.r_k / b.b))} after exactly k iterations"""
    kind = _hp_kind(max(shape), force_mp)
    return run_cgls(Operator(entries, shape, kind), b, x0, ks, damp)[0]


class Envelope:
    """the extended-precision iterates of one problem, and how far the float64 twins stray from them"""

    def __init__(self, entries, shape, b, x0, ks, damp=0.0, force_mp=False, row_orders=ROW_ORDERS):
        self.ks = tuple(ks)
        kind = _hp_kind(max(shape), force_mp)
        ref, self.nres_hist, self.resid_hist = run_cgls(Operator(entries, shape, kind), b, x0, ks, damp)
        self.ref_x = {k: v[0] for k, v in ref.items()}
        self.ref_nres = {k: v[1] for k, v in ref.items()}
        self.ref_resid = {k: v[2] for k, v in ref.items()}
        self.twin_dev = {k: {} for k in ks}  # k -> twin name -> (x, normal residual, residual) deviations
        for row_order in row_orders:
            Op = Operator(entries, shape, "f64", row_order)
            for order in DOT_ORDERS:
                out, _, _ = run_cgls(Op, b, x0, ks, damp, dot_order=order)
                for k in ks:
                    self.twin_dev[k][f"{row_order}/{order}"] = (self.x_dev(k, out[k][0]), self.nres_dev(k, out[k][1]), self.resid_dev(k, out[k][2]))

    def x_dev(self, k, x):
        """max |x - ref_k| / max |ref_k|"""
        return _xdev(x, self.ref_x[k])

    @staticmethod
    def _dev(res, ref, hist, k):
        # solver_ref.Envelope.resid_dev's construction: the scale is the reference's value, or a quarter of the one before it
        return abs(res - ref[k]) / max(ref[k], hist[k - 1] / 4 if k else 0.0, 1e-300)

    def nres_dev(self, k, res):
        return self._dev(res, self.ref_nres, self.nres_hist, k)

    def resid_dev(self, k, res):
        return self._dev(res, self.ref_resid, self.resid_hist, k)

    def envelope(self, k, what=0):
        return max(FLOOR, max(d[what] for d in self.twin_dev[k].values()))

    def gate(self, k):
        return F * self.envelope(k, 0)

    def gate_nres(self, k):
        return F * self.envelope(k, 1)

    def gate_resid(self, k):
        return F * self.envelope(k, 2)


# ---- the problems of tests/test_gpu_cgls.py (entry lists with dyadic values; shared with the CPU checks) ---------------------------
def rect(m, n, k, seed):
    """k random entries per row (multiples of 2^-20 in (-1, 1), duplicates allowed) and one dominant entry per row at column
    i mod n, of magnitude 2 * sum |off| + 2^-10 (exact): (row, col, val) grouped by row, columns in random order within a row.
    Full column rank for m >= n (the first n rows are strictly dominant); for m < n the columns >= m carry random entries only."""
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(m), k)
    c = rng.integers(0, n, m * k)
    v = rng.integers(-(2**20) + 1, 2**20, m * k) / 2.0**20
    dom = np.zeros(m)
    np.add.at(dom, r, np.abs(v))
    dom = 2 * dom + 2.0**-10
    rr, cc, vv = np.concatenate([r, np.arange(m)]), np.concatenate([c, np.arange(m) % n]), np.concatenate([v, dom])
    o = np.lexsort((rng.random(len(rr)), rr))
    return rr[o], cc[o], vv[o]


BAND_OFFSETS = (-8, -5, -3, -1, 0, 2, 3)


def band(m, n, seed):
    """seven diagonals of an m x n matrix (m >= n: every row keeps at least one entry, every column lies below the DIA product's
    column bound), the main one the largest: (row, col, val) in (row, diagonal) order, no duplicates"""
    assert m >= n and m - n < 8
    rng = np.random.default_rng(seed)
    i = np.repeat(np.arange(m), len(BAND_OFFSETS))
    off = np.tile(np.array(BAND_OFFSETS), m)
    v = rng.integers(-(2**20) + 1, 2**20, len(i)) / 2.0**20
    v[off == 0] = 4.0 + 2.0**-10  # (the six others sum to less than 6: CGLS is still far from the noise floor at k = 13)
    j = i + off
    keep = (j >= 0) & (j < n) & (v != 0)
    return i[keep], j[keep], v[keep]


PROBLEMS = ("s1x1", "s2x1", "s3x2", "r33x17", "r4097x4097", "r6001x4097", "r4097x6001", "band4099", "big")


def problem(name, big_shape=None):
    """(shape, (row, col, val), b, x0, ks): the least-squares problems of the step-by-step tests with a random right-hand side and
    a random non-zero start.  The small problems end at iteration min(m, n), so only k <= min(m, n) is asked of them."""
    seed = 2000 + PROBLEMS.index(name)
    if name.startswith("s"):
        m, n = (int(t) for t in name[1:].split("x"))
        dense = {(1, 1): [[3.0]], (2, 1): [[2.0], [-0.5]], (3, 2): [[3.0, -1.0], [0.5, 4.0], [-0.25, 1.5]]}[m, n]
        dense = np.array(dense)
        row, col = np.nonzero(dense)
        ent = (row, col, dense[row, col])
    elif name.startswith("r"):
        m, n = (int(t) for t in name[1:].split("x"))
        ent = rect(m, n, 6, 7)
    elif name == "band4099":
        m, n = 4099, 4093
        ent = band(m, n, 7)
    elif name == "big":
        m, n = big_shape
        ent = rect(m, n, 1, 7)  # (two entries per row: this one is about the vector kernels' sweeps, and its reference takes seconds)
    else:
        raise KeyError(name)
    rng = np.random.default_rng(seed)
    b, x0 = rng.uniform(-1, 1, m), rng.uniform(-1, 1, n)
    small = min(m, n) <= 3
    return (m, n), ent, b, x0, tuple(k for k in KS if k <= min(m, n) or not small)


def csr_arrays(m, row, col, val):
    """(row_ptr, col, val) int32 / int32 / float64 of an entry list grouped by row"""
    assert np.all(np.diff(row) >= 0)
    rp = np.searchsorted(row, np.arange(m + 1)).astype(np.int32)
    return rp, np.asarray(col, dtype=np.int32), np.asarray(val, dtype=np.float64)


def true_normal_residual(entries, shape, b, x, damp):
    """||A^T (b - A x) - damp^2 x|| / ||A^T b|| in extended precision from a float64 x"""
    kind = _hp_kind(max(shape))
    Op = Operator(entries, shape, kind)
    b, x = _conv(b, kind), _conv(x, kind)
    d2 = _conv(np.array([damp]), kind)[0] ** 2
    s = Op.rmv(b - Op.mv(x)) - d2 * x
    atb = Op.rmv(b)
    return float(_sqrt(_dot(s, s) / _dot(atb, atb), kind))


def run_to_tolerance(entries, shape, b, x0, damp, rel_tol, max_iter, dot_order="pairwise"):
    """the float64 twin run to spmv_cgls's stopping rule (gamma <= rel_tol^2 ||A^T b||^2, looked at every iteration): (x, iterations)"""
    Op = Operator(entries, shape, "f64")
    dot = lambda a, c: _dot(a, c, dot_order)
    b, x = _conv(b, "f64"), _conv(x0, "f64")
    d2 = float(damp) ** 2
    atb = Op.rmv(b)
    limit = rel_tol * rel_tol * dot(atb, atb)
    r = b - Op.mv(x)
    s = Op.rmv(r) - d2 * x
    p = s.copy()
    gamma = dot(s, s)
    k = 0
    while k < max_iter and gamma > limit:
        q = Op.mv(p)
        alpha = gamma / (dot(q, q) + d2 * dot(p, p))
        x = x + alpha * p
        r = r - alpha * q
        s = Op.rmv(r) - d2 * x
        gamma_new = dot(s, s)
        p = s + (gamma_new / gamma) * p
        gamma = gamma_new
        k += 1
    return x, k
