"""References for the solver step (spmv_cg) - TEST INFRASTRUCTURE ONLY (no GPU needed).

cg_reference is textbook (preconditioned) conjugate gradients over an entry list in extended precision (np.longdouble where its
eps is 2^-63 or better - x86's 80-bit format - else mpmath at 80 decimal digits for n <= MP_MAX_N): the iterate x_k and the
recurrence residual ||r_k|| / ||b|| after exactly k iterations from a given x0, for every k asked for.  At eps ~ 1e-19 its own
rounding is four decades below anything float64 can show over a dozen iterations.

The float64 TWINS are the same recurrences in numpy float64, in the two arrangements csrc/solver.hip runs - the textbook one
(three launches per iteration: q = A p; alpha, x, r; beta, p) and the Chronopoulos-Gear one (two launches: w = A u, delta = u.w;
then beta, alpha, p, s, x, r, u, gamma in one pass), written as that file's header comments state them - each with its dot
products summed forward, reversed and pairwise.  How far the twins stray from the extended-precision iterate at step k is what
separate float64 roundings of this recurrence on this problem do to x_k; Envelope.gate(k) is the largest such deviation (max-norm,
relative), floored at 2^-50, times F.  It is measured on this file's own arithmetic and never on the engine.  F = 8 because the
engine's dot products are one more rounding of the same sums (32 slotted partial sums, fma) and separate roundings of one
recurrence differ by small factors; a GPU iterate beyond 8 envelopes is a finding to explain, not a reason to raise F.

A wrong beta, a stale ring slot, an element of x left out: each moves x_k by 1e-1 .. 1e-4 at the first k it touches (the
mutation check in tests/test_solver_ref.py), ten decades above the gate.
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble
EXTENDED = bool(np.finfo(LD).eps <= 2.0**-63)  # 80-bit extended (or better): the reference's arithmetic
MP_MAX_N = 5000  # without it: mpmath, for systems up to this size (larger cases are skipped by the caller, see available())
F = 8.0
FLOOR = 2.0**-50
DOT_ORDERS = ("forward", "reversed", "pairwise")


def available(n: int, force_mp: bool = False):
    """None where cg_reference can serve n unknowns, else the reason it cannot (the caller skips with it)"""
    if (EXTENDED and not force_mp) or n <= MP_MAX_N:
        return None
    return f"np.longdouble has eps {np.finfo(LD).eps:.3g} > 2^-63 here and the mpmath fallback serves n <= {MP_MAX_N} only (n = {n})"


# ---- arithmetic: "f64", "ld" (np.longdouble) or "mp" (object arrays of mpmath.mpf) ----------------------------------------------
def _conv(a, kind):
    a = np.asarray(a)
    if kind == "f64":
        return a.astype(np.float64)
    if kind == "ld":
        return a.astype(LD)
    import mpmath

    mpmath.mp.dps = 80
    return np.array([mpmath.mpf(float(v)) for v in a.ravel()], dtype=object).reshape(a.shape)


def _zeros(n, kind):
    return _conv(np.zeros(n), kind)


def _sqrt(v, kind):
    if kind == "mp":
        import mpmath

        return mpmath.sqrt(v)
    return np.sqrt(v)


def _dot(a, b, order="pairwise"):
    t = a * b
    if t.dtype == object:
        return sum(t.tolist())
    if order == "forward":
        return np.cumsum(t)[-1]
    if order == "reversed":
        return np.cumsum(t[::-1])[-1]
    return np.sum(t)  # numpy's pairwise summation


class System:
    """A (entry list, duplicates summed) as CSR in one arithmetic, its diagonal, and the preconditioner M^-1"""

    def __init__(self, entries, n, kind, precond=None):
        row, col, val = (np.asarray(a) for a in entries)
        row, col = row.astype(np.int64), col.astype(np.int64)
        o = np.lexsort((col, row))
        row, col, val = row[o], col[o], _conv(val, "ld" if kind == "f64" else kind)[o]
        first = np.flatnonzero(np.r_[True, (row[1:] != row[:-1]) | (col[1:] != col[:-1])]) if len(row) else np.zeros(0, np.int64)
        self.n, self.kind = n, kind
        self.r, self.c = row[first], col[first]
        v = np.add.reduceat(val, first) if len(first) else val
        self.v = v.astype(np.float64) if kind == "f64" else v
        self.rp = np.searchsorted(self.r, np.arange(n + 1))
        if np.any(np.diff(self.rp) == 0):
            raise ValueError("a row without entries: not positive definite")
        on = self.r == self.c
        if on.sum() != n:
            raise ValueError("a row without a diagonal entry")
        self.diag = self.v[on]
        self.precond = precond
        if precond is None:
            self.apply_m = lambda r: r.copy()
        elif precond == "jacobi":
            dinv = 1 / self.diag
            self.apply_m = lambda r: r * dinv
        elif isinstance(precond, tuple) and precond[0] == "symgs":
            self._symgs_setup(np.asarray(precond[1], dtype=np.int64), precond[2] if len(precond) > 2 else None)
            self.apply_m = self._symgs
        else:
            raise ValueError(f"unknown preconditioner {precond!r}")

    def mv(self, x):
        return np.add.reduceat(self.v * x[self.c], self.rp[:-1])

    # one symmetric Gauss-Seidel step on A z = r from z = 0: forward through `order`, then backward
    def _symgs_setup(self, order, colour):
        n = self.n
        if not np.array_equal(np.sort(order), np.arange(n)):
            raise ValueError("symgs: the order is not a permutation of the rows")
        off = self.r != self.c
        self.off_r, self.off_c, self.off_v = self.r[off], self.c[off], self.v[off]
        self.off_rp = np.searchsorted(self.off_r, np.arange(n + 1))
        self.order, self.groups = order, None
        if colour is None:
            return
        # vectorised per colour class - valid only where the colouring is proper (no stored entry couples two rows of a class) and
        # the order runs through the classes one after the other
        colour = np.asarray(colour, dtype=np.int64)
        co = colour[order]
        if np.any(np.diff(co) < 0) or np.any(colour[self.off_r] == colour[self.off_c]):
            raise ValueError("symgs: not a proper colouring swept class by class: pass the order alone (sequential sweep)")
        cuts = np.flatnonzero(np.r_[True, co[1:] != co[:-1], True])
        self.groups = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            rows = order[a:b]
            lens = self.off_rp[rows + 1] - self.off_rp[rows]
            idx = np.repeat(self.off_rp[rows], lens) + (np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens))
            has = lens > 0
            starts = (np.cumsum(lens) - lens)[has]
            self.groups.append((rows, idx, has, starts))

    def _symgs(self, r):
        z = _zeros(self.n, self.kind)
        if self.groups is not None:
            for sweep in (self.groups, self.groups[::-1]):
                for rows, idx, has, starts in sweep:
                    s = _zeros(len(rows), self.kind)
                    if len(idx):
                        s[has] = np.add.reduceat(self.off_v[idx] * z[self.off_c[idx]], starts)
                    z[rows] = (r[rows] - s) / self.diag[rows]
            return z
        rp, c, v, d = self.off_rp, self.off_c, self.off_v, self.diag
        for seq in (self.order, self.order[::-1]):
            for i in seq:
                lo, hi = rp[i], rp[i + 1]
                s = (v[lo:hi] * z[c[lo:hi]]).sum() if hi > lo else 0
                z[i] = (r[i] - s) / d[i]
        return z


def _record(out, resid_hist, k, ks, x, r, bb, kind, dot_order):
    res = _sqrt(_dot(r, r, dot_order) / bb, kind)
    resid_hist.append(float(res))  # every k, asked for or not
    if k in ks:
        out[k] = (x.copy(), float(res))


def run_textbook(S: System, b, x0, ks, dot_order="pairwise", mutate=None):
    """x_k, ||r_k|| / ||b|| for k in ks; three-launch arrangement: q = A p; alpha = rz / p.q; x += alpha p; r -= alpha q;
    z = M^-1 r; beta = rz' / rz; p = z + beta p.  mutate (the mutation check): "restart" beta = 0 whenever (k + 1) % 4 == 0;
    "stale" beta's denominator from four iterations ago; "tail" the last element of x never updated"""
    kind = S.kind
    dot = lambda a, c: _dot(a, c, dot_order)
    b, x = _conv(b, kind), _conv(x0, kind)
    ks = set(ks)
    r = b - S.mv(x)
    z = S.apply_m(r)
    p = z.copy()
    rz, bb = dot(r, z), dot(b, b)
    out, scale, hist = {}, [], []
    _record(out, scale, 0, ks, x, r, bb, kind, dot_order)
    for k in range(max(ks)):
        q = S.mv(p)
        alpha = rz / dot(p, q)
        xn = x + alpha * p
        if mutate == "tail":
            xn[-1] = x[-1]
        x = xn
        r = r - alpha * q
        z = S.apply_m(r)
        rz_next = dot(r, z)
        hist.append(rz)
        beta = rz_next / rz
        if mutate == "restart" and (k + 1) % 4 == 0:
            beta = beta * 0
        if mutate == "stale" and k >= 4:
            beta = rz_next / hist[k - 4]
        p = z + beta * p
        rz = rz_next
        _record(out, scale, k + 1, ks, x, r, bb, kind, dot_order)
    return out, scale


def run_chronopoulos_gear(S: System, b, x0, ks, dot_order="pairwise"):
    """the two-launch arrangement of csrc/solver.hip: w = A u, delta = u.w;  beta = gamma / gamma_old (0 at k = 0);
    alpha = gamma / (delta - beta gamma / alpha_old);  p = u + beta p;  s = w + beta s;  x += alpha p;  r -= alpha s;  u = M^-1 r;
    gamma' = r.u"""
    kind = S.kind
    dot = lambda a, c: _dot(a, c, dot_order)
    b, x = _conv(b, kind), _conv(x0, kind)
    ks = set(ks)
    r = b - S.mv(x)
    u = S.apply_m(r)
    p, s = _zeros(S.n, kind), _zeros(S.n, kind)
    gamma, bb = dot(r, u), dot(b, b)
    gamma_old = alpha_old = None
    out, scale = {}, []
    _record(out, scale, 0, ks, x, r, bb, kind, dot_order)
    for k in range(max(ks)):
        w = S.mv(u)
        delta = dot(u, w)
        if gamma_old is None:
            alpha = gamma / delta
            p, s = u.copy(), w
        else:
            beta = gamma / gamma_old
            alpha = gamma / (delta - beta * gamma / alpha_old)
            p = u + beta * p
            s = w + beta * s
        x = x + alpha * p
        r = r - alpha * s
        u = S.apply_m(r)
        gamma_old, alpha_old = gamma, alpha
        gamma = dot(r, u)
        _record(out, scale, k + 1, ks, x, r, bb, kind, dot_order)
    return out, scale


def _hp_kind(n, force_mp=False):
    why = available(n, force_mp)
    if why:
        raise RuntimeError(why)
    return "ld" if EXTENDED and not force_mp else "mp"


def cg_reference(entries, b, x0, ks, precond=None, arrangement="textbook", force_mp=False):
    """{k: (x_k in the reference's precision, ||r_k|| / ||b|| of the recurrence residual)} of (preconditioned) conjugate gradients
    after exactly k iterations from x0.  precond: None | "jacobi" | ("symgs", order[, colour]) - one forward and one
    backward Gauss-Seidel sweep from z = 0 in that row order; sequential, or one vector operation per colour class where a colour
    array is given (it must be a proper colouring and the order must run class by class).  Duplicate entries are summed."""
    n = len(b)
    S = System(entries, n, _hp_kind(n, force_mp), precond)
    run = run_textbook if arrangement == "textbook" else run_chronopoulos_gear
    out, _ = run(S, b, x0, ks)
    return out


def _xdev(x, ref):
    """max-norm relative deviation of an iterate from the reference iterate (computed in the reference's precision)"""
    ref = np.asarray(ref)
    d = np.abs(np.asarray(x).astype(ref.dtype) - ref) if ref.dtype != object else np.abs(np.asarray(x, dtype=object) - ref)
    return float(d.max() / np.abs(ref).max())


class Envelope:
    """the extended-precision iterates of one problem, and how far the float64 twins stray from them"""

    def __init__(self, entries, b, x0, ks, precond=None, force_mp=False):
        n = len(b)
        self.ks = tuple(ks)
        kind = _hp_kind(n, force_mp)
        ref, self.resid_hist = run_textbook(System(entries, n, kind, precond), b, x0, ks)
        self.ref_x = {k: v[0] for k, v in ref.items()}
        self.ref_resid = {k: v[1] for k, v in ref.items()}
        S = System(entries, n, "f64", precond)
        self.twin_dev = {k: {} for k in ks}  # k -> twin name -> (x deviation, residual deviation)
        for name, run in (("textbook", run_textbook), ("chronopoulos-gear", run_chronopoulos_gear)):
            for order in DOT_ORDERS:
                out, _ = run(S, b, x0, ks, dot_order=order)
                for k in ks:
                    self.twin_dev[k][f"{name}/{order}"] = (self.x_dev(k, out[k][0]), self.resid_dev(k, out[k][1]))

    def x_dev(self, k, x):
        """max |x - ref_k| / max |ref_k|"""
        return _xdev(x, self.ref_x[k])

    def resid_dev(self, k, res):
        """|res - ref_k| / max(ref_k, ref_{k-1} / 4).  The update r_k = r_{k-1} - alpha q rounds on the scale of r_{k-1}: one
        rounding of it (2^-52 |r_{k-1}|) is 2^-50 of a quarter of it, so where an iteration takes the residual down by more than
        4x (n <= 3: to zero, or to what rounding leaves of it) the scale is the previous residual's and the floor of the gate is
        that one rounding."""
        return abs(res - self.ref_resid[k]) / max(self.ref_resid[k], self.resid_hist[k - 1] / 4 if k else 0.0, 1e-300)

    def envelope(self, k, what=0):
        return max(FLOOR, max(d[what] for d in self.twin_dev[k].values()))

    def gate(self, k):
        return F * self.envelope(k, 0)

    def gate_resid(self, k):
        return F * self.envelope(k, 1)


# ---- the problems of tests/test_gpu_solver_steps.py (entry lists; shared with the CPU checks) ------------------------------------
def laplacian_2d(m):
    """5-point Laplacian on an m x m grid: (n, row, col, val), rows and columns ascending"""
    n = m * m
    idx = np.arange(n).reshape(m, m)
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [np.full(n, 4.0)]
    for a, b in ((idx[:, :-1], idx[:, 1:]), (idx[:-1, :], idx[1:, :])):
        rows += [a.ravel(), b.ravel()]
        cols += [b.ravel(), a.ravel()]
        vals += [np.full(a.size, -1.0)] * 2
    r, c, v = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    o = np.lexsort((c, r))
    return n, r[o], c[o], v[o]


def dominant_symmetric(n, k, seed, margin=2.0**-6):
    """B + B^T (k random entries per row of B, dyadic values in (-1, 1)) with the diagonal sum |off| (1 + margin), stored TWICE
    (3/4 and 1/4 of it: both exact, so the summed duplicates are the same number in every precision) and every row's columns in
    random order: (n, row, col, val) grouped by row.  Strictly dominant by the margin alone: CG is still far from the noise floor
    after 13 iterations (asserted in tests/test_solver_ref.py)."""
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(n), k)
    c = rng.integers(0, n, n * k)
    v = rng.integers(-(2**20) + 1, 2**17, n * k) / 2.0**20
    keep = (r != c) & (v != 0)
    r, c, v = r[keep], c[keep], v[keep]
    rr, cc, vv = np.concatenate([r, c]), np.concatenate([c, r]), np.concatenate([v, v])
    dom = np.zeros(n)
    np.add.at(dom, rr, np.abs(vv))  # multiples of 2^-20 below 2^6: exact
    dom = dom * (1 + margin) + 2.0**-10  # exact: 27 + 7 bits
    rr = np.concatenate([rr, np.arange(n), np.arange(n)])
    cc = np.concatenate([cc, np.arange(n), np.arange(n)])
    vv = np.concatenate([vv, 0.75 * dom, 0.25 * dom])
    o = np.lexsort((rng.random(len(rr)), rr))  # by row; columns in random order within a row
    return n, rr[o], cc[o], vv[o]


def csr_arrays(n, row, col, val):
    """(row_ptr, col, val) int32 / int32 / float64 of an entry list grouped by row"""
    assert np.all(np.diff(row) >= 0)
    rp = np.searchsorted(row, np.arange(n + 1)).astype(np.int32)
    return rp, np.asarray(col, dtype=np.int32), np.asarray(val, dtype=np.float64)


KS = (1, 2, 3, 4, 5, 8, 9, 13)  # the iterates checked: around the ring's period of 4, and far enough for an error to grow
PROBLEMS = ("n1", "n2", "n3", "lap33", "rand4097", "lap725", "lap1025")


def problem(name):
    """(n, (row, col, val), b, x0, ks): the systems of the step-by-step tests, with a random right-hand side and a random nonzero
    start.  n1..n3 are solved exactly by iteration n, so only k <= n is asked of them; lap725 (n = 525,625) and lap1025
    (n = 1,050,625) are odd and beyond one sweep of the one-element and the two-element kernels' grids."""
    if name in ("n1", "n2", "n3"):
        n = int(name[1:])
        dense = (np.diag([3.0, 4.0, 5.0][:n]) - np.eye(n, k=1) - np.eye(n, k=-1)) if n > 1 else np.array([[3.0]])
        row, col = np.nonzero(dense)
        val = dense[row, col]
    elif name.startswith("lap"):
        n, row, col, val = laplacian_2d(int(name[3:]))
    elif name == "rand4097":
        n, row, col, val = dominant_symmetric(4097, 6, 7)
    else:
        raise KeyError(name)
    rng = np.random.default_rng(1000 + PROBLEMS.index(name))
    b, x0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    return n, (row, col, val), b, x0, tuple(k for k in KS if k <= n or n > 3)
