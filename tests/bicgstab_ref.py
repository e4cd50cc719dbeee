"""References for the nonsymmetric solver (spmv_bicgstab) - TEST INFRASTRUCTURE ONLY (no GPU needed).  The BiCGSTAB twin of
tests/cgls_ref.py, over its Operator.mv, with the arithmetic helpers, gate factor and floor of tests/solver_ref.py taken over
unchanged (_conv, _dot, _sqrt, _hp_kind, _xdev, F = 8, FLOOR = 2^-50).

run_bicgstab is right-preconditioned BiCGSTAB over an entry list (square, duplicates allowed) in one arithmetic - np.longdouble
for the reference (mpmath where solver_ref.available says so), float64 for the twins - written as csrc/solver_bicgstab.hip states it:

    r = b - A x;  rhat = r;  p = r;  rho = rhat.r
    loop:  phat = M^-1 p;  v = A phat;  alpha = rho / (rhat.v);  s = r - alpha v;  shat = M^-1 s;  t = A shat;
           omega = (t.s) / (t.t);  x += alpha phat + omega shat;  r = s - omega t;  rho' = rhat.r;
           beta = (rho' / rho) * (alpha / omega);  p = r + beta (p - omega v);  rho = rho'

M = I, or diag(A) (duplicates summed) for precond = "jacobi", or an operator of tests/precond_ops.py (FSAI, ILU(0), Chebyshev: the
preconditioners the engine applies by launches), which every run uses in its own arithmetic and every twin as its own variant.
The engine's special cases are here too: t.t = 0 gives omega = 0,
x += alpha phat, r = s (and beta = 0).  One is not: the engine lets an iteration that starts with r.r <= 1e-28 b.b pass quietly,
and the reference does not; so an iterate k is DROPPED from a problem's list when the reference's ||r_{k-1}|| / ||b|| is at or
below DROP_BELOW = 1e-13 - ten times the engine's floor of 1e-14, so that the engine's rounding does not decide on which side
it falls.  Envelope asserts that no problem with n > 3 loses more than MAX_DROPPED = 2 of its eight k: a cap, not a tolerance.

The float64 TWINS vary the order of the dot products (forward, reversed, pairwise) and the order in which a row's products are
added (stored, reversed): six of them.  Envelope.gate(k) = F * max(FLOOR, the largest deviation of a twin's x_k from the
extended-precision x_k); gate_resid(k) the same for ||r_k|| / ||b||, on cgls_ref.Envelope's scale.  Both are measured on this
file's arithmetic and never on the engine: an engine iterate beyond them is a finding to explain, not a reason to raise F.

Observed here (x86, np.longdouble; b then x0 from default_rng(seed).uniform(-1, 1); tests/test_bicgstab_ref.py prints them):
  ||r_12|| / ||b|| of the reference, plain:   r33 2.0e-13, r4097 2.4e-07, band4099 5.1e-10 - nothing dropped;
  Jacobi:  r33 1.3e-16 and r4097 8.7e-15 - both lose k = 13 and nothing else; band4099 (constant diagonal) as plain.
  Twin envelopes over every problem and k: x 1.1e-15 .. 3e-14, residual 9e-16 .. 6.4e-11.
  Leave-one-out (one twin against the envelope of the other five), worst over every problem, preconditioner and k: 1.97 for x
  and 3.64 for the residual from the random starts (both on band4099, plain), 4.07 for the residual from x0 = 0 (band4099,
  Jacobi) - F = 8 holds for this file's own arithmetic with about a factor of two to spare.  From x0 = 0, r33 loses k = 13
  plain as well (7.7e-15 at k = 12).
  Under the operators of tests/precond_ops.py (FSAI, ILU(0) in row order, Chebyshev with given bounds; precond_ops.BICGSTAB_CASES but
  big): ||r_12|| / ||b|| from the random starts lap33 5.2e-04 (FSAI level 2) and 5.5e-05 (Chebyshev, degree 4), convdiff45 1.5e-05
  (ILU(0)) - nothing dropped, from x0 = 0 either; n2 and n3 under ILU(0), an exact factorisation of a dense matrix, end at k = 1 and
  keep that k alone.  band4099 under ILU(0) would lose three of its eight k and is not among the cases.  Twin envelopes x 8.9e-16
  (the floor) .. 3.4e-12, residual 8.9e-16 .. 1.3e-11; leave-one-out 2.10 for x and 3.63 for the residual (both lap33, Chebyshev,
  random start).
"""
from __future__ import annotations

import numpy as np

import precond_ops
from cgls_ref import BAND_OFFSETS, ROW_ORDERS, Operator, band, csr_arrays, rect  # noqa: F401
from solver_ref import DOT_ORDERS, F, FLOOR, _conv, _dot, _hp_kind, _sqrt, _xdev, available  # noqa: F401

KS = (1, 2, 3, 4, 5, 8, 9, 13)
DROP_BELOW = 1e-13
MAX_DROPPED = 2
OBSERVED_LEAVE_ONE_OUT = {"x": 1.97, "residual": 4.07}  # the worst ratios seen here (asserted <= F in tests/test_bicgstab_ref.py)
OBSERVED_LEAVE_ONE_OUT_LAUNCHED = {"x": 2.10, "residual": 3.63}  # the same under the preconditioners applied by launches
MUTATIONS = ("beta", "omega", "stale_p", "tail", "left")
# those that only a preconditioner applied by launches makes possible (precond: an operator of tests/precond_ops.py)
LAUNCHED_MUTATIONS = ("stale_phat", "stale_shat", "x_unhat", "tail")


def inverse_diagonal(Op: Operator):
    """1 / a_ii in Op's arithmetic, duplicates of a diagonal entry summed"""
    n = Op.shape[0]
    rows = np.repeat(np.arange(n), np.diff(Op.f_ptr))
    on = rows == Op.f_col
    diag = _conv(np.zeros(n), Op.kind)
    for i, v in zip(rows[on], Op.f_val[on]):  # (one entry per row, now and then two: the order of two additions is no order)
        diag[i] = diag[i] + v
    assert np.all(diag != 0), "a zero or missing diagonal entry"
    return 1 / diag


def run_bicgstab(Op: Operator, b, x0, ks, precond=None, dot_order="pairwise", mutate=None):
    """({k: (x_k, sqrt(r_k.r_k / b.b))}, the residual history for every k up to max(ks)).  mutate (the mutation check): "beta" drops
    the alpha / omega factor; "omega" t.s / s.s; "stale_p" p = r + beta p; "tail" the last element of x never updated; "left" M^-1
    applied on the left (to the residual and both products) instead of to p and s.  precond may be an operator of
    tests/precond_ops.py (M^-1 applied by launches), used in Op's arithmetic and as this twin's variant; then also "stale_phat" and
    "stale_shat": from the second iteration on M^-1 is applied to the p (the s) of the iteration before; "x_unhat": x += alpha p +
    omega s"""
    kind = Op.kind
    dot = lambda a, c: _dot(a, c, dot_order)
    b, x = _conv(b, kind), _conv(x0, kind)
    ks = set(ks)
    launched = precond_ops.is_op(precond)
    assert launched or precond in (None, "jacobi")
    dinv = inverse_diagonal(Op) if precond == "jacobi" else None
    left = mutate == "left" and dinv is not None
    right = (lambda u: u * dinv) if dinv is not None and not left else (lambda u: u)
    if launched:
        right = precond_ops.bound(precond, kind, Op.row_order, dot_order)
    p_before = s_before = None
    mv = (lambda u: Op.mv(u) * dinv) if left else Op.mv
    bb = dot(b, b)
    r = b * dinv - mv(x) if left else b - mv(x)
    rhat, p = r.copy(), r.copy()
    rho = dot(rhat, r)
    out, hist = {}, []

    def record(k):
        res = float(_sqrt(dot(r, r) / bb, kind))
        hist.append(res)
        if k in ks:
            out[k] = (x.copy(), res)

    record(0)
    for k in range(max(ks) if ks else 0):
        phat = right(p_before if mutate == "stale_phat" and k else p)
        v = mv(phat)
        alpha = rho / dot(rhat, v)
        s = r - alpha * v
        shat = right(s_before if mutate == "stale_shat" and k else s)
        p_before, s_before = p, s
        t = mv(shat)
        tt = dot(t, t)
        landed = tt == 0  # s = 0: the half step is the whole step
        omega = tt * 0 if landed else dot(t, s) / (dot(s, s) if mutate == "omega" else tt)
        xn = x + alpha * (p if mutate == "x_unhat" else phat) + omega * (s if mutate == "x_unhat" else shat)
        if mutate == "tail":
            xn[-1] = x[-1]
        x = xn
        r = s - omega * t
        rho_new = dot(rhat, r)
        if landed:
            beta = tt * 0
        else:
            beta = rho_new / rho if mutate == "beta" else (rho_new / rho) * (alpha / omega)
        p = r + beta * (p if mutate == "stale_p" else p - omega * v)
        rho = rho_new
        record(k + 1)
    return out, hist


def kept(ks, resid_hist):
    """the k of ks that no quiet iteration of the engine can touch: ||r_{k-1}|| / ||b|| of the reference above DROP_BELOW for every
    iteration up to k"""
    out = []
    for k in ks:
        if any(resid_hist[j] <= DROP_BELOW for j in range(k)):
            break
        out.append(k)
    return tuple(out)


def bicgstab_reference(entries, n, b, x0, ks, precond=None, force_mp=False):
    """{k: (x_k in the reference's precision, sqrt(r_k.r_k / b.b))} after exactly k iterations"""
    return run_bicgstab(Operator(entries, (n, n), _hp_kind(n, force_mp)), b, x0, ks, precond)[0]


class Envelope:
    """the extended-precision iterates of one problem, and how far the float64 twins stray from them.  self.ks is what is left of
    the ks asked for after the drop rule; self.dropped the rest"""

    def __init__(self, entries, n, b, x0, ks, precond=None, force_mp=False, row_orders=ROW_ORDERS):
        kind = _hp_kind(n, force_mp)
        ref, self.resid_hist = run_bicgstab(Operator(entries, (n, n), kind), b, x0, ks, precond)
        self.ks = kept(ks, self.resid_hist)
        self.dropped = tuple(k for k in ks if k not in self.ks)
        assert n <= 3 or len(self.dropped) <= MAX_DROPPED, f"{len(self.dropped)} of {len(ks)} iterates dropped at the noise floor (n = {n}, {precond})"
        self.ref_x = {k: ref[k][0] for k in self.ks}
        self.ref_resid = {k: ref[k][1] for k in self.ks}
        self.twin_dev = {k: {} for k in self.ks}  # k -> twin name -> (x deviation, residual deviation)
        for row_order in row_orders:
            Op = Operator(entries, (n, n), "f64", row_order)
            for order in DOT_ORDERS:
                out, _ = run_bicgstab(Op, b, x0, self.ks, precond, dot_order=order)
                for k in self.ks:
                    self.twin_dev[k][f"{row_order}/{order}"] = (self.x_dev(k, out[k][0]), self.resid_dev(k, out[k][1]))

    def x_dev(self, k, x):
        """max |x - ref_k| / max |ref_k|"""
        return _xdev(x, self.ref_x[k])

    def resid_dev(self, k, res):
        # solver_ref.Envelope.resid_dev's construction: the scale is the reference's value, or a quarter of the one before it
        return abs(res - self.ref_resid[k]) / max(self.ref_resid[k], self.resid_hist[k - 1] / 4 if k else 0.0, 1e-300)

    def envelope(self, k, what=0):
        return max(FLOOR, max(d[what] for d in self.twin_dev[k].values()))

    def gate(self, k):
        return F * self.envelope(k, 0)

    def gate_resid(self, k):
        return F * self.envelope(k, 1)

    def leave_one_out(self, k, what=0):
        """the largest deviation of one twin over the envelope (floored) of the other five"""
        devs = self.twin_dev[k]
        return max(d[what] / max(FLOOR, max(o[what] for m, o in devs.items() if m != name)) for name, d in devs.items())


# ---- the problems of tests/test_gpu_bicgstab.py (entry lists with dyadic values; shared with the CPU checks) ------------------------
PROBLEMS = ("n1", "n2", "n3", "r33", "r4097", "band4099", "big")
SEEDS = {"n1": 3003, "n2": 3004, "n3": 3005, "r33": 3001, "r4097": 3000, "band4099": 3002, "big": 3006}
DENSE = {1: [[3.0]], 2: [[3.0, -1.0], [0.5, 4.0]], 3: [[3.0, -1.0, 0.5], [0.25, 4.0, -1.0], [-0.5, 1.0, 5.0]]}


def problem(name, big_n=None):
    """(n, (row, col, val), b, x0, ks): the square nonsymmetric systems of the step-by-step tests with a random right-hand side and
    a random non-zero start.  n1..n3 end at iteration n, so only k <= n is asked of them.  ks is the list before the drop rule:
    Envelope.ks is what a test runs."""
    if name in ("n1", "n2", "n3"):
        n = int(name[1:])
        dense = np.array(DENSE[n])
        row, col = np.nonzero(dense)
        ent = (row, col, dense[row, col])
    elif name in ("r33", "r4097"):
        n = int(name[1:])
        ent = rect(n, n, 6, 7)
    elif name == "band4099":
        n = 4099
        ent = band(n, n, 7)  # the seven BAND_OFFSETS diagonals, the main one 4 + 2^-10
    elif name == "big":
        n = int(big_n)
        assert n % 2 == 1
        ent = rect(n, n, 1, 7)  # (two entries per row: this one is about the vector kernels' sweeps, and its reference takes seconds)
    else:
        raise KeyError(name)
    rng = np.random.default_rng(SEEDS[name])
    b, x0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    return n, ent, b, x0, tuple(k for k in KS if k <= n or n > 3)


def true_residual(entries, n, b, x):
    """||b - A x|| / ||b|| in extended precision from a float64 x"""
    kind = _hp_kind(n)
    Op = Operator(entries, (n, n), kind)
    b, x = _conv(b, kind), _conv(x, kind)
    r = b - Op.mv(x)
    return float(_sqrt(_dot(r, r) / _dot(b, b), kind))


def run_to_tolerance(entries, n, b, x0, precond, rel_tol, max_iter, dot_order="pairwise"):
    """the float64 twin run to spmv_bicgstab's stopping rule (r.r <= rel_tol^2 b.b, looked at every iteration): (x, iterations)"""
    Op = Operator(entries, (n, n), "f64")
    dot = lambda a, c: _dot(a, c, dot_order)
    b, x = _conv(b, "f64"), _conv(x0, "f64")
    dinv = inverse_diagonal(Op) if precond == "jacobi" else 1.0
    bb = dot(b, b)
    limit = rel_tol * rel_tol * bb
    r = b - Op.mv(x)
    rhat, p = r.copy(), r.copy()
    rho = rr = dot(r, r)
    k = 0
    while k < max_iter and rr > limit:
        phat = p * dinv
        v = Op.mv(phat)
        alpha = rho / dot(rhat, v)
        s = r - alpha * v
        shat = s * dinv
        t = Op.mv(shat)
        tt = dot(t, t)
        omega = 0.0 if tt == 0 else dot(t, s) / tt
        x = x + alpha * phat + omega * shat
        r = s - omega * t
        rho_new, rr = dot(rhat, r), dot(r, r)
        beta = 0.0 if tt == 0 else (rho_new / rho) * (alpha / omega)
        p = r + beta * (p - omega * v)
        rho = rho_new
        k += 1
    return x, k
