"""References for restarted GMRES (spmv_gmres) - TEST INFRASTRUCTURE ONLY (no GPU needed).  The GMRES twin of
tests/bicgstab_ref.py, over cgls_ref.Operator.mv, with the arithmetic helpers, gate factor and floor of tests/solver_ref.py
(_conv, _dot, _sqrt, _hp_kind, _xdev, F = 8, FLOOR = 2^-50) and the problems, drop rule (DROP_BELOW, kept) and cap (MAX_DROPPED = 2)
of tests/bicgstab_ref.py taken over unchanged.

run_gmres is right-preconditioned GMRES(m) with classical Gram-Schmidt run twice over an entry list (square, duplicates allowed)
in one arithmetic - np.longdouble for the reference (mpmath where solver_ref.available says so), float64 for the twins - written
as csrc/solver_gmres.hip states it:

    r = b - A x;  beta = ||r||;                                   (a cycle starts)   v_0 = r / beta;  g = (beta, 0, ...)
    for j = 0 .. m-1:
        z = M^-1 v_j;  w = A z;  h = 0
        twice:  c_i = v_i . w  for i = 0..j, all against the same w;   w -= sum_i c_i v_i (ascending i);   h_i += c_i
        h_{j+1} = ||w||;  v_{j+1} = w / h_{j+1}
        rotations 0..j-1 applied to h;  d = sqrt(h_j^2 + h_{j+1}^2);  (cs_j, sn_j) = (h_j, h_{j+1}) / d;  h_j = d
        g_{j+1} = -sn_j g_j;  g_j = cs_j g_j;      the recurrence's residual is |g_{j+1}|
    the cycle ends at j = m, at a stop, at max_iter or when it landed:
        y = R^-1 g (row i: t = g_i, t -= R_ik y_k for ascending k > i, y_i = t / R_ii);  x += M^-1 (sum_i y_i v_i), ascending i;
        and if the solve goes on, r = b - A x again

x_k is the GMRES iterate formed from the columns that stand after k iterations (what spmv_gmres leaves at max_iter = k,
rel_tol = 0), its residual |g_{j+1}| / ||b||.  M = I, or diag(A) (duplicates summed) for precond = "jacobi", or an operator of
tests/precond_ops.py (FSAI, ILU(0), Chebyshev as the engine applies them by launches: every arithmetic, every twin its own variant), or
any callable (the ILU(0) application of tests/ilu0_ref.py, float64 only).
v_{j+1} is formed when the next iteration asks for it, so the last
iteration of a 1 x 1 .. 3 x 3 system divides nothing by a norm that is rounding noise.  The engine lets an iteration that starts
with |g_j| <= 1e-14 ||b|| pass quietly and the reference does not: bicgstab_ref's drop rule takes such k off a problem's list.

The float64 TWINS vary the order of the dot products (forward, reversed, pairwise) and the order in which a row's products are
added (stored, reversed): six of them.  Envelope.gate(k) = F * max(FLOOR, the largest deviation of a twin's x_k from the
extended-precision x_k); gate_resid(k) the same for the residual.  Both are measured on this file's arithmetic and never on the
engine: an engine iterate beyond them is a finding to explain, not a reason to raise F.

Observed here (x86, np.longdouble): OBSERVED_LEAVE_ONE_OUT below; tests/test_gmres_ref.py prints every figure and records them in
its docstring.
"""
from __future__ import annotations

import numpy as np

import bicgstab_ref as br
import precond_ops
from bicgstab_ref import DROP_BELOW, MAX_DROPPED, PROBLEMS, inverse_diagonal, kept, true_residual  # noqa: F401
from cgls_ref import ROW_ORDERS, Operator, csr_arrays  # noqa: F401
from solver_ref import DOT_ORDERS, F, FLOOR, _conv, _dot, _hp_kind, _sqrt, _xdev, available  # noqa: F401

KS = br.KS  # (1, 2, 3, 4, 5, 8, 9, 13)
RESTARTS = (4, 30)  # m = 4 puts restarts inside 13 iterations, m = 30 puts none
# the wide basis: every tile edge of the dots kernel, a full basis, the restart behind it; and m = 1, a restart behind every iteration
WIDE_KS = {64: (16, 17, 33, 64, 65, 66), 8: (8, 9, 16, 17), 1: (1, 2, 3)}
MUTATIONS = ("rot", "g", "last_col", "keep_vm", "left", "no_minv", "tail")
# those that only a preconditioner applied by launches makes possible (precond: an operator of tests/precond_ops.py)
LAUNCHED_MUTATIONS = ("stale_z", "no_minv", "tail")
# the worst leave-one-out ratios seen here (asserted <= F in tests/test_gmres_ref.py, which prints them)
OBSERVED_LEAVE_ONE_OUT = {"x": 1.49, "residual": 2.60}
OBSERVED_LEAVE_ONE_OUT_LAUNCHED = {"x": 1.35, "residual": 3.83}  # the same under the preconditioners applied by launches


def _gmres(mv, minv, b, x0, kind, m, ks, dot_order="pairwise", mutate=None, rel_tol=None, max_iter=None):
    """the recurrence over callables.  ks: ({k: (x_k, |g| / ||b||)}, the residual history for every k up to max(ks)).  rel_tol: run
    to spmv_gmres's stopping rule instead, looked at every iteration (|g_{j+1}| <= rel_tol ||b||; at a restart the recomputed
    ||r||): (x, iterations)"""
    dot = lambda a, c: _dot(a, c, dot_order)
    sqrt = lambda v: _sqrt(v, kind)
    b, x = _conv(b, kind), _conv(x0, kind)
    ks = set(ks)
    to_tol = rel_tol is not None
    kmax = max_iter if to_tol else (max(ks) if ks else 0)
    bnorm = sqrt(dot(b, b))
    limit = rel_tol * bnorm if to_tol else None
    zero = bnorm * 0
    out, hist = {}, []
    r = b - mv(x)
    beta = sqrt(dot(r, r))
    hist.append(float(beta / bnorm))
    if 0 in ks:
        out[0] = (x.copy(), hist[0])
    k = 0
    if to_tol and (beta <= limit or kmax == 0):
        return x, 0
    pending = (r, beta)  # the next basis vector, before its division
    while k < kmax:
        V, R, cs, sn = [], [], [], []  # R: its columns
        g, g_plain = [beta], [beta]
        for j in range(m):
            V.append(pending[0] / pending[1])
            w = mv(minv(V[j - 1] if mutate == "stale_z" and j else V[j]))
            h = [zero] * (j + 2)
            for _ in range(2):
                c = [dot(V[i], w) for i in range(j + 1)]  # all against the same w
                for i in range(j + 1):
                    w = w - c[i] * V[i]
                    h[i] = h[i] + c[i]
            h[j + 1] = sqrt(dot(w, w))
            pending = (w, h[j + 1])
            if mutate != "rot":
                for i in range(j):
                    h[i], h[i + 1] = cs[i] * h[i] + sn[i] * h[i + 1], cs[i] * h[i + 1] - sn[i] * h[i]
            d = sqrt(h[j] * h[j] + h[j + 1] * h[j + 1])
            cs.append(h[j] / d)
            sn.append(h[j + 1] / d)
            R.append(h[:j] + [d])
            g.append(-sn[j] * g[j])
            g[j] = cs[j] * g[j]
            g_plain.append(zero)
            k += 1
            res = abs(g[j + 1])
            hist.append(float(res / bnorm))
            full = j + 1 == m
            stop = (to_tol and res <= limit) or k == kmax
            if k in ks or full or stop:
                nc = j + 1 - (1 if mutate == "last_col" and not full else 0)
                rhs = g_plain if mutate == "g" else g
                y = [zero] * nc
                for i in range(nc - 1, -1, -1):
                    t = rhs[i]
                    for q in range(i + 1, nc):
                        t = t - R[q][i] * y[q]
                    y[i] = t / R[i][i]
                xk = x
                if nc:
                    u = y[0] * V[0]
                    for i in range(1, nc):
                        u = u + y[i] * V[i]
                    xk = x + (u if mutate == "no_minv" else minv(u))
                    if mutate == "tail":
                        xk[-1] = x[-1]
                if k in ks:
                    out[k] = (xk.copy(), float(res / bnorm))
                if stop:
                    return (xk, k) if to_tol else (out, hist)
                if full:
                    x = xk
        # a restart
        if mutate == "keep_vm":
            beta = abs(g[m])  # v_0 = v_m and the rotated g's last entry instead of the recomputed residual
            continue
        r = b - mv(x)
        beta = sqrt(dot(r, r))
        pending = (r, beta)
        if to_tol and beta <= limit:
            return x, k
    return (x, k) if to_tol else (out, hist)


def _sides(Op, precond, mutate, dot_order="pairwise"):
    """(mv, M^-1, scale of b) of one Operator: precond None, "jacobi", an operator of tests/precond_ops.py (any arithmetic; the twin's
    variant from its row and dot order) or a callable (float64); the mutation "left" moves Jacobi to the other side"""
    if precond is None:
        return Op.mv, (lambda u: u), None
    if precond_ops.is_op(precond):
        return Op.mv, precond_ops.bound(precond, Op.kind, Op.row_order, dot_order), None
    if callable(precond):
        assert Op.kind == "f64"
        return Op.mv, precond, None
    assert precond == "jacobi"
    dinv = inverse_diagonal(Op)
    if mutate == "left":
        return (lambda u: Op.mv(u) * dinv), (lambda u: u), dinv
    return Op.mv, (lambda u: u * dinv), None


def run_gmres(Op: Operator, b, x0, ks, m, precond=None, dot_order="pairwise", mutate=None):
    """({k: (x_k, |g_{j+1}| / ||b||)}, the residual history for every k up to max(ks)).  mutate (the mutation check): "rot" the old
    rotations not applied to the new column; "g" y from the unrotated g = (beta, 0, ...); "last_col" the last column left out of
    x where the cycle is not full; "keep_vm" a restart that keeps v_m and |g_m| instead of recomputing r; "left" M^-1 on the left
    (of A and of b); "no_minv" x += V y without M^-1; "tail" the last element of x never updated; "stale_z" from a cycle's second column
    on M^-1 is applied to the basis vector before (z is not refreshed)"""
    mv, minv, scale = _sides(Op, precond, mutate, dot_order)
    bb = _conv(b, Op.kind)
    return _gmres(mv, minv, bb * scale if scale is not None else bb, x0, Op.kind, m, ks, dot_order, mutate)


def gmres_reference(entries, n, b, x0, ks, m, precond=None, force_mp=False):
    """{k: (x_k in the reference's precision, |g_{j+1}| / ||b||)} after exactly k iterations"""
    return run_gmres(Operator(entries, (n, n), _hp_kind(n, force_mp)), b, x0, ks, m, precond)[0]


def run_to_tolerance(entries, n, b, x0, m, precond, rel_tol, max_iter, dot_order="pairwise"):
    """the float64 twin run to spmv_gmres's stopping rule, looked at every iteration: (x, iterations).  precond: None, "jacobi" or
    a callable M^-1 (ilu0_ref.Ilu0.apply)"""
    Op = Operator(entries, (n, n), "f64")
    mv, minv, _ = _sides(Op, precond, None)
    return _gmres(mv, minv, b, x0, "f64", m, (), dot_order, rel_tol=rel_tol, max_iter=max_iter)


class Envelope(br.Envelope):
    """the extended-precision iterates of one problem under GMRES(m), and how far the float64 twins stray from them;
    bicgstab_ref.Envelope's construction, drop rule and measures over run_gmres.  self.ks is what is left of the ks asked for after
    the drop rule; self.dropped the rest"""

    def __init__(self, entries, n, b, x0, ks, m, precond=None, force_mp=False, row_orders=ROW_ORDERS):
        kind = _hp_kind(n, force_mp)
        self.m = m
        ref, self.resid_hist = run_gmres(Operator(entries, (n, n), kind), b, x0, ks, m, precond)
        self.ks = kept(ks, self.resid_hist)
        self.dropped = tuple(k for k in ks if k not in self.ks)
        assert n <= 3 or len(self.dropped) <= MAX_DROPPED, f"{len(self.dropped)} of {len(ks)} iterates dropped at the noise floor (n = {n}, m = {m}, {precond})"
        self.ref_x = {k: ref[k][0] for k in self.ks}
        self.ref_resid = {k: ref[k][1] for k in self.ks}
        self.twin_dev = {k: {} for k in self.ks}  # k -> twin name -> (x deviation, residual deviation)
        for row_order in row_orders:
            Op = Operator(entries, (n, n), "f64", row_order)
            for order in DOT_ORDERS:
                out, _ = run_gmres(Op, b, x0, self.ks, m, precond, dot_order=order)
                for k in self.ks:
                    self.twin_dev[k][f"{row_order}/{order}"] = (self.x_dev(k, out[k][0]), self.resid_dev(k, out[k][1]))


# ---- the problems of tests/test_gpu_gmres.py: bicgstab_ref's, and the wide basis -----------------------------------------------------
WIDE = "tri4099"


def problem(name, big_n=None):
    """(n, (row, col, val), b, x0, ks): bicgstab_ref.problem's systems; "tri4099" is the 4099-row tridiagonal matrix with -1.25
    below the diagonal, 2.25 + 2^-10 on it and -1 above, b then x0 from default_rng(3010).uniform(-1, 1) - far from converged after
    66 iterations, so that a basis of 64 vectors fills; its ks depend on m (WIDE_KS) and are () here"""
    if name != WIDE:
        return br.problem(name, big_n)
    n = 4099
    i = np.arange(n)
    row = np.concatenate([i[1:], i, i[:-1]])
    col = np.concatenate([i[:-1], i, i[1:]])
    val = np.concatenate([np.full(n - 1, -1.25), np.full(n, 2.25 + 2.0**-10), np.full(n - 1, -1.0)])
    o = np.lexsort((col, row))
    rng = np.random.default_rng(3010)
    b, x0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    return n, (row[o], col[o], val[o]), b, x0, ()
