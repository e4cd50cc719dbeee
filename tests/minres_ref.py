"""References for the symmetric indefinite solver (spmv_minres) - TEST INFRASTRUCTURE ONLY (no GPU needed).  The MINRES twin of
tests/bicgstab_ref.py, over cgls_ref.Operator.mv, with the arithmetic helpers, gate factor and floor of tests/solver_ref.py taken
over unchanged (_conv, _dot, _sqrt, _hp_kind, _xdev, F = 8, FLOOR = 2^-50).

run_minres is Paige and Saunders' preconditioned MINRES for (A - shift I) x = b over an entry list (square, symmetric, duplicates
allowed) in one arithmetic - np.longdouble for the reference (mpmath where solver_ref.available says so), float64 for the twins -
written as csrc/solver_minres.hip states it:

    r1 = b - (A - shift I) x0;  y = M^-1 r1;  beta1 = sqrt(r1.y);  r2 = r1;  beta = beta1;  oldb = 0;  dbar = epsln = 0;
    phibar = beta1;  cs = -1;  sn = 0;  w = w2 = 0
    loop:  v = y / beta;  y = A v - shift v;  from the second iteration on  y -= (beta / oldb) r1;  alfa = v.y;
           y -= (alfa / beta) r2;  r1 = r2;  r2 = y;  y = M^-1 r2;  oldb = beta;  beta = sqrt(r2.y);  oldeps = epsln;
           delta = cs dbar + sn alfa;  gbar = sn dbar - cs alfa;  epsln = sn beta;  dbar = -cs beta;  gamma = sqrt(gbar^2 + beta^2);
           cs = gbar / gamma;  sn = beta / gamma;  phi = cs phibar;  phibar = sn phibar;  w1 = w2;  w2 = w;
           w = (v - oldeps w1 - delta w2) / gamma;  x += phi w

M = I, or diag(P) for precond = "jacobi", P the operator Pop (None: A itself; duplicates of a diagonal entry summed), or an operator
of tests/precond_ops.py (FSAI or Chebyshev of a positive definite P, as the engine applies them by launches), which every run uses in
its own arithmetic and every twin as its own variant.  The residual
reported is phibar / beta_b, beta_b = sqrt(b.M^-1 b): the M^-1 norm of r_k over that of b, the 2-norms without a preconditioner.
beta = 0 (the Krylov space is exhausted, the iterate exact) ends the run; the iterates behind it are the one that stands, phibar 0.

One special case of the engine is not here: it lets an iteration that starts with phibar <= 1e-14 beta_b pass quietly, and the
reference does not; so an iterate k is DROPPED from a problem's list when the reference's phibar_{k-1} / beta_b is at or below
DROP_BELOW = 1e-13 - ten times the engine's floor, so that the engine's rounding does not decide on which side it falls.  Envelope
asserts that no problem with n > 3 loses more than MAX_DROPPED = 2 of its eight k: a cap, not a tolerance.

The float64 TWINS vary the order of the dot products (forward, reversed, pairwise) and the order in which a row's products are
added (stored, reversed): six of them.  Envelope.gate(k) = F * max(FLOOR, the largest deviation of a twin's x_k from the
extended-precision x_k); gate_resid(k) the same for phibar_k / beta_b, on solver_ref.Envelope's scale.  Both are measured on this
file's arithmetic and never on the engine: an engine iterate beyond them is a finding to explain, not a reason to raise F.

Observed here (x86, np.longdouble; b then x0 from default_rng(seed).uniform(-1, 1); tests/test_minres_ref.py prints them):
  phibar_12 / beta_b of the reference from the random starts: r33 3.2e-01, r4097 4.3e-01, band4099 4.1e-01 (Jacobi, a constant
  diagonal, the same), saddle 3.7e-02 plain and 4.2e-02 with Jacobi of blockdiag(K, I), shifted 1.1e-01 with and without Jacobi of the
  Laplacian - nothing is dropped anywhere, from x0 = 0 either: these systems are far from done at k = 13.
  Twin envelopes over every problem and k: x 8.9e-16 (the floor) .. 8.4e-14, residual 8.9e-16 .. 9.8e-14.
  Leave-one-out (one twin against the envelope of the other five), worst over every problem, preconditioner, start and k: 2.17 for
  x and 2.18 for the residual (both r33, plain, random start) - F = 8 holds for this file's own arithmetic with a factor of more
  than three to spare.
  Under the operators of tests/precond_ops.py (FSAI and Chebyshev with given bounds of a separate positive definite P;
  precond_ops.SYM_CASES but big): phibar_12 / beta_b from the random starts shifted 1.1e-01 (both), saddle 2.0e-02 (FSAI) and 9.4e-03
  (Chebyshev) - nothing dropped, from x0 = 0 either.  Twin envelopes x 8.9e-16 .. 6.3e-14, residual 8.9e-16 .. 3.0e-14; leave-one-out
  1.63 for x (shifted, Chebyshev, x0 = 0) and 3.23 for the residual (saddle, FSAI, random start).
"""
from __future__ import annotations

import collections

import numpy as np

import precond_ops
from cgls_ref import ROW_ORDERS, Operator, csr_arrays  # noqa: F401
from solver_ref import DOT_ORDERS, F, FLOOR, _conv, _dot, _hp_kind, _sqrt, _xdev, available  # noqa: F401

KS = (1, 2, 3, 4, 5, 8, 9, 13)
DROP_BELOW = 1e-13
MAX_DROPPED = 2
OBSERVED_LEAVE_ONE_OUT = {"x": 2.17, "residual": 2.18}  # the worst ratios seen here (asserted <= F in tests/test_minres_ref.py)
OBSERVED_LEAVE_ONE_OUT_LAUNCHED = {"x": 1.63, "residual": 3.23}  # the same under the preconditioners applied by launches
MUTATIONS = ("r1_term", "stale_w1", "dbar_sign", "no_shift", "beta_rr", "tail")
# those that only a preconditioner applied by launches makes possible (precond: an operator of tests/precond_ops.py)
LAUNCHED_MUTATIONS = ("stale_y", "beta_b_bb", "alfa_r2", "beta_rr", "tail")


def inverse_diagonal(Op: Operator):
    """1 / p_ii in Op's arithmetic, duplicates of a diagonal entry summed; every one must be positive"""
    n = Op.shape[0]
    rows = np.repeat(np.arange(n), np.diff(Op.f_ptr))
    on = rows == Op.f_col
    diag = _conv(np.zeros(n), Op.kind)
    for i, v in zip(rows[on], Op.f_val[on]):  # (one entry per row, now and then two: the order of two additions is no order)
        diag[i] = diag[i] + v
    assert np.all(diag > 0), "a diagonal entry that is not positive: no Jacobi preconditioner for MINRES"
    return 1 / diag


def run_minres(Op: Operator, b, x0, ks, shift=0.0, precond=None, Pop: Operator | None = None, dot_order="pairwise", mutate=None):
    """({k: (x_k, phibar_k / beta_b)}, that ratio for every k up to max(ks)).  mutate (the mutation check): "r1_term" drops the
    (beta / oldb) r1 term; "stale_w1" w1 is not rotated (stays the w2 of the iteration before); "dbar_sign" dbar = +cs beta;
    "no_shift" the shift ignored; "beta_rr" beta = sqrt(r2.r2) under a preconditioner; "tail" the last element of x never updated.
    precond may be an operator of tests/precond_ops.py (M^-1 applied by launches; Pop is not read), used in Op's arithmetic and as
    this twin's variant; then also "stale_y": y = M^-1 of the r2 before; "beta_b_bb": beta_b = sqrt(b.b); "alfa_r2": alfa = v.r2"""
    kind = Op.kind
    dot = lambda a, c: _dot(a, c, dot_order)
    b, x = _conv(b, kind), _conv(x0, kind)
    sh = _conv(np.array([0.0 if mutate == "no_shift" else shift]), kind)[0]
    ks = set(ks)
    launched = precond_ops.is_op(precond)
    assert launched or precond in (None, "jacobi")
    dinv = inverse_diagonal(Pop if Pop is not None else Op) if precond == "jacobi" else None
    minv = (lambda u: u * dinv) if dinv is not None else (lambda u: u)
    if launched:
        minv = precond_ops.bound(precond, kind, Op.row_order, dot_order)
    beta_b = _sqrt(dot(b, b if mutate == "beta_b_bb" else minv(b)), kind)
    r2 = b - (Op.mv(x) - sh * x)
    r1 = r2
    y = minv(r2)
    beta = _sqrt(dot(r2, y), kind)
    oldb = dbar = epsln = sn = beta * 0
    cs, phibar = sn - 1, beta
    w = w2 = w1_stale = x * 0
    out, hist = {}, []

    def record(k):
        res = float(phibar / beta_b)
        hist.append(res)
        if k in ks:
            out[k] = (x.copy(), res)

    record(0)
    for k in range(max(ks) if ks else 0):
        if beta == 0:  # exhausted: the iterate is exact and stands
            record(k + 1)
            continue
        v = y / beta
        y = Op.mv(v) - sh * v
        if k > 0 and mutate != "r1_term":
            y = y - (beta / oldb) * r1
        alfa = dot(v, r2 if mutate == "alfa_r2" else y)
        y = y - (alfa / beta) * r2
        r1, r2 = r2, y
        y = minv(r1 if mutate == "stale_y" else r2)
        oldb = beta
        beta = _sqrt(dot(r2, r2 if mutate == "beta_rr" else y), kind)
        oldeps = epsln
        delta = cs * dbar + sn * alfa
        gbar = sn * dbar - cs * alfa
        epsln = sn * beta
        dbar = cs * beta if mutate == "dbar_sign" else -cs * beta
        gamma = _sqrt(gbar * gbar + beta * beta, kind)
        cs, sn = gbar / gamma, beta / gamma
        phi, phibar = cs * phibar, sn * phibar
        w1 = w1_stale if mutate == "stale_w1" else w2
        w1_stale = w2
        w2 = w
        w = (v - oldeps * w1 - delta * w2) / gamma
        xn = x + phi * w
        if mutate == "tail":
            xn[-1] = x[-1]
        x = xn
        record(k + 1)
    return out, hist


def kept(ks, resid_hist):
    """the k of ks that no quiet iteration of the engine can touch: phibar_{k-1} / beta_b of the reference above DROP_BELOW for every
    iteration up to k"""
    out = []
    for k in ks:
        if any(resid_hist[j] <= DROP_BELOW for j in range(k)):
            break
        out.append(k)
    return tuple(out)


class Envelope:
    """the extended-precision iterates of one problem, and how far the float64 twins stray from them.  self.ks is what is left of
    the ks asked for after the drop rule; self.dropped the rest"""

    def __init__(self, entries, n, b, x0, ks, shift=0.0, precond=None, p_entries=None, force_mp=False, row_orders=ROW_ORDERS):
        kind = _hp_kind(n, force_mp)
        pop = lambda k, order="stored": Operator(p_entries, (n, n), k, order) if p_entries is not None else None
        ref, self.resid_hist = run_minres(Operator(entries, (n, n), kind), b, x0, ks, shift, precond, pop(kind))
        self.ks = kept(ks, self.resid_hist)
        self.dropped = tuple(k for k in ks if k not in self.ks)
        assert n <= 3 or len(self.dropped) <= MAX_DROPPED, f"{len(self.dropped)} of {len(ks)} iterates dropped at the noise floor (n = {n}, {precond})"
        self.ref_x = {k: ref[k][0] for k in self.ks}
        self.ref_resid = {k: ref[k][1] for k in self.ks}
        self.twin_dev = {k: {} for k in self.ks}  # k -> twin name -> (x deviation, residual deviation)
        for row_order in row_orders:
            Op, Pop = Operator(entries, (n, n), "f64", row_order), pop("f64", row_order)
            for order in DOT_ORDERS:
                out, _ = run_minres(Op, b, x0, self.ks, shift, precond, Pop, dot_order=order)
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


# ---- the problems of tests/test_gpu_minres.py (entry lists with dyadic values; shared with the CPU checks) -------------------------
PROBLEMS = ("n1", "n2", "n3", "r33", "r4097", "band4099", "saddle", "shifted", "big")
SEEDS = {name: 4000 + i for i, name in enumerate(PROBLEMS)}
# 1 x 1 negative; the swap; 3 x 3 indefinite (eigenvalues of both signs)
DENSE = {1: [[-3.0]], 2: [[0.0, 1.0], [1.0, 0.0]], 3: [[1.0, 2.0, -0.5], [2.0, -3.0, 1.0], [-0.5, 1.0, 0.25]]}
SYM_OFFSETS = (-8, -3, -1, 0, 1, 3, 8)
SADDLE_K, SADDLE_B = 2049, 1024
SHIFTED_GRID = (65, 63)
Problem = collections.namedtuple("Problem", "n entries b x0 ks shift p_entries")


def _mirror(i, j, v, diag):
    """(row, col, val) of a symmetric matrix from its strictly upper entries (i < j) given once and its diagonal: every pair is
    stored twice with the same value, so the symmetry is exact"""
    n = len(diag)
    r, c, vv = np.concatenate([i, j, np.arange(n)]), np.concatenate([j, i, np.arange(n)]), np.concatenate([v, v, diag])
    return r, c, vv


def random_symmetric(n, k, seed):
    """k random pairs per row (dyadic values in (-1, 1), each pair stored at (i, j) and (j, i); duplicates allowed) and a diagonal
    of alternating sign, of magnitude sum |off| (1 + 2^-6) + 2^-10 (exact): strictly dominant, so the eigenvalues lie on both sides
    of 0 and away from it.  Grouped by row, columns in random order within a row"""
    rng = np.random.default_rng(seed)
    i, j = np.repeat(np.arange(n), k), rng.integers(0, n, n * k)
    v = rng.integers(-(2**20) + 1, 2**20, n * k) / 2.0**20
    keep = (i != j) & (v != 0)
    i, j, v = i[keep], j[keep], v[keep]
    dom = np.zeros(n)
    np.add.at(dom, i, np.abs(v))
    np.add.at(dom, j, np.abs(v))  # multiples of 2^-20 below 2^6: exact
    dom = (dom * (1 + 2.0**-6) + 2.0**-10) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    r, c, vv = _mirror(i, j, v, dom)
    o = np.lexsort((rng.random(len(r)), r))
    return r[o], c[o], vv[o]


def band_symmetric(n, seed):
    """the seven SYM_OFFSETS diagonals, the upper three random dyadic in (-1, 1) and mirrored, the main one 1/4: the six others sum
    to about 3 in a row, so the spectrum straddles 0.  (row, col, val) in (row, diagonal) order, no duplicates"""
    rng = np.random.default_rng(seed)
    up = {d: rng.integers(-(2**20) + 1, 2**20, n) / 2.0**20 for d in SYM_OFFSETS if d > 0}  # up[d][i] = a(i, i + d)
    i = np.repeat(np.arange(n), len(SYM_OFFSETS))
    off = np.tile(np.array(SYM_OFFSETS), n)
    j = i + off
    v = np.zeros(len(i))
    for d, vals in up.items():
        v[off == d] = vals
        v[off == -d] = np.roll(vals, d)  # a(i, i - d) = a(i - d, i) = up[d][i - d]
    v[off == 0] = 0.25
    keep = (j >= 0) & (j < n) & (v != 0)
    return i[keep], j[keep], v[keep]


def saddle():
    """[[K, B^T], [B, 0]]: K the 1-D Laplacian (2, -1) of SADDLE_K rows, B SADDLE_B rows of two entries (1 at column 2 i, -1/2 at
    2 i + 1: full row rank), and its preconditioner's matrix blockdiag(K, I).  Both grouped by row, columns ascending"""
    nk, nb = SADDLE_K, SADDLE_B
    n = nk + nb
    ki = np.arange(nk - 1)
    bi = np.arange(nb)
    i = np.concatenate([ki, 2 * bi, 2 * bi + 1])
    j = np.concatenate([ki + 1, nk + bi, nk + bi])
    v = np.concatenate([np.full(nk - 1, -1.0), np.full(nb, 1.0), np.full(nb, -0.5)])
    diag = np.concatenate([np.full(nk, 2.0), np.zeros(nb)])
    r, c, vv = _mirror(i, j, v, diag)
    keep = vv != 0  # (the zero block has no entries)
    r, c, vv = r[keep], c[keep], vv[keep]
    o = np.lexsort((c, r))
    pr, pc, pv = _mirror(ki, ki + 1, np.full(nk - 1, -1.0), np.concatenate([np.full(nk, 2.0), np.ones(nb)]))
    po = np.lexsort((pc, pr))
    return n, (r[o], c[o], vv[o]), (pr[po], pc[po], pv[po])


def laplacian_eigenvalues(grid):
    """the eigenvalues of the 5-point Laplacian (4, -1) on a grid[0] x grid[1] grid, ascending"""
    a, c = (4 * np.sin(np.arange(1, m + 1) * np.pi / (2 * (m + 1))) ** 2 for m in grid)
    return np.sort((a[:, None] + c[None, :]).ravel())


def shifted():
    """the 5-point Laplacian on the SHIFTED_GRID grid (4095 rows; it is its own preconditioner's matrix) and a shift in the widest gap
    among its 40 smallest eigenvalues, a multiple of 2^-20: about 20 eigenvalues of A - shift I are negative"""
    gx, gy = SHIFTED_GRID
    idx = np.arange(gx * gy).reshape(gx, gy)
    rows, cols = [idx.ravel()], [idx.ravel()]
    for a, c in ((idx[:, :-1], idx[:, 1:]), (idx[:-1, :], idx[1:, :])):
        rows += [a.ravel(), c.ravel()]
        cols += [c.ravel(), a.ravel()]
    r, c = np.concatenate(rows), np.concatenate(cols)
    v = np.where(r == c, 4.0, -1.0)
    o = np.lexsort((c, r))
    lam = laplacian_eigenvalues(SHIFTED_GRID)[:40]
    at = 10 + int(np.argmax(np.diff(lam[10:])))
    shift = np.round((lam[at] + lam[at + 1]) / 2 * 2.0**20) / 2.0**20
    assert lam[at] < shift < lam[at + 1]
    return gx * gy, (r[o], c[o], v[o]), float(shift)


def problem(name, big_n=None):
    """Problem(n, entries, b, x0, ks, shift, p_entries): the symmetric systems of the step-by-step tests with a random right-hand
    side and a random non-zero start.  n1..n3 end at iteration n, so only k <= n is asked of them.  ks is the list before the drop
    rule: Envelope.ks is what a test runs.  p_entries: the matrix the preconditioner is built from (None: the system's own)"""
    shift, pent = 0.0, None
    if name in ("n1", "n2", "n3"):
        n = int(name[1:])
        dense = np.array(DENSE[n])
        assert np.array_equal(dense, dense.T)
        row, col = np.nonzero(dense)
        ent = (row, col, dense[row, col])
    elif name in ("r33", "r4097"):
        n = int(name[1:])
        ent = random_symmetric(n, 3, 7)
    elif name == "band4099":
        n = 4099
        ent = band_symmetric(n, 7)
    elif name == "saddle":
        n, ent, pent = saddle()
    elif name == "shifted":
        n, ent, shift = shifted()
        pent = ent
    elif name == "big":
        n = int(big_n)
        assert n % 2 == 1
        ent = band_symmetric(n, 7)
    else:
        raise KeyError(name)
    rng = np.random.default_rng(SEEDS[name])
    b, x0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    return Problem(n, ent, b, x0, tuple(k for k in KS if k <= n or n > 3), shift, pent)


def true_residual(entries, n, b, x, shift=0.0):
    """||b - (A - shift I) x|| / ||b|| in extended precision from a float64 x"""
    kind = _hp_kind(n)
    Op = Operator(entries, (n, n), kind)
    b, x = _conv(b, kind), _conv(x, kind)
    r = b - (Op.mv(x) - _conv(np.array([shift]), kind)[0] * x)
    return float(_sqrt(_dot(r, r) / _dot(b, b), kind))


def run_to_tolerance(entries, n, b, x0, shift, rel_tol, max_iter, dot_order="pairwise"):
    """the float64 twin without a preconditioner run to spmv_minres's stopping rule (phibar <= rel_tol ||b||, looked at every
    iteration): (x, iterations)"""
    Op = Operator(entries, (n, n), "f64")
    dot = lambda a, c: _dot(a, c, dot_order)
    b, x = _conv(b, "f64"), _conv(x0, "f64")
    limit = rel_tol * np.sqrt(dot(b, b))
    r2 = b - (Op.mv(x) - shift * x)
    r1 = y = r2
    beta = phibar = np.sqrt(dot(r2, r2))
    oldb = dbar = epsln = sn = 0.0
    cs = -1.0
    w = w2 = np.zeros(n)
    k = 0
    while k < max_iter and phibar > limit and beta > 0:
        v = y / beta
        y = Op.mv(v) - shift * v
        if k > 0:
            y = y - (beta / oldb) * r1
        alfa = dot(v, y)
        y = y - (alfa / beta) * r2
        r1, r2 = r2, y
        oldb, beta = beta, np.sqrt(dot(y, y))
        oldeps, delta, gbar = epsln, cs * dbar + sn * alfa, sn * dbar - cs * alfa
        epsln, dbar = sn * beta, -cs * beta
        gamma = np.sqrt(gbar * gbar + beta * beta)
        cs, sn = gbar / gamma, beta / gamma
        phi, phibar = cs * phibar, sn * phibar
        w1, w2 = w2, w
        w = (v - oldeps * w1 - delta * w2) / gamma
        x = x + phi * w
        k += 1
    return x, k
