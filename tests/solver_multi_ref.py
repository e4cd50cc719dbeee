"""References for the k-column solver step (spmv_cg_multi) - TEST INFRASTRUCTURE ONLY (no GPU needed).

run_multi is the float64 numpy twin of the loop csrc/solver_multi.hip runs: k independent Chronopoulos-Gear recurrences over one
solver_ref.System, with the loop's own rules - the host looks at r.r every check_every iterations and after the last one, a column
with rr_c <= rel_tol^2 bb_c at a look is frozen (its iterate stays, iters[c] = that iteration), a column with b_c = 0 is frozen
before the first iteration with iters = 0 and rel_resid = 0, a column at or below 1e-28 bb_c passes quietly.  Unmutated and without
a freeze it IS solver_ref.run_chronopoulos_gear column by column, bit for bit (tests/test_solver_multi_ref.py asserts that), so the
GPU's columns are held to the yardstick of tests/solver_ref.py: one Envelope per distinct column, gate F = 8 twin envelopes.

The columns of a test (columns()): column 0 is solver_ref.problem's own b and x0, column 1 is drawn from a second seed, and column
c >= 2 is 2^(c // 2) times column c % 2 - a power of two scales every number of the recurrence exactly, so its reference is the
scaled reference of column c % 2 and two Envelopes per problem serve any k.

mutate (the mutation check): "alpha_next" column c uses column c + 1's alpha; "gamma_old_next" beta_c takes gamma_old of column
c + 1; "frozen_updated" column 0 goes on being updated after it was frozen; "tail" the last row of X is never updated.
"""
from __future__ import annotations

import numpy as np

import solver_ref as sr

MUTATIONS = ("alpha_next", "gamma_old_next", "frozen_updated", "tail")
# special_columns(): at rel_tol = 1e-10 lap33's residual falls by ~1.4x per iteration, so no look is a factor 2 from the limit on both
# sides; at this rel_tol and check_every = 5 both ordinary columns are (the twin: 2.1x), and another rounding of the same
# recurrence stops at the same look (tests/test_solver_multi_ref.py checks the margin)
MARGIN_REL_TOL = 2.9e-11


class Breakdown(ArithmeticError):
    def __init__(self, column, iteration):
        super().__init__(f"column {column}: no descent direction at iteration {iteration}")
        self.column = column


def columns(name, k):
    """(n, entries, B, X0, ks): B and X0 (n, k) float64, C-contiguous - the row-major blocks spmv_cg_multi takes"""
    n, ent, b, x0, ks = sr.problem(name)
    rng = np.random.default_rng(2000 + sr.PROBLEMS.index(name))
    b1, x1 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    B, X0 = np.empty((n, k)), np.empty((n, k))
    for c in range(k):
        scale = 2.0 ** (c // 2)
        B[:, c] = scale * (b, b1)[c % 2]
        X0[:, c] = scale * (x0, x1)[c % 2]
    return n, ent, B, X0, ks


_ENV = {}


def envelopes(name, precond=None):
    """(Envelope of column 0, Envelope of column 1) of a problem under one preconditioner, computed once per process"""
    key = (name, precond)
    if key not in _ENV:
        n, ent, B, X0, ks = columns(name, 2)
        _ENV[key] = tuple(sr.Envelope(ent, B[:, c].copy(), X0[:, c].copy(), ks, precond) for c in range(2))
    return _ENV[key]


def column_dev(env_pair, c, j, x_col, resid=None):
    """(x deviation, residual deviation or None) of column c's iterate j from its own reference: column c is 2^(c // 2) times
    column c % 2, so the iterate is scaled back (exactly) and the relative residual compares as it is"""
    env = env_pair[c % 2]
    dev = env.x_dev(j, np.asarray(x_col) / 2.0 ** (c // 2))
    return dev, (None if resid is None else env.resid_dev(j, resid))


def _mv(S, X):
    return np.stack([S.mv(X[:, c]) for c in range(X.shape[1])], axis=1)


def _apply_m(S, R):
    return np.stack([S.apply_m(R[:, c]) for c in range(R.shape[1])], axis=1)


def _dots(A, B, order):
    return np.array([sr._dot(A[:, c], B[:, c], order) for c in range(A.shape[1])], dtype=np.float64)


def run_multi(S: sr.System, B, X0, max_iter, rel_tol=0.0, check_every=1, dot_order="pairwise", mutate=None, keep=()):
    """(X, iters, rel_resid, kept): the k-column loop in float64.  kept[j] = a copy of X after iteration j for j in keep;
    rr_hist is returned as kept["rr"]: rr_hist[j][c] = r.r of column c after iteration j (j = 0: the start)"""
    assert S.kind == "f64"
    B, X = np.array(B, dtype=np.float64), np.array(X0, dtype=np.float64)
    n, k = B.shape
    R = B - _mv(S, X)
    U = _apply_m(S, R)
    P, Sv = np.zeros((n, k)), np.zeros((n, k))
    gamma, bb, rr = _dots(R, U, dot_order), _dots(B, B, dot_order), _dots(R, R, dot_order)
    if not (np.all(np.isfinite(bb)) and np.all(np.isfinite(rr))):
        raise Breakdown(int(np.flatnonzero(~(np.isfinite(bb) & np.isfinite(rr)))[0]), 0)
    gamma_old, alpha_old = np.zeros(k), np.zeros(k)
    limit, floor = rel_tol * rel_tol * bb, 1e-28 * bb
    with np.errstate(invalid="ignore", divide="ignore"):
        rel_resid = np.where(bb > 0, np.sqrt(rr / np.where(bb > 0, bb, 1.0)), 0.0)
    frozen = ~(bb > 0) | (rr <= limit)
    iters = np.zeros(k, dtype=np.int32)
    every = max(1, check_every)
    kept = {"rr": [rr.copy()]}
    if 0 in keep:
        kept[0] = X.copy()
    j = 0
    while j < max_iter and (not frozen.all() or (mutate == "frozen_updated" and bb[0] > 0)):
        W = _mv(S, U)
        delta = _dots(U, W, dot_order)
        live = ~frozen & (rr > floor)
        if mutate == "frozen_updated" and bb[0] > 0:
            live[0] = rr[0] > floor[0]
        g_old = np.roll(gamma_old, -1) if mutate == "gamma_old_next" else gamma_old
        with np.errstate(invalid="ignore", divide="ignore"):
            beta = np.where(g_old > 0, gamma / np.where(g_old > 0, g_old, 1.0), 0.0)
            denom = np.where(beta != 0, delta - beta * gamma / np.where(beta != 0, alpha_old, 1.0), delta)
            bad = live & (~(denom > 0) | ~(gamma > 0))
            if bad.any():
                if mutate is not None:
                    break  # a mutated recurrence may lose its descent direction: what it did until then is in `kept`
                raise Breakdown(int(np.flatnonzero(bad)[0]), j)
            alpha = gamma / np.where(live, denom, 1.0)
        a_used = np.roll(alpha, -1) if mutate == "alpha_next" else alpha
        for c in np.flatnonzero(live):
            if gamma_old[c] == 0.0 and beta[c] == 0.0:
                P[:, c], Sv[:, c] = U[:, c], W[:, c]  # the first iteration, as run_chronopoulos_gear writes it
            else:
                P[:, c] = U[:, c] + beta[c] * P[:, c]
                Sv[:, c] = W[:, c] + beta[c] * Sv[:, c]
            xn = X[:, c] + a_used[c] * P[:, c]
            if mutate == "tail":
                xn[-1] = X[-1, c]
            X[:, c] = xn
            R[:, c] = R[:, c] - a_used[c] * Sv[:, c]
            U[:, c] = S.apply_m(R[:, c])
            gamma_old[c], alpha_old[c] = gamma[c], alpha[c]
            gamma[c] = sr._dot(R[:, c], U[:, c], dot_order)
            rr[c] = sr._dot(R[:, c], R[:, c], dot_order)
        j += 1
        kept["rr"].append(rr.copy())
        if j in keep:
            kept[j] = X.copy()
        if j % every == 0 or j == max_iter:
            newly = ~frozen & (rr <= limit)
            iters[newly] = j
            rel_resid[newly] = np.sqrt(rr[newly] / bb[newly])
            frozen |= newly
    open_ = ~frozen
    iters[open_] = j
    rel_resid[open_] = np.sqrt(rr[open_] / bb[open_])
    return X, iters, rel_resid, kept


def special_columns():
    """(n, entries, B, X0, kinds, rel_tol) on lap33, k = 4: an ordinary column (solver_ref.problem's), a column with b = 0 and
    x0 = 0, a column that x0 already solves exactly (x0 dyadic and b = A x0 in integer arithmetic, tests/exact.py: every partial sum
    of A x0 is exact in any order, so r_0 is exactly 0 in float64 as well), and a second ordinary column"""
    import exact

    n, ent, B2, X2, _ = columns("lap33", 2)
    row, col, val = ent
    bits, e = exact.choose_bits(5)
    xs = exact.dyadic(np.random.default_rng(77), n, bits, e)
    bs = exact.exact_product(n, row, col, val, xs, e)
    B, X0 = np.zeros((n, 4)), np.zeros((n, 4))
    B[:, 0], X0[:, 0] = B2[:, 0], X2[:, 0]
    B[:, 2], X0[:, 2] = bs, xs
    B[:, 3], X0[:, 3] = B2[:, 1], X2[:, 1]
    return n, ent, B, X0, ("ordinary", "zero", "solved", "ordinary"), 1e-10


def stopping_margin(kept, bb, c, rel_tol, check_every, iters_c):
    """how far (as a factor on ||r||) the twin's column c was from the limit at the look that froze it, and at the look before:
    (limit / resid at the stopping look, resid at the look before / limit); both >= 2 means another rounding of the same recurrence
    stops at the same look"""
    rr = kept["rr"]
    limit = rel_tol * rel_tol * bb[c]
    every = max(1, check_every)
    before = iters_c - every if iters_c % every == 0 else (iters_c // every) * every
    under = np.sqrt(limit / rr[iters_c][c]) if rr[iters_c][c] > 0 else np.inf
    over = np.sqrt(rr[before][c] / limit) if before >= 0 else np.inf
    return float(under), float(over)


def freeze_columns():
    """(n, entries, B, X0) on lap33, k = 2: column 0 is an eigenvector of the 33 x 33 grid's Laplacian from x0 = 0 (one iteration
    solves it), column 1 is random"""
    n, ent, B2, X2, _ = columns("lap33", 2)
    m = 33
    s = np.sin(np.pi * np.arange(1, m + 1) / (m + 1))
    B, X0 = np.zeros((n, 2)), np.zeros((n, 2))
    B[:, 0] = np.outer(s, s).ravel()
    B[:, 1], X0[:, 1] = B2[:, 1], X2[:, 1]
    return n, ent, B, X0
