"""NumPy twin of CSR with single-precision value storage (csrc/csr_f32_settings.hpp, convert_f32.hip, solver_refine.hip) - TEST
INFRASTRUCTURE ONLY (no GPU needed).

demote      what spmv_csr_to_f32 does to the values: np.float32 rounding (nearest, ties to even) and the three statistics - the
            values that changed, the nonzero values that became zero or subnormal, the largest relative change among the changed
            values that did not underflow - and the overflow rule (a value that is not finite, or rounds to +-inf: ValueError with
            the count and the first entry).
pack        the entry word: the column in the low 32 bits, the float's IEEE bits in the high 32.
product     y0 + A x of the WIDENED values in np.longdouble, and (|A||x|, entries per row) for the rounding gate.
cg, refine  the loop of spmv_refine over a textbook conjugate-gradient iteration: the yardstick for its counts, never its engine.
"""
from __future__ import annotations

import numpy as np

FLT_MIN = float(np.finfo(np.float32).tiny)  # the smallest normal float


def demote(val):
    """(float32 values, inexact, underflow, max_rel_err); raises ValueError where a value cannot be stored"""
    v = np.asarray(val, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        f = v.astype(np.float32)
    w = f.astype(np.float64)
    bad = ~np.isfinite(v) | ~np.isfinite(w)
    if bad.any():
        raise ValueError(f"{int(bad.sum())} values are not finite or round to +-inf (the first is entry {int(np.flatnonzero(bad)[0])})")
    changed = w != v
    under = (v != 0.0) & (np.abs(w) < FLT_MIN)
    rest = changed & ~under
    rel = float(np.max(np.abs(w[rest] - v[rest]) / np.abs(v[rest]), initial=0.0))
    return f, int(changed.sum()), int(under.sum()), rel


def widen(f32) -> np.ndarray:
    return np.asarray(f32, dtype=np.float32).astype(np.float64)


def pack(col, f32) -> np.ndarray:
    """uint64 entry words"""
    c = np.asarray(col, dtype=np.int32).view(np.uint32).astype(np.uint64)
    b = np.ascontiguousarray(f32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return c | (b << np.uint64(32))


def unpack(words):
    """(int32 columns, float32 values) of uint64 entry words"""
    w = np.asarray(words, dtype=np.uint64)
    col = (w & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    val = (w >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return col, val


def product(row_ptr, col, f32, x, y0) -> np.ndarray:
    """y0 + A x in np.longdouble, A the widened values"""
    rp = np.asarray(row_ptr, dtype=np.int64)
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    y = np.asarray(y0, dtype=np.longdouble).copy()
    np.add.at(y, rows, widen(f32).astype(np.longdouble) * np.asarray(x, dtype=np.longdouble)[np.asarray(col, dtype=np.int64)])
    return y


def abs_product(row_ptr, col, f32, x):
    """((|A||x|)_i, entries of row i)"""
    rp = np.asarray(row_ptr, dtype=np.int64)
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    s = np.zeros(len(rp) - 1)
    np.add.at(s, rows, np.abs(widen(f32)) * np.abs(np.asarray(x, dtype=np.float64)[np.asarray(col, dtype=np.int64)]))
    return s, np.diff(rp)


def dense(nrow, ncol, row_ptr, col, val) -> np.ndarray:
    rp = np.asarray(row_ptr, dtype=np.int64)
    M = np.zeros((nrow, ncol))
    np.add.at(M, (np.repeat(np.arange(nrow), np.diff(rp)), np.asarray(col, dtype=np.int64)), np.asarray(val, dtype=np.float64))
    return M


def cg(A, b, x, rel_tol: float, max_iter: int):
    """conjugate gradients on the dense matrix A from x (changed in place), stopping on the recurrence residual as spmv_cg does:
    returns the iterations"""
    r = b - A @ x
    bb, rr = float(b @ b), float(r @ r)
    limit = rel_tol * rel_tol * bb
    if not bb > 0.0 or rr <= limit:
        return 0
    p = r.copy()
    k = 0
    while k < max_iter:
        q = A @ p
        alpha = rr / float(p @ q)
        x += alpha * p
        r -= alpha * q
        k += 1
        rr_new = float(r @ r)
        if rr_new <= limit:
            break
        p = r + (rr_new / rr) * p
        rr = rr_new
    return k


def refine(A, A_lo, b, x, inner_tol: float, rel_tol: float, max_outer: int, inner_max_iter: int):
    """spmv_refine's loop with the twin's cg as the inner solver, on dense matrices; x is changed in place.
    Returns (outer, inner_total, rel_resid)"""
    bb = float(b @ b)
    if not bb > 0.0:
        return 0, 0, 0.0
    outer = inner_total = 0
    best, xbest, k = 0.0, None, 0
    while True:
        r = b - A @ x
        res = float(np.sqrt(float(r @ r) / bb))
        if k > 0 and not res < best:
            x[:] = xbest
            return outer, inner_total, best
        best = res
        if res <= rel_tol or k >= max_outer:
            return outer, inner_total, res
        xbest = x.copy()
        d = np.zeros_like(x)
        inner_total += cg(A_lo, r, d, inner_tol, inner_max_iter)
        x += d
        outer += 1
        k += 1


def scaled_laplacian(m: int = 24, seed: int = 7):
    """(n, row_ptr, col, val) of D L D: L the 5-point Laplacian of an m x m grid, D = diag(uniform(0.5, 2)): symmetric positive
    definite, and every value takes a rounding to become a float"""
    n = m * m
    d = np.random.default_rng(seed).uniform(0.5, 2.0, size=n)
    rp, col, val = [0], [], []
    for i in range(m):
        for j in range(m):
            r = i * m + j
            for e in ((r - m, -1.0, i > 0), (r - 1, -1.0, j > 0), (r, 4.0, True), (r + 1, -1.0, j < m - 1), (r + m, -1.0, i < m - 1)):
                if e[2]:
                    col.append(e[0])
                    val.append(d[r] * e[1] * d[e[0]])
            rp.append(len(col))
    return n, np.array(rp, np.int32), np.array(col, np.int32), np.array(val)


# ---- block-diagonal copies past one trip of the set-up kernels' grid (tests/tiled.py) ------------------------------------------------
TILED_ROWS, TILED_NCOL = 128, 307
LANES = (1, 2, 4, 8, 16, 32, 64)


def tiled_structure():
    """(row_ptr, col) of a 128-row base: every row length of the 300-row matrix of tests/test_gpu_csr_f32.py once (0, 1, and for every
    lane count lpr + 1 and 4 lpr + 1, and 300), the other rows of 0, 1, 2, 3 and 5 entries - a mean near 10, so that the copies
    pass one trip in rows before they pass 5 M entries; columns distinct inside a row and in random order"""
    rng = np.random.default_rng(171)
    once = sorted({n for lpr in LANES for n in (0, 1, lpr + 1, 4 * lpr + 1)} | {300})
    short = (0, 1, 2, 3, 5)
    counts = [once[i // 8] if i % 8 == 3 and i // 8 < len(once) else short[i % 5] for i in range(TILED_ROWS)]
    assert set(once) <= set(counts)
    col = np.concatenate([rng.permutation(TILED_NCOL)[:n] for n in counts]).astype(np.int32)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), col


def tiled_rounded():
    """(row_ptr, col, val): values that essentially all take a rounding, three of them underflowing (to zero, to a subnormal, a
    subnormal float as it is)"""
    rp, col = tiled_structure()
    rng = np.random.default_rng(172)
    val = rng.standard_normal(len(col)) * np.ldexp(1.0, rng.integers(-30, 31, size=len(col)))
    val[[5, len(val) // 2, len(val) - 2]] = [1e-46, -1e-40, 2.0**-149]
    return rp, col, val


def tiled_copies(row_ptr, trip):
    """(k, conditions): the least number of copies with which the kernels over the entries (f32_pack, f32_widen, the packed-range
    check) and over the rows (csr_f32_row_max) take a later trip (one trip: `trip` items)"""
    nrow0, nnz0 = len(row_ptr) - 1, int(row_ptr[-1])
    k = max(trip // nnz0 + 1, trip // nrow0 + 1)
    return k, {"nnz > one trip": k * nnz0 > trip, "nrow > one trip": k * nrow0 > trip}


# a value with a larger relative change than rounding a random value gives: just below the tie between 1 and 1 + 2^-23, it rounds to 1
WORST_VALUE = 1.0 + 2.0**-24 - 2.0**-40
WORST_REL = (WORST_VALUE - 1.0) / WORST_VALUE
