"""NumPy reference for the triangular solves with a caller's matrix (spmv_trsv_*; csrc/sptrsv.hip) - TEST INFRASTRUCTURE ONLY
(no GPU needed).

The definition the engine is held to (include/spmv_abi.h states the same).  T is the strictly lower (TRSV_LOWER) or strictly upper
(TRSV_UPPER) part of a square CSR matrix, selected by row and column index, plus the diagonal; entries of the other triangle are
ignored.  Duplicates of the diagonal entry are summed in stored order; every other stored entry - duplicates and stored zeros
included - is a term of its own, and the order inside a row is kept.  TRSV_UNIT: the diagonal is 1 and stored diagonal entries are
ignored.  TRSV_TRANSPOSE: the working copy is the transpose of the selected triangle, a row's entries in ascending column index,
duplicates in stored order (a stable sort of the selected entries by column).

  extract              the working copy (ptr, col, val, diag, has_diag) and whether it is lower triangular
  solve_longdouble     substitution in np.longdouble: what the engine is compared with
  solve_twin           float64 twins: a row's sum in the working copy's order from 0.0 (lanes = 1: the order contract of the k-column
                       solve), or the strided partial sums of 4 / 16 lanes met in wave.hpp's group_sum tree (the one right-hand-side solve)
  level_hist, schedule, launches   the levels of a working copy and what csrc/tri_levels.hpp's rule makes of them for T lanes per row
  assert_trsv_budget   the conditions under which a solve is exact in any order of any sum, checked in integer arithmetic
  random_system        the general inputs of tests/test_gpu_trsv.py
"""
from __future__ import annotations

import math

import numpy as np

import ilu0_ref as ir
from ilu0_ref import _fma

TRSV_LOWER, TRSV_UPPER, TRSV_UNIT, TRSV_TRANSPOSE = 0, 1, 2, 4
ALL_FLAGS = tuple(range(8))
SMALL_LEVEL, SOLVE_THREADS = ir.SMALL_LEVEL, 1024  # csrc/tri_levels.hpp: kSmallLevel, kSolveThreads

# tests/test_gpu_trsv.py, general inputs: the engine's norm-wise error against np.longdouble over the largest error of the three
# float64 twins on the same system (never below the unit roundoff 2^-53, under which one rounding of x itself hides).  The engine's
# sums are fma chains in the twins' orders; the twins round every product (no fma in the interpreter), so the two land on either
# side of a rounding now and then.  Largest ratio measured on an MI355X over all cases of that test: ENVELOPE_MEASURED; the test
# asserts ratio <= ENVELOPE_MEASURED * ENVELOPE_SLACK.
ENVELOPE_MEASURED = 1.070  # at n = 5000, 1 entry per row, lower transposed; 176 solves, most of them at or just below 1.000
ENVELOPE_SLACK = 1.5
UNIT_ROUNDOFF = 2.0**-53


def flag_name(flags):
    return ("upper" if flags & TRSV_UPPER else "lower") + ("_unit" if flags & TRSV_UNIT else "") + ("_transposed" if flags & TRSV_TRANSPOSE else "")


# ---- the working copy ---------------------------------------------------------------------------------------------------------------
def extract(n, rp, cc, cv, flags):
    """(ptr, col, val, diag, has_diag, lower): the working copy of the triangle `flags` selects - the transpose under TRSV_TRANSPOSE -
    the diagonal with its duplicates summed in stored order (0.0 where none is stored), which rows store one, and whether the copy
    is lower triangular (solved in ascending row order)"""
    rp, cc, cv = np.asarray(rp, np.int64), np.asarray(cc, np.int64), np.asarray(cv, np.float64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    diag, has = np.zeros(n), np.zeros(n, bool)
    on = np.flatnonzero(cc == rows)
    for e in on.tolist():  # (np.add.at adds in index order too; the loop says so)
        diag[rows[e]] += cv[e]
    has[rows[on]] = True
    sel = cc > rows if flags & TRSV_UPPER else cc < rows
    r, c, v = rows[sel], cc[sel], cv[sel]  # stored order
    if flags & TRSV_TRANSPOSE:
        o = np.argsort(c, kind="stable")  # by column; a column's entries in stored order: ascending row, duplicates as stored
        r, c, v = c[o], r[o], v[o]
    ptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int64)
    lower = bool(flags & TRSV_UPPER) == bool(flags & TRSV_TRANSPOSE)
    return ptr, c, v, diag, has, lower


def bad_diagonal_row(diag, has):
    """the smallest row whose diagonal is missing, zero or not finite (what a set-up without TRSV_UNIT names), or -1"""
    bad = np.flatnonzero(~has | (diag == 0.0) | ~np.isfinite(diag))
    return int(bad[0]) if len(bad) else -1


def multiply(n, ptr, col, val, diag, x, unit, dtype=np.float64):
    """b = (T + D) x (unit: T + I) with the working copy, x of shape (n,) or (n, k)"""
    x = np.asarray(x, dtype)
    rows = np.repeat(np.arange(n), np.diff(ptr))
    b = x.copy() if unit else (np.asarray(diag, dtype).reshape((n,) + (1,) * (x.ndim - 1)) * x)
    np.add.at(b, rows, np.asarray(val, dtype).reshape((-1,) + (1,) * (x.ndim - 1)) * x[col])
    return b


# ---- substitution ---------------------------------------------------------------------------------------------------------------------
def solve_longdouble(n, ptr, col, val, diag, lower, b, unit):
    """x = (T + D)^-1 b in np.longdouble, b of shape (n,) or (n, k)"""
    x = np.array(b, dtype=np.longdouble)
    v, d, p = np.asarray(val, np.longdouble), np.asarray(diag, np.longdouble), np.asarray(ptr).tolist()
    for i in (range(n) if lower else range(n - 1, -1, -1)):
        a, e = p[i], p[i + 1]
        if e > a:
            x[i] = x[i] - np.tensordot(v[a:e], x[col[a:e]], axes=(0, 0))
        if not unit:
            x[i] = x[i] / d[i]
    return x


def _tree(parts):
    """wave.hpp: group_sum - lanes i and i + 1, then i and i + 2, ... meet; lane 0 holds the sum"""
    step = 1
    while step < len(parts):
        for i in range(0, len(parts), 2 * step):
            parts[i] = parts[i] + parts[i + step]
        step *= 2
    return parts[0]


def solve_twin(n, ptr, col, val, diag, lower, b, unit, lanes=1):
    """float64 substitution for one right-hand side: lane l of `lanes` adds the row's entries l, l + lanes, ... left to right from
    0.0, the lanes meet in group_sum's tree; then x = b - acc, or (b - acc) / d"""
    x = np.array(b, dtype=np.float64).tolist()
    p, c, v, d = np.asarray(ptr).tolist(), np.asarray(col).tolist(), np.asarray(val).tolist(), np.asarray(diag).tolist()
    for i in (range(n) if lower else range(n - 1, -1, -1)):
        a, e = p[i], p[i + 1]
        parts = [0.0] * lanes
        for l in range(min(lanes, e - a)):
            acc = 0.0
            for j in range(a + l, e, lanes):
                acc = _fma(v[j], x[c[j]], acc)
            parts[l] = acc
        r = x[i] - _tree(parts)
        x[i] = r if unit else r / d[i]
    return np.asarray(x)


def rel_error(got, want):
    """norm-wise: max |got - want| / max |want|, in np.longdouble"""
    want = np.asarray(want, np.longdouble)
    scale = np.max(np.abs(want)) if want.size else 0.0
    return float(np.max(np.abs(np.asarray(got, np.longdouble) - want)) / scale) if scale > 0 else 0.0


# ---- levels and launches ------------------------------------------------------------------------------------------------------------
def level_hist(n, ptr, col, lower):
    """rows per level of a working copy: level(i) = 1 + the largest level among the rows that row i names (0 without any)"""
    p, c, lev = np.asarray(ptr).tolist(), np.asarray(col).tolist(), [0] * n
    for i in (range(n) if lower else range(n - 1, -1, -1)):
        a, e = p[i], p[i + 1]
        if e > a:
            lev[i] = 1 + max(lev[j] for j in c[a:e])
    return np.bincount(np.asarray(lev, np.int64), minlength=1) if n else np.zeros(0, np.int64)


def lanes_of(n, nnz):
    """csrc/tri_levels.hpp: lanes per row of the one right-hand-side solve from the entries per row"""
    avg = nnz / n if n else 0.0
    return next((w for bound, w in ir.LANE_STEPS if avg <= bound), 16)


def width_of(k):
    """csrc/sptrsv.hip: lanes per row of the k-column solve, the next power of two >= min(k, 16)"""
    t = 1
    while t < min(k, 16):
        t *= 2
    return t


def schedule(hist, lanes):
    """[(first level, levels)]: a level of more than SMALL_LEVEL lanes alone, runs of smaller levels together"""
    sched, lv = [], 0
    while lv < len(hist):
        end = lv
        while end < len(hist) and hist[end] * lanes <= SMALL_LEVEL:
            end += 1
        end = max(end, lv + 1)
        sched.append((lv, end - lv))
        lv = end
    return sched


def launches(hist, lanes):
    """(launches of one solve, those of them that run the one-level kernel: a segment of one level with more than SOLVE_THREADS lanes;
    every other segment is one workgroup stepping through its levels)"""
    sched = [(lv, k) for lv, k in schedule(hist, lanes) if sum(hist[lv:lv + k]) > 0]
    return len(sched), sum(1 for lv, k in sched if k == 1 and hist[lv] * lanes > SOLVE_THREADS)


# ---- exactness ------------------------------------------------------------------------------------------------------------------------
def _grid(a, g, what):
    s = np.ldexp(np.asarray(a, np.float64), g)
    if not (np.all(np.isfinite(s)) and np.array_equal(s, np.round(s)) and (s.size == 0 or np.max(np.abs(s)) < 2.0**62)):
        raise AssertionError(f"{what}: not on the grid 2^-{g}")
    return s.astype(np.int64)


def assert_trsv_budget(n, ptr, col, val, diag, x, unit, g=2, gx=0):
    """The conditions under which b = (T + D) x and the solve that returns x from it are exact in any order of any sum, checked in
    INTEGER arithmetic (as ilu0_ref.assert_exact_budget does): the entries of T and D are multiples of 2^-g, x (shape (n,) or (n, k))
    of 2^-gx, D is +- a power of two (unit: not looked at), and for every row |d_i x_i| + sum_j |t_ij x_j| stays below 2^53 on the grid
    2^-(g + gx).  Then every term and every partial sum of b_i and of the solve's acc_i is a float64 whatever came first, b_i - acc_i is
    d_i x_i exactly, and the division by a power of two is exact.  Returns (the largest of those magnitudes in bits, b as float64)."""
    it, ix = _grid(val, g, "an entry of T"), _grid(x, gx, "x")
    ix2 = ix.reshape(n, -1)
    if unit:
        idg = np.full(n, 1 << g, np.int64)
    else:
        idg = _grid(diag, g, "a diagonal entry")
        mag = np.abs(idg)
        assert np.all(mag > 0) and np.all(mag & (mag - 1) == 0), "a diagonal entry is not +- a power of two"
    assert np.abs(it).max(initial=0) < 2**31 and np.abs(ix2).max(initial=0) < 2**31 and np.abs(idg).max(initial=0) < 2**31, "int64 would overflow"
    rows = np.repeat(np.arange(n), np.diff(ptr))
    terms = it[:, None] * ix2[np.asarray(col, np.int64)]
    ib, mag = idg[:, None] * ix2, np.abs(idg[:, None] * ix2)
    np.add.at(ib, rows, terms)
    np.add.at(mag, rows, np.abs(terms))
    worst = max(1, int(mag.max(initial=0)))
    assert worst < 2**53, f"a sum needs {math.log2(worst):.1f} bits on the grid 2^-{g + gx} (budget 53)"
    b = np.ldexp(ib.astype(np.float64), -(g + gx)).reshape(np.shape(x))
    return math.log2(worst), b


# ---- general inputs -----------------------------------------------------------------------------------------------------------------
def random_system(n, per_row, seed):
    """(n, rp, cc, cv): `per_row` off-diagonal entries per row at random columns of BOTH triangles in random order (so: unsorted, with
    duplicates; one entry of every row is stored twice on purpose, a tenth are stored zeros), scaled so that neither a row's nor a
    column's sum of magnitudes passes 1/2 (a unit diagonal dominates, transposed too), and the diagonal entry +-(1 + the row's sum)
    split into two stored parts: |d_i| >= 1 + sum_j |t_ij| for either triangle, by rows and by columns"""
    rng = np.random.default_rng([seed, 5])
    k = per_row if n > 1 else 0
    rows = np.repeat(np.arange(n), k).reshape(n, k)
    cols = (rows + 1 + rng.integers(0, max(n - 1, 1), (n, k))) % max(n, 1)
    vals = rng.uniform(-1, 1, (n, k))
    vals[rng.random((n, k)) < 0.1] = 0.0
    if k > 1:
        cols[:, 1] = cols[:, 0]  # a duplicate in every row
    row_abs = np.abs(vals).sum(axis=1) if k else np.zeros(n)
    col_abs = np.zeros(n)
    np.add.at(col_abs, cols.ravel(), np.abs(vals).ravel())
    top = max(row_abs.max(initial=0.0), col_abs.max(initial=0.0))
    if top > 0.5:
        vals *= 0.5 / top
        row_abs *= 0.5 / top
    d = np.where(rng.random(n) < 0.5, -1.0, 1.0) * (1.0 + row_abs)
    cc = np.concatenate([cols, np.arange(n)[:, None], np.arange(n)[:, None]], axis=1)
    cv = np.concatenate([vals, (0.75 * d)[:, None], (0.25 * d)[:, None]], axis=1)
    perm = np.argsort(rng.uniform(size=cc.shape), axis=1)
    cc, cv = np.take_along_axis(cc, perm, 1), np.take_along_axis(cv, perm, 1)
    rp = (np.arange(n + 1) * (k + 2)).astype(np.int32)
    return n, rp, cc.ravel().astype(np.int32), cv.ravel()


def lower_bidiagonal_gaps(n, every=8):
    """(n, rp, cc, cv, x): the diagonal (+- 1/2, 1, 2) and the sub-diagonal (multiples of 1/4 in [-3/4, 3/4]), the sub-diagonal entry
    dropped on every `every`-th row: `every` levels of about n / every rows, 1 lane; x integers in [-8, 8]"""
    rng = np.random.default_rng([n, 6])
    i = np.arange(n)
    has_sub = (i % every) != 0
    d = np.where(rng.random(n) < 0.5, -1.0, 1.0) * np.ldexp(1.0, rng.integers(-1, 2, n))
    s = rng.integers(-3, 4, n) / 4.0
    cnt = 1 + has_sub.astype(np.int64)
    rp = np.concatenate([[0], np.cumsum(cnt)])
    cc, cv = np.empty(rp[-1], np.int32), np.empty(rp[-1])
    cc[rp[:-1]] = np.where(has_sub, i - 1, i)
    cv[rp[:-1]] = np.where(has_sub, s, d)
    cc[rp[1:][has_sub] - 1] = i[has_sub]
    cv[rp[1:][has_sub] - 1] = d[has_sub]
    return n, rp.astype(np.int32), cc, cv, rng.integers(-8, 9, n).astype(np.float64)
