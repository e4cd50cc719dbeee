"""Inputs whose sum is exact in any order - TEST INFRASTRUCTURE ONLY (no GPU needed).

Every value, x entry and y0 entry is DYADIC: +-m * 2^e with an integer m in [1, 2^B) and e in [-E, E].  Then every product a * x
is a multiple of 2^-2E, and as long as an output keeps (|y0| + reps * sum |a x|) * 2^2E below 2^53 every partial sum is exact as
well: in any order, with or without fma, through atomics, LDS partial sums, scans and split rows.  Every correct kernel returns
the same bits, and those bits come from integer arithmetic: scale to int64, sum, scale back (exact_product).  A dropped or
doubled term, a pad product that leaks into y, a term read from the wrong place: each changes the bits, however small it is
next to its row (the parity gate of oracle_lib allows 1e-10 x (|A||x|)_i; the smallest term here can sit 2^40 below the largest).

Poisoned x: every entry no stored entry reads is NaN or +-inf (poison); a kernel that multiplies an unread x entry, even by 0.0,
turns its output into NaN.
"""
from __future__ import annotations

import numpy as np

BUDGET = 2.0**53
E_MAX, B_MAX = 10, 10


def choose_bits(terms: int, reps: int = 1) -> tuple[int, int]:
    """(B, E) for outputs of at most `terms` products accumulated `reps` times onto a dyadic y0: the widest exponent range first
    (E <= E_MAX), then the widest mantissa, such that even the worst case stays within the 2^53 budget"""
    n = max(1, int(terms)) * max(1, int(reps))
    for e in range(E_MAX, -1, -1):
        for b in range(B_MAX, 0, -1):
            if n * 2.0 ** (2 * b + 4 * e) + 2.0 ** (b + 3 * e) < BUDGET:
                return b, e
    raise ValueError(f"no exact inputs for {terms} terms x {reps} calls per output")


def choose_bits_dot(total_terms: int, nout: int, reps: int = 1) -> tuple[int, int]:
    """(B, E) for a product whose dot w . y is exact as well: w, the values, x and y0 all dyadic with B bits and exponents in
    [-E, E], so every term w_i * a * x of the dot is a multiple of 2^-3E (three dyadic factors) of at most 2^(3B + 3E).  The whole
    of sum_i |w_i| (|y0_i| + reps * sum_j |a_ij x_j|) - `total_terms` products over `nout` outputs - stays below 2^53 on that grid,
    so every partial sum of the dot is exact in any order (lanes, wavefronts, the 32 slots, the host's sum over them), and every
    y_i is (|w_i| 2^E >= 1)."""
    t, n = max(1, int(total_terms)) * max(1, int(reps)), max(1, int(nout))
    for e in range(E_MAX, -1, -1):
        for b in range(B_MAX, 0, -1):
            if 2.0 ** (b + 2 * e) * (t * 2.0 ** (2 * b + 4 * e) + n * 2.0 ** (b + 3 * e)) < BUDGET:
                return b, e
    raise ValueError(f"no exact inputs for a dot over {total_terms} terms x {reps} calls in {nout} outputs")


def exact_dot(w, y, e_w: int, e_y: int) -> float:
    """w . y in int64 (w on the grid 2^-e_w, y on 2^-e_y), returned as float64.  Raises where sum |w_i y_i| reaches 2^53 on the
    grid 2^-(e_w + e_y): a float64 sum would stop being exact in some order (and below that bound int64 cannot overflow)."""
    iw, iy = scaled(w, e_w), scaled(y, e_y)
    if iw.shape != iy.shape:
        raise ValueError("exact_dot: shapes differ")
    mag = float(np.dot(np.abs(iw).astype(np.float64), np.abs(iy).astype(np.float64))) if iw.size else 0.0
    if mag * (1 + 1e-9) >= BUDGET:
        raise ValueError(f"exact_dot: the sum needs {np.log2(mag):.1f} bits (budget 53): choose smaller bits / exponents")
    return float(np.ldexp(float(np.sum(iw * iy)), -(e_w + e_y)))


def dyadic(rng, shape, bits: int, e: int, e_lo: int | None = None) -> np.ndarray:
    """float64 +-m * 2^x, m in [1, 2^bits), x in [e_lo, e] (e_lo = -e by default)"""
    lo = -e if e_lo is None else e_lo
    m = rng.integers(1, 2**bits, size=shape).astype(np.float64)
    s = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    return np.ldexp(s * m, rng.integers(lo, e + 1, size=shape))


def scaled(a: np.ndarray, e: int) -> np.ndarray:
    """the int64 twin a * 2^e of a dyadic array (raises where a * 2^e is not an integer, or not finite)"""
    a = np.asarray(a, dtype=np.float64)
    s = np.ldexp(a, e)
    if not np.all(np.isfinite(s)) or not np.array_equal(s, np.round(s)) or (s.size and np.max(np.abs(s)) >= BUDGET):
        raise ValueError(f"not a dyadic array on the grid 2^-{e}")
    return s.astype(np.int64)


def draw(rng, shape, bits: int, e: int):
    """(float64 values, their int64 twin scaled by 2^e)"""
    v = dyadic(rng, shape, bits, e)
    return v, scaled(v, e)


def exact_product(nout: int, out_idx, in_idx, val, x, e: int, y0=None, reps: int = 1) -> np.ndarray:
    """y0 + reps * (A x) over the entry list (out_idx[t], in_idx[t], val[t]) in int64, returned as float64.  Values and x entries
    are on the grid 2^-e, y0 on 2^-2e.  Raises where an output's |y0| + reps * sum |a x| reaches 2^53 (the sum would stop being
    exact in some order)."""
    out_idx = np.asarray(out_idx, dtype=np.int64)
    in_idx = np.asarray(in_idx, dtype=np.int64)
    iv = scaled(val, e)
    ix = scaled(np.asarray(x, dtype=np.float64)[in_idx], e) if len(in_idx) else np.zeros(0, np.int64)
    if len(iv) and float(np.max(np.abs(iv))) * float(np.max(np.abs(ix), initial=0)) >= BUDGET:
        raise ValueError("exact_product: a single product needs more than 53 bits: choose smaller bits / exponents")
    t = iv * ix
    acc = np.zeros(nout, np.int64) if y0 is None else scaled(y0, 2 * e)
    mag = np.abs(acc).astype(np.float64)
    if len(t):
        order = np.argsort(out_idx, kind="stable")
        o, ts = out_idx[order], t[order]
        starts = np.flatnonzero(np.r_[True, o[1:] != o[:-1]])
        rows = o[starts]
        mag_t = np.add.reduceat(np.abs(ts).astype(np.float64), starts)
        mag[rows] += reps * mag_t
        if np.any(mag * (1 + 1e-9) >= BUDGET):
            raise ValueError(f"exact_product: an output needs {np.log2(mag.max()):.1f} bits (budget 53): choose smaller bits / exponents")
        acc[rows] += reps * np.add.reduceat(ts, starts)
    elif np.any(mag >= BUDGET):
        raise ValueError("exact_product: y0 beyond the budget")
    return np.ldexp(acc.astype(np.float64), -2 * e)


def exact_multi(nout: int, out_idx, in_idx, val, X, e: int, Y0=None, reps: int = 1) -> np.ndarray:
    """exact_product for every column of X (nin, k): Y0 + reps * (A X), (nout, k); Y0 None: A X"""
    k = X.shape[1]
    Y = np.empty((nout, k))
    for c in range(k):
        Y[:, c] = exact_product(nout, out_idx, in_idx, val, np.ascontiguousarray(X[:, c]), e, y0=None if Y0 is None else Y0[:, c], reps=reps)
    return Y


# ---- entry lists (out index, in index, value) of the forward product y += A x ----------------------------------------------------
def csr_entries(row_ptr, col, val):
    rp = np.asarray(row_ptr, dtype=np.int64)
    return np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp)), np.asarray(col, dtype=np.int64), np.asarray(val)


def coo_entries(row, col, val):
    return np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64), np.asarray(val)


def csc_entries(col_ptr, row, val):
    cp = np.asarray(col_ptr, dtype=np.int64)
    return np.asarray(row, dtype=np.int64), np.repeat(np.arange(len(cp) - 1, dtype=np.int64), np.diff(cp)), np.asarray(val)


def ell_entries(nrow: int, k: int, col, val):
    """every slot (column-major: slot s of row i at i + s * nrow), padding included: its product 0.0 * x[pad column] is counted"""
    return np.tile(np.arange(nrow, dtype=np.int64), k), np.asarray(col, dtype=np.int64), np.asarray(val)


def dia_entries(nrow: int, ncol: int, offsets, val, col_bound: int = 0):
    """the in-bound terms of a row-major DIA handle: row i, diagonal d reads column j = i + off_d for 0 <= j < the forward column
    bound (col_bound where set, else min(nrow, ncol); never beyond ncol)"""
    offs = np.asarray(offsets, dtype=np.int64)
    nd = len(offs)
    jmax = min(col_bound if col_bound > 0 else min(nrow, ncol), ncol)
    i = np.repeat(np.arange(nrow, dtype=np.int64), nd)
    d = np.tile(np.arange(nd, dtype=np.int64), nrow)
    j = i + offs[d] if nd else i
    keep = (j >= 0) & (j < jmax)
    return i[keep], j[keep], np.asarray(val)[(i * nd + d)[keep]]


def transposed(entries):
    """the entry list of A^T from A's: out and in swapped"""
    out_idx, in_idx, val = entries
    return in_idx, out_idx, val


def max_terms(out_idx, nout: int) -> int:
    """the largest number of products one output takes"""
    return int(np.bincount(np.asarray(out_idx, dtype=np.int64), minlength=max(nout, 1)).max(initial=0))


def poison(x, used) -> np.ndarray:
    """a copy of x with every entry whose index is not in `used` set to NaN, +inf, -inf in turn"""
    x = np.array(x, dtype=np.float64)
    mask = np.ones(x.size, dtype=bool)
    u = np.asarray(used, dtype=np.int64)
    mask[u[(u >= 0) & (u < x.size)]] = False
    idx = np.flatnonzero(mask)
    x[idx] = np.array([np.nan, np.inf, -np.inf])[idx % 3]
    return x


def avoid_columns(col, ncol: int, panel_cols=()):
    """columns moved off 0, ncol - 1, every multiple of 16 and every panel base (multiples of panel_cols): where a kernel's pad
    reads land on one of these, they land on poison.  Needs ncol >= 34 (returns col unchanged below)."""
    c = np.array(col, dtype=np.int64)
    if ncol < 34:
        return c.astype(np.int32)

    def bad(v):
        b = (v % 16 == 0) | (v == ncol - 1)
        for p in panel_cols:
            b |= v % p == 0
        return b

    for _ in range(8):
        m = bad(c)
        if not m.any():
            break
        c[m] = np.where(c[m] + 1 < ncol - 1, c[m] + 1, c[m] - 3)
    assert not bad(c).any()
    return c.astype(np.int32)
