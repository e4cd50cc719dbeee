"""NumPy twins of the sampled dense-dense product (spmv_sddmm) - TEST INFRASTRUCTURE ONLY (no GPU needed).

    out[e] = alpha * sum_{c < k} U[row(e), c] * V[col(e), c] + beta * out0[e]        for every stored entry e of a CSR pattern

sddmm_longdouble: the same in np.longdouble, for rounded inputs, with the magnitude the error bound is taken from.
sddmm_exact:      int64 arithmetic for DYADIC inputs (tests/exact.py): U and V on the grid 2^-e, out0 on 2^-2e, alpha and beta signed
                  powers of two.  Every product, every partial sum in any order, both scalings and the final sum are then exact in
                  float64 as long as the whole stays below 2^53 on its grid, so a correct kernel returns exactly these bits.
"""
from __future__ import annotations

import numpy as np

import exact


def entry_rows(row_ptr) -> np.ndarray:
    rp = np.asarray(row_ptr, dtype=np.int64)
    return np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))


def _as2d(a) -> np.ndarray:
    a = np.asarray(a)
    return a.reshape(-1, 1) if a.ndim == 1 else a


def sddmm_longdouble(row_ptr, col, U, V, alpha=1.0, beta=0.0, out0=None):
    """(out, mag) in np.longdouble: mag[e] = |alpha| sum_c |U V| + |beta out0[e]|, the scale of the classical dot-product bound.
    beta == 0: out0 is not read"""
    rows, cols = entry_rows(row_ptr), np.asarray(col, dtype=np.int64)
    Ul, Vl = _as2d(U).astype(np.longdouble)[rows], _as2d(V).astype(np.longdouble)[cols]
    a, b = np.longdouble(alpha), np.longdouble(beta)
    out = a * (Ul * Vl).sum(axis=1)
    mag = abs(a) * np.abs(Ul * Vl).sum(axis=1)
    if beta != 0.0:
        o = np.asarray(out0, dtype=np.longdouble)
        out = out + b * o
        mag = mag + np.abs(b * o)
    return out, mag


def pow2_exponent(a: float) -> int:
    """p with |a| = 2^p (raises for anything else)"""
    m, p = np.frexp(abs(float(a)))
    if m != 0.5:
        raise ValueError(f"{a} is no signed power of two")
    return int(p) - 1


def sddmm_exact(row_ptr, col, U, V, e: int, alpha=1.0, beta=0.0, out0=None) -> np.ndarray:
    """the exact result as float64, from int64 arithmetic.  U, V dyadic on 2^-e, out0 on 2^-2e, alpha and beta +-2^p (beta may be 0).
    Raises where an entry's |alpha| sum |U V| + |beta out0| needs more than 53 bits on the common grid"""
    rows, cols = entry_rows(row_ptr), np.asarray(col, dtype=np.int64)
    iu, iv = exact.scaled(_as2d(U), e)[rows], exact.scaled(_as2d(V), e)[cols]
    pa = pow2_exponent(alpha)
    pb = pow2_exponent(beta) if beta != 0.0 else pa
    g = min(pa, pb, 0)  # the common grid is 2^(g - 2e): both scalings become integer factors 2^(pa - g), 2^(pb - g)
    fa = int(np.sign(alpha)) * 2 ** (pa - g)
    dot = (iu * iv).sum(axis=1)
    mag = float(abs(fa)) * np.abs(iu * iv).astype(np.float64).sum(axis=1)
    acc = fa * dot
    if beta != 0.0:
        io = exact.scaled(out0, 2 * e)
        fb = int(np.sign(beta)) * 2 ** (pb - g)
        acc = acc + fb * io
        mag = mag + float(abs(fb)) * np.abs(io).astype(np.float64)
    if mag.size and float(mag.max()) * (1 + 1e-9) >= exact.BUDGET:
        raise ValueError(f"sddmm_exact: an entry needs {np.log2(mag.max()):.1f} bits (budget 53): choose smaller bits / exponents")
    return np.ldexp(acc.astype(np.float64), g - 2 * e)


def dyadic_inputs(rng, nrow: int, ncol: int, nnz: int, k: int, shrink: int = 8):
    """(U, V, out0, e): dyadic U (nrow, k), V (ncol, k) and out0 (nnz) whose sddmm is exact for alpha, beta in +-{1/2, 1, 2} (on the
    common grid the factors are at most 4 and 2): bits and exponents from exact.choose_bits for `shrink` = 8 times k terms, which
    leaves room for 4 k products and out0's wider exponent range (2^(b + 4e + 1) <= 4 k 2^(2b + 4e)); sddmm_exact checks the budget"""
    b, e = exact.choose_bits(terms=shrink * k)
    U = exact.dyadic(rng, (nrow, k), b, e)
    V = exact.dyadic(rng, (ncol, k), b, e)
    out0 = exact.dyadic(rng, nnz, b, 2 * e, e_lo=-2 * e)
    return U, V, out0, e


# ---- the patterns and constants the GPU tests share (tests/test_gpu_sddmm.py and its torch child) -------------------------------------
def settings() -> dict:
    """the integer constants of csrc/sddmm_settings.hpp by name (kSddmmRun, kSddmmMaxGrid, ...)"""
    import re
    from pathlib import Path

    text = (Path(__file__).resolve().parent.parent / "arm-spmv_amd" / "csrc" / "sddmm_settings.hpp").read_text()
    return {name: int(eval(expr, {"__builtins__": {}})) for name, expr in re.findall(r"constexpr int (kSddmm\w+)\s*=\s*([^;]+);", text)}


def trip_entries() -> int:
    """entries one trip of the full grid covers: a pattern with more sends wavefronts round a second time"""
    s = settings()
    return s["kSddmmMaxGrid"] * (s["kSddmmBlock"] // s["kSddmmWave"]) * s["kSddmmRun"]


def from_lengths(rng, lens, ncol):
    """(row_ptr, col) int32 with the given row lengths; a row's columns distinct and ascending"""
    lens = np.asarray(lens, dtype=np.int64)
    rp = np.zeros(len(lens) + 1, np.int32)
    rp[1:] = np.cumsum(lens)
    col = np.concatenate([np.sort(rng.choice(ncol, size=int(n), replace=False)) for n in lens] + [np.zeros(0, np.int64)])
    return rp, col.astype(np.int32)


def tridiagonal(n):
    i = np.arange(n, dtype=np.int64)
    col = np.stack([i - 1, i, i + 1], axis=1).ravel()
    col = col[(col >= 0) & (col < n)]
    lens = np.full(n, 3, np.int64)
    lens[0] = lens[-1] = 2 if n > 1 else 1
    rp = np.zeros(n + 1, np.int32)
    rp[1:] = np.cumsum(lens)
    return rp, col.astype(np.int32)


def patterns() -> dict:
    """name -> (nrow, ncol, row_ptr, col): the shapes at which the entry-parallel kernel can go wrong"""
    rng = np.random.default_rng(2024)
    run = settings()["kSddmmRun"]
    out = {}
    lens = rng.integers(0, 41, size=300)
    lens[0] = lens[-1] = 0
    out["rand300x257"] = (300, 257, *from_lengths(rng, lens, 257))
    out["one_row"] = (1, 5000, *from_lengths(rng, [5000], 5000))
    out["middle_row"] = (3, 5000, *from_lengths(rng, [0, 5000, 0], 5000))
    out["run_edges"] = (4, 2 * run + 1, *from_lengths(rng, [run - 1, run, run + 1, 2 * run + 1], 2 * run + 1))
    out["tridiagonal2000"] = (2000, 2000, *tridiagonal(2000))
    out["empty"] = (5, 7, np.zeros(6, np.int32), np.zeros(0, np.int32))
    return out


KS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64)
SCALINGS = ((1.0, 0.0), (-2.0, 0.5), (0.5, -1.0))
