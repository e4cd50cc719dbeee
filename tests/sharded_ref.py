"""CPU references for the sharded solver step - TEST INFRASTRUCTURE ONLY (no GPU needed).

What tests/child_sharded_ops.py and tests/child_sharded_ranks.py hold dist.HipShardOps to, in plain numpy / Python-int code that
owes nothing to the engine's kernels:
  * the per-rank row bounds (capi.partition_rows: host arithmetic, itself pinned to the oracle in test_dist_gloo.py);
  * the column-split twin: a shard's CSR arrays cut into `inside` [c0, c1) (columns rebased by c0) and `outside` (global
    columns), the order inside every row kept - the documented result of spmv_csr_split_columns;
  * dyadic inputs (tests/exact.py) sized so that not only one product but the whole of w . (A p), and A^T x summed over the
    ranks onto a dyadic y0, is exact in ANY order: fits_53 is the condition, tests/test_sharded_ref.py asserts it in Python
    integers for every case below, so no GPU case can pass by rounding.
"""
from __future__ import annotations

import numpy as np

import exact as ex

N_OPS = 1003  # 17 * 59: no multiple of any world size below; 8 ranks own 125 rows each, the last 128
OPS_CASES = ((N_OPS, 1), (N_OPS, 2), (N_OPS, 3), (N_OPS, 8), (5, 8))  # (n, world); n = 5: seven ranks own no rows, the last all five
E = 3  # exponents of every dyadic factor in [-E, E]
RAGGED_COLUMNS = ((0, 100), (100, 777), (777, N_OPS))  # explicit column bounds of the transposed exchange at world 3


def fits_53(bits: int, e: int, longest: int, length: int) -> bool:
    """Do all partial sums, in any order, fit 53 bits?  Every factor (value, direction, weight, y0) is +-m * 2^x with m < 2^bits
    and |x| <= e.  The widest sum the sharded step forms is the dot w . (A p): at most length * longest terms w_i a_ij p_j, each
    a multiple of 2^-3e below 2^(3 bits + 3e), i.e. below 2^(3 bits + 6e) on the integer grid; `length` more terms of that size
    cover a starting vector (y0, or the q the inside part left).  A^T x summed over the ranks (two factors, at most `longest`
    terms per column) is narrower.  longest: the longest row or column; length: the vector's length."""
    return (int(length) * int(longest) + int(length)) * 2 ** (3 * int(bits) + 6 * int(e)) < 2**53


def choose_bits(longest: int, length: int, e: int = E) -> int:
    """the widest mantissa that fits_53 allows at exponent range e (at least 3 bits, or the shape is too large for this scheme)"""
    for bits in range(ex.B_MAX, 2, -1):
        if fits_53(bits, e, longest, length):
            return bits
    raise ValueError(f"no exact inputs: longest row / column {longest}, length {length}, exponents +-{e}")


def row_bounds(nrow: int, world: int) -> list[tuple[int, int]]:
    """[begin, end) of every rank: the engine's host arithmetic (spmv_partition_rows)"""
    from __graft_entry__ import load_package

    capi = load_package().capi
    return [capi.partition_rows(nrow, world, r) for r in range(world)]


def shard_arrays(rp, cc, cv, lo: int, hi: int):
    """rows [lo, hi) of a CSR matrix the way the reference's NUMA driver cuts them: rebased int32 row_ptr, global columns"""
    rp = np.asarray(rp, dtype=np.int64)
    b, e = int(rp[lo]), int(rp[hi])
    return ((rp[lo:hi + 1] - b).astype(np.int32), np.ascontiguousarray(cc[b:e], dtype=np.int32), np.ascontiguousarray(cv[b:e], dtype=np.float64))


def split_columns(srp, scol, sval, c0: int, c1: int):
    """(inside, outside) of a shard's CSR arrays: entries with a column in [c0, c1), rebased by c0, and the rest with their global
    columns; each (row_ptr int32, col int32, val), the order inside every row kept"""
    rows = np.repeat(np.arange(len(srp) - 1), np.diff(srp))
    inside = (scol >= c0) & (scol < c1)

    def part(mask, rebase):
        rp = np.zeros(len(srp), np.int64)
        np.add.at(rp, rows[mask] + 1, 1)
        return (np.cumsum(rp).astype(np.int32), np.ascontiguousarray(scol[mask] - rebase, dtype=np.int32),
                np.ascontiguousarray(sval[mask]))

    return part(inside, c0), part(~inside, 0)


def ops_pattern(rng, n: int):
    """square, nonsymmetric: about 6 entries per row in random column order (duplicates allowed) anywhere in [0, n), a few empty
    rows, and one row fifty times longer than the rest next to the end (in the last shard at every world size)"""
    lens = rng.integers(4, 9, n)
    lens[rng.choice(max(n - 2, 1), size=max(1, n // 100), replace=False)] = 0
    lens[max(n - 2, 0)] = min(300, 8 * n)
    rp = np.zeros(n + 1, np.int64)
    rp[1:] = np.cumsum(lens)
    return rp, rng.integers(0, n, int(rp[-1])).astype(np.int32)


class OpsProblem:
    """one seeded matrix with its dyadic direction p, weights w, transposed input x, start y0 and a second pair (u, v) for the
    BLAS-1 checks, and the exact results of every local operation of every rank"""

    ALPHA, BETA = -1.5, 0.25  # axpby's coefficients: multiples of 2^-2

    def __init__(self, n: int, world: int):
        self.n, self.world, self.e = n, world, E
        rng = np.random.default_rng(77_000 + 16 * n + world)
        self.rp, self.cc = ops_pattern(rng, n)
        self.rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(self.rp))
        self.longest = max(ex.max_terms(self.rows, n), ex.max_terms(self.cc, n))
        self.bits = choose_bits(self.longest, n)
        self.cv = ex.dyadic(rng, len(self.cc), self.bits, E)
        self.p, self.w, self.x, self.y0, self.u, self.v = (ex.dyadic(rng, n, self.bits, E) for _ in range(6))
        self.bounds = row_bounds(n, world)

    def shard(self, rank: int):
        return shard_arrays(self.rp, self.cc, self.cv, *self.bounds[rank])

    def want_product(self, rank: int):
        """(q_own, w_own . q_own) of rank's rows, from integers"""
        lo, hi = self.bounds[rank]
        srp, scol, sval = self.shard(rank)
        q = ex.exact_product(hi - lo, *ex.csr_entries(srp, scol, sval), self.p, E)
        return q, ex.exact_dot(self.w[lo:hi], q, E, 2 * E)

    def want_transpose(self, rank: int) -> np.ndarray:
        """A_p^T x_p over all n columns, from integers"""
        lo, hi = self.bounds[rank]
        srp, scol, sval = self.shard(rank)
        return ex.exact_product(self.n, *ex.transposed(ex.csr_entries(srp, scol, sval)), self.x[lo:hi], E)

    def want_transpose_whole(self, y0=None) -> np.ndarray:
        """y0 + A^T x of the whole matrix, from integers"""
        return ex.exact_product(self.n, self.cc, self.rows, self.cv, self.x, E, y0=y0)

    def want_axpby(self, lo: int, hi: int) -> np.ndarray:
        """ALPHA u + BETA v on [lo, hi), from integers (on the grid 2^-(E + 2))"""
        acc = ex.scaled(self.u[lo:hi], E) * int(self.ALPHA * 4) + ex.scaled(self.v[lo:hi], E) * int(self.BETA * 4)
        return np.ldexp(acc.astype(np.float64), -(E + 2))

    def want_dot(self, lo: int, hi: int) -> float:
        return ex.exact_dot(self.u[lo:hi], self.v[lo:hi], E, E)
