"""One statement about the clock for spmv_minres (`pytest -m gpu` records it, `-m "gpu or gpu_perf"` asserts it, as the project's
wall-clock checks are): one MINRES iteration on the 2048^2 Laplacian is no slower than one mid-cycle iteration of spmv_gmres(30) of the
same build, timed interleaved in the same test.  MINRES moves 15 doubles per row beside its product, a GMRES iteration in the middle
of its cycle about a hundred (csrc/solver_gmres.hip); a loss would be a finding about the kernels of csrc/solver_minres.hip.

The method is tools/bench_gmres.py's: an iteration's time is the difference of a solve of ITERS_LONG and one of ITERS_SHORT iterations
over the difference of the counts (rel_tol = 0, one look of the host at the end, x = 0 set before every solve and outside the window);
for GMRES both counts lie inside one cycle, so the iterations between them are its columns 10 .. 25.
"""
import time

import numpy as np
import pytest

from conftest import perf_expect

pytestmark = pytest.mark.gpu
ITERS_SHORT, ITERS_LONG = 10, 26
ROUNDS = 3


def _laplacian_2d_csr(m):
    """(n, row_ptr, col, val) of the 5-point Laplacian on an m x m grid, columns ascending, without a sort"""
    n = m * m
    i = np.arange(n, dtype=np.int64)
    r, c = i // m, i % m
    cols = np.stack([i - m, i - 1, i, i + 1, i + m], axis=1)
    keep = np.stack([r > 0, c > 0, np.ones(n, bool), c < m - 1, r < m - 1], axis=1)
    vals = np.broadcast_to(np.array([-1.0, -1.0, 4.0, -1.0, -1.0]), (n, 5))
    row_ptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32)
    return n, row_ptr, cols[keep].astype(np.int32), np.ascontiguousarray(vals[keep])


def test_a_minres_iteration_is_no_slower_than_a_gmres_iteration(ctx):
    n, rp, cc, cv = _laplacian_2d_csr(2048)
    A = ctx.csr(n, n, rp, cc, cv)
    del rp, cc, cv
    b, x = ctx.gen_vector(n, seed=5), ctx.vector(n)

    def solve(run, iters):
        x.fill(0.0)
        ctx.sync()
        t = time.perf_counter()
        done, res = run(iters)
        ctx.sync()
        assert done == iters and np.isfinite(res), (done, res)
        return (time.perf_counter() - t) * 1e3

    minres = lambda iters: ctx.minres(A, b, x, shift=0.5, max_iter=iters, rel_tol=0.0, check_every=iters)  # (0.5: inside the spectrum (0, 8))
    gmres = lambda iters: ctx.gmres(A, b, x, restart=30, max_iter=iters, rel_tol=0.0, check_every=iters)
    for run in (minres, gmres):
        solve(run, ITERS_SHORT)  # warm-up
    t = {(name, it): [] for name in ("minres", "gmres") for it in (ITERS_SHORT, ITERS_LONG)}
    for _ in range(ROUNDS):  # interleaved
        for it in (ITERS_SHORT, ITERS_LONG):
            t["minres", it].append(solve(minres, it))
            t["gmres", it].append(solve(gmres, it))
    per = {name: (float(np.median(t[name, ITERS_LONG])) - float(np.median(t[name, ITERS_SHORT]))) / (ITERS_LONG - ITERS_SHORT) for name in ("minres", "gmres")}
    print(f"2048^2 Laplacian: one MINRES iteration {per['minres']:.4f} ms, one mid-cycle GMRES(30) iteration {per['gmres']:.4f} ms, "
          f"ratio {per['gmres'] / per['minres']:.2f}")
    assert per["minres"] > 0 and per["gmres"] > 0, per
    perf_expect(per["minres"] <= per["gmres"], f"one MINRES iteration takes {per['minres']:.4f} ms, one mid-cycle GMRES(30) iteration {per['gmres']:.4f} ms")
