"""One statement about the clock for spmv_trsv_solve_multi (marker `gpu_perf`: not part of `-m gpu`; `-m "gpu or gpu_perf"` runs and
asserts it, as the project's wall-clock checks are): on the lower triangle of the 64^3 Laplacian in row order - 190 levels, every one
of them far below a full device, the solve launch-bound - one solve of k = 8 right-hand sides is faster than 8 solves of one, timed
interleaved in the same process.  No absolute number; tools/bench_trsv.py records the ratio (profiles/r24_bench_trsv.jsonl)."""
import time

import numpy as np
import pytest

import ilu0_ref as ir
import trsv_ref as tr
from conftest import perf_expect

pytestmark = pytest.mark.gpu_perf
K, REPS, ROUNDS = 8, 10, 3


def test_eight_columns_at_once_beat_eight_solves(ctx):
    n, rp, cc, cv = ir.laplacian_3d(64)
    A = ctx.csr(n, n, rp, cc, cv)
    del rp, cc, cv
    ctx.trsv_setup(A, tr.TRSV_LOWER)
    info = ctx.trsv_info(A, tr.TRSV_LOWER)
    assert info["levels"] == 190, info
    b, x = ctx.gen_vector(n, seed=5), ctx.vector(n)
    B, X = ctx.gen_vector(n * K, seed=6), ctx.vector(n * K)

    def window(op):
        ctx.sync()
        t = time.perf_counter()
        for _ in range(REPS):
            op()
        ctx.sync()
        return (time.perf_counter() - t) * 1e3 / REPS

    single = lambda: ctx.trsv_solve(A, b, x, tr.TRSV_LOWER)
    multi = lambda: ctx.trsv_solve_multi(A, B, X, K, tr.TRSV_LOWER)
    window(single), window(multi)  # warm-up
    t_single, t_multi = [], []
    for _ in range(ROUNDS):  # interleaved
        t_single.append(window(single))
        t_multi.append(window(multi))
    ms_single, ms_multi = float(np.median(t_single)), float(np.median(t_multi))
    print(f"64^3 Laplacian, lower triangle, {info['levels']} levels: one solve {ms_single:.4f} ms ({info['launches']} launches), k = {K} at once "
          f"{ms_multi:.4f} ms ({A.get_param('trsv_multi_launches')} launches), {K} single solves / one k = {K} solve = {K * ms_single / ms_multi:.2f}")
    assert ms_single > 0 and ms_multi > 0
    perf_expect(ms_multi < K * ms_single, f"one k = {K} solve takes {ms_multi:.4f} ms, {K} single solves {K * ms_single:.4f} ms")
