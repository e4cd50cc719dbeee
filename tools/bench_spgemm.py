#!/usr/bin/env python3
"""spmv_spgemm measured: the LDS row kernels (SPMV_SPGEMM_ROWS) against the global expand-sort-compress (SPMV_SPGEMM_SORT), the
technique spmv_amg_setup builds P^T A P with and the in-engine baseline (the reference project has no sparse-sparse product).

One JSON line per input, printed as it is made, every figure from this one process.  The two methods are timed interleaved, one call
each per round, after a warm-up round; the figures are medians over --rounds rounds of the wall time of the whole synchronous call
(counting, both passes, the allocation of C and its analysis - without timing launches: SPMV_PANEL_TRIAL=0 is set for the run, so
the result's kernel is the model's pick under both methods).
  ms_rows, ms_sort, speedup (ms_sort / ms_rows), products, products per second of each, nnz_c, rows and products per path under
  ROWS, transient bytes of each, and ms as a multiple of one spmv_apply of A (spmv_apply_timed).

Inputs: lap2d_2048_squared, lap3d_160_squared, rmat16_squared (R-MAT scale 16, 8 edges a vertex, a = 0.57, b = c = 0.19, duplicate
edges removed), galerkin_lap2d_2048 (A P and P^T (A P) with level 0's aggregates of spmv_amg_setup; the transpose of P is made
outside the window and reported on its own).

  python tools/bench_spgemm.py [--inputs lap2d_2048_squared,...] [--rounds 3] [--out profiles/r16_bench_spgemm.jsonl]
Needs a GPU; there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

os.environ["SPMV_PANEL_TRIAL"] = "0"
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from bench_ilu0 import capi, stencil  # noqa: E402

INPUTS = ("lap2d_2048_squared", "lap3d_160_squared", "rmat16_squared", "galerkin_lap2d_2048")
REPS_APPLY = 20


def rmat(scale, edge_factor, seed=1, a=0.57, b=0.19, c=0.19):
    """(n, row_ptr, col, val): an R-MAT graph, duplicate edges removed, columns ascending, values uniform in (-1, 1)"""
    rng = np.random.default_rng(seed)
    n, edges = 1 << scale, edge_factor << scale
    row, col = np.zeros(edges, dtype=np.int64), np.zeros(edges, dtype=np.int64)
    for _ in range(scale):
        r = rng.random(edges)
        row = (row << 1) | (r >= a + b)
        col = (col << 1) | (((r >= a) & (r < a + b)) | (r >= a + b + c))
    key = np.unique(row * n + col)
    row, col = key // n, key % n
    rp = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=n))]).astype(np.int32)
    return n, rp, col.astype(np.int32), rng.uniform(-1, 1, len(col))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--inputs", default=",".join(INPUTS))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    ctx = capi.Context(0)
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def timed(call):
        ctx.sync()
        t = time.perf_counter()
        result = call()
        ctx.sync()
        return (time.perf_counter() - t) * 1e3, result

    for name in a.inputs.split(","):
        extra = {}
        if name == "rmat16_squared":
            n, rp, cc, cv = rmat(16, 8)
        else:
            n, rp, cc, cv = stencil(160, 3, False) if name.startswith("lap3d") else stencil(2048, 2, False)
        A = ctx.csr(n, n, rp, cc, cv)
        del rp, cc, cv
        if name.startswith("galerkin"):
            ctx.amg_setup(A)
            agg = ctx.amg_level(A, 0)[0]
            nc = int(ctx.amg_info(A)[1][1])
            P = ctx.csr(n, nc, np.arange(n + 1, dtype=np.int32), agg, np.ones(n))
            ms_t, Pt = timed(lambda: ctx.csr_transpose(P))
            extra = dict(aggregates=nc, ms_transpose_p=round(ms_t, 3))
            product = lambda method: ctx.spgemm(Pt, ctx.spgemm(A, P, method), method)
            parts = lambda method: (ctx.spgemm(A, P, method),)
        else:
            product = lambda method: ctx.spgemm(A, A, method)
            parts = lambda method: ()
        x, y = ctx.gen_vector(n, seed=5), ctx.vector(n)
        y.fill(0.0)
        ms = {capi.SPGEMM_ROWS: [], capi.SPGEMM_SORT: []}
        rec = dict(input=name, nrow=n, nnz_a=int(A.info.nnz), **extra)
        try:
            for rnd in range(a.rounds + 1):  # round 0 warms up
                for method in ms:
                    t, C = timed(lambda: product(method))
                    if rnd:
                        ms[method].append(t)
                    if rnd == a.rounds:  # what the last call did
                        tag = "rows" if method == capi.SPGEMM_ROWS else "sort"
                        stats = [C] + list(parts(method))
                        rec.update({f"transient_bytes_{tag}": sum(int(s.get_param("spgemm_transient_bytes")) for s in stats)})
                        if method == capi.SPGEMM_ROWS:
                            rec.update(products=sum(int(s.get_param("spgemm_products")) for s in stats), nnz_c=int(C.info.nnz),
                                       rows_lds=sum(int(s.get_param("spgemm_rows_lds")) for s in stats),
                                       rows_sorted=sum(int(s.get_param("spgemm_rows_sorted")) for s in stats),
                                       lds_products=int(C.get_param("spgemm_lds_products")))
                        del stats
                    del C
            ms_apply = ctx.apply_timed(A, x, y, REPS_APPLY)
            t_rows, t_sort = float(np.median(ms[capi.SPGEMM_ROWS])), float(np.median(ms[capi.SPGEMM_SORT]))
            rec.update(ms_rows=round(t_rows, 3), ms_sort=round(t_sort, 3), speedup=round(t_sort / t_rows, 3),
                       gproducts_per_s_rows=round(rec["products"] / t_rows / 1e6, 3), gproducts_per_s_sort=round(rec["products"] / t_sort / 1e6, 3),
                       ms_apply_a=round(ms_apply, 4), rows_in_applies=round(t_rows / ms_apply, 1), sort_in_applies=round(t_sort / ms_apply, 1))
        except capi.SpmvError as e:
            rec.update(error=str(e))
        emit(rec)
        del A, x, y
    if out:
        out.close()


if __name__ == "__main__":
    main()
