#!/usr/bin/env python3
"""One CGLS iteration (spmv_cgls) against the two products it is built on: how far an iteration is above one spmv_apply plus one
spmv_apply_transpose of the same handle - that is, what its four vector kernels and six launches cost.

One JSON line per (shape, damp): the median over --rounds rounds of
  ms_iter        one iteration of spmv_cgls: the difference of a solve of ITERS_LONG and one of ITERS_SHORT iterations over the
                 difference of the counts (rel_tol = 0, one look of the host at the end, from x = 0, set again before every solve
                 and outside the timed window; a window is one whole call between two device synchronisations);
  ms_setup       what the short solve takes beyond its iterations: the work vectors, ||A^T b||^2, the first residual and gradient;
  ms_forward     spmv_apply_timed, ms_transpose  spmv_apply_transpose_timed (REPS products between two device events);
the three interleaved in the same process after a warm-up.  over_products = ms_iter / (ms_forward + ms_transpose).
bytes_vectors: what the four vector kernels of an iteration must move - q.q 8 nrow; the update 32 ncol + 24 nrow (x and p read, x
and s written; r and q read, r written); s.s 8 ncol; the direction 24 ncol (s and p read, p written) - on top of the products' own
reads of p and r and writes of q and s.

Shapes: c2_band (CSR 10M x 10M x 32, columns in a band of 65536), c2_uniform (the same, uniform columns), lap2d_2048 (the 5-point
Laplacian on 2048^2 points, 4.2M rows), rect_2to1 (CSR 8M x 4M x 16, uniform columns).

  python tools/bench_cgls.py [--shapes c2_band,c2_uniform,lap2d_2048,rect_2to1] [--out profiles/r10_bench_cgls.jsonl]
Needs a GPU; there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from __graft_entry__ import load_package  # noqa: E402

capi = load_package().capi
ITERS_SHORT, ITERS_LONG = 10, 50
REPS = 20


def laplacian_2d(m):
    """(n, row_ptr, col, val) of the 5-point Laplacian on an m x m grid, Dirichlet boundary, columns ascending"""
    n = m * m
    idx = np.arange(n, dtype=np.int64).reshape(m, m)
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [np.full(n, 4.0)]
    for lo, hi in ((idx[:, :-1], idx[:, 1:]), (idx[:-1, :], idx[1:, :])):
        rows += [lo.ravel(), hi.ravel()]
        cols += [hi.ravel(), lo.ravel()]
        vals += [np.full(lo.size, -1.0)] * 2
    r, c, v = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    o = np.argsort(r * n + c, kind="stable")
    r, c, v = r[o], c[o], v[o]
    return n, np.searchsorted(r, np.arange(n + 1)).astype(np.int32), c.astype(np.int32), v


def make(ctx, shape):
    if shape in ("c2_band", "c2_uniform"):
        n = 10_000_000
        return ctx.gen_csr_uniform(0, n, n, 32, 65536 if shape == "c2_band" else 0, seed=3)
    if shape == "lap2d_2048":
        n, rp, cc, cv = laplacian_2d(2048)
        return ctx.csr(n, n, rp, cc, cv)
    if shape == "rect_2to1":
        return ctx.gen_csr_uniform(0, 8_000_000, 4_000_000, 16, 0, seed=3)
    raise SystemExit(f"unknown shape {shape}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="c2_band,c2_uniform,lap2d_2048,rect_2to1")
    ap.add_argument("--damps", default="0,0.5")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    ctx = capi.Context(0)
    out = open(a.out, "a") if a.out else None
    for shape in a.shapes.split(","):
        A = make(ctx, shape)
        info = A.info
        nrow, ncol = int(info.nrow), int(info.ncol)
        b, x = ctx.gen_vector(nrow, seed=5), ctx.vector(ncol)
        xf, yf = ctx.gen_vector(ncol, seed=6), ctx.vector(nrow)
        xt, yt = ctx.gen_vector(nrow, seed=7), ctx.vector(ncol)
        yf.fill(0.0)
        yt.fill(0.0)
        ctx.sync()
        t0 = time.perf_counter()
        A.transpose_setup()
        setup_s = time.perf_counter() - t0
        for damp in (float(s) for s in a.damps.split(",")):

            def solve(iters):
                x.fill(0.0)
                ctx.sync()
                t = time.perf_counter()
                done, _, _ = ctx.cgls(A, b, x, max_iter=iters, rel_tol=0.0, check_every=iters, damp=damp)
                ctx.sync()
                assert done == iters, done
                return (time.perf_counter() - t) * 1e3

            solve(ITERS_SHORT)  # warm-up
            ctx.apply_timed(A, xf, yf, 2)
            ctx.apply_transpose_timed(A, xt, yt, 2)
            ms_s, ms_l, ms_f, ms_t = [], [], [], []
            for _ in range(a.rounds):
                ms_s.append(solve(ITERS_SHORT))
                ms_l.append(solve(ITERS_LONG))
                ms_f.append(ctx.apply_timed(A, xf, yf, REPS))
                ms_t.append(ctx.apply_transpose_timed(A, xt, yt, REPS))
            short, long_, mf, mt = (float(np.median(v)) for v in (ms_s, ms_l, ms_f, ms_t))
            mi = (long_ - short) / (ITERS_LONG - ITERS_SHORT)
            bytes_vectors = 8 * nrow + 32 * ncol + 24 * nrow + 8 * ncol + 24 * ncol
            rec = dict(shape=shape, nrow=nrow, ncol=ncol, nnz=int(info.nnz), damp=damp, iters_short=ITERS_SHORT, iters_long=ITERS_LONG, forward_kernel=int(info.kernel),
                       transpose_kernel=A.get_param("transpose_kernel"), transpose_setup_s=round(setup_s, 3), ms_iter=round(mi, 4),
                       ms_setup=round(short - ITERS_SHORT * mi, 4),
                       ms_forward=round(mf, 4), ms_transpose=round(mt, 4), over_products=round(mi / (mf + mt), 3),
                       ms_above_products=round(mi - mf - mt, 4), bytes_vectors=int(bytes_vectors), launches_per_iter=6,
                       rounds_short=[round(v, 4) for v in ms_s], rounds_long=[round(v, 4) for v in ms_l], rounds_forward=[round(v, 4) for v in ms_f],
                       rounds_transpose=[round(v, 4) for v in ms_t])
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
        del A, b, x, xf, yf, xt, yt
    if out:
        out.close()


if __name__ == "__main__":
    main()
