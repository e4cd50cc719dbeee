#!/usr/bin/env python3
"""One BiCGSTAB iteration (spmv_bicgstab) against the two forward products it is built on: how far an iteration is above two
spmv_apply of the same handle - that is, what its two dot kernels, three vector kernels and seven launches cost.

One JSON line per (shape, precond): the median over --rounds rounds of
  ms_iter        one iteration of spmv_bicgstab: the difference of a solve of ITERS_LONG and one of ITERS_SHORT iterations over the
                 difference of the counts (rel_tol = 0, one look of the host at the end, from x = 0, set again before every solve
                 and outside the timed window; a window is one whole call between two device synchronisations);
  ms_setup       what the short solve takes beyond its iterations: the work vectors, the first residual (Jacobi: the diagonal);
  ms_forward     spmv_apply_timed (REPS products between two device events);
the two interleaved in the same process after a warm-up.  over_products = ms_iter / (2 ms_forward).
bytes_vectors: what the five vector kernels of an iteration must move, in doubles of nrow - rhat.v 2 (rhat, v read); the half step 3
(r, v read, s written); t.s and t.t 2 (t, s read); the update 7 (x read and written, phat, shat, t, rhat read, r written; plain, phat
and shat are p and s); the direction 4 (r, v, p read, p written): 18 nrow doubles, on top of the products' own reads of phat and
shat and writes of v and t.  Jacobi adds dinv read and shat written in the half step and dinv read and phat written in the
direction: 22.

The shapes are the benchmark's matrices, not systems chosen to converge: with rel_tol = 0 every iteration runs its seven launches
whatever the residual does, unless a breakdown, a non-finite residual or (Jacobi on the generated matrices) a missing diagonal
entry ends the solve - then the line carries the error instead of a time.  lap2d_2048 converges, but 50 iterations leave its
residual (rel_resid_long) far above the solver's quiet floor of 1e-14, below which an iteration's vector kernels do nothing.

Shapes: c2_band (CSR 10M x 10M x 32, columns in a band of 65536), c2_uniform (the same, uniform columns), lap2d_2048 (the 5-point
Laplacian on 2048^2 points, 4.2M rows).

  python tools/bench_bicgstab.py [--shapes c2_band,c2_uniform,lap2d_2048] [--out profiles/r11_bench_bicgstab.jsonl]
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
    raise SystemExit(f"unknown shape {shape}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="c2_band,c2_uniform,lap2d_2048")
    ap.add_argument("--preconds", default="0,1", help="0 plain, 1 Jacobi")
    ap.add_argument("--rounds", type=int, default=5)
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

    for shape in a.shapes.split(","):
        A = make(ctx, shape)
        info = A.info
        nrow = int(info.nrow)
        b, x = ctx.gen_vector(nrow, seed=5), ctx.vector(nrow)
        xf, yf = ctx.gen_vector(nrow, seed=6), ctx.vector(nrow)
        yf.fill(0.0)
        ctx.sync()
        for precond in (int(s) for s in a.preconds.split(",")):
            base = dict(shape=shape, nrow=nrow, nnz=int(info.nnz), precond=precond, iters_short=ITERS_SHORT, iters_long=ITERS_LONG)

            def solve(iters):
                x.fill(0.0)
                ctx.sync()
                t = time.perf_counter()
                done, res = ctx.bicgstab(A, b, x, max_iter=iters, rel_tol=0.0, check_every=iters, precond=precond)
                ctx.sync()
                assert done == iters, done
                return (time.perf_counter() - t) * 1e3, res

            try:
                solve(ITERS_SHORT)  # warm-up
                ctx.apply_timed(A, xf, yf, 2)
                ms_s, ms_l, ms_f, res_l = [], [], [], 0.0
                for _ in range(a.rounds):
                    ms_s.append(solve(ITERS_SHORT)[0])
                    ms, res_l = solve(ITERS_LONG)
                    ms_l.append(ms)
                    ms_f.append(ctx.apply_timed(A, xf, yf, REPS))
            except capi.SpmvError as e:
                emit(dict(base, error=str(e)))
                continue
            short, long_, mf = (float(np.median(v)) for v in (ms_s, ms_l, ms_f))
            mi = (long_ - short) / (ITERS_LONG - ITERS_SHORT)
            bytes_vectors = 8 * nrow * (22 if precond else 18)
            emit(dict(base, forward_kernel=int(A.info.kernel), rel_resid_long=res_l, ms_iter=round(mi, 4), ms_setup=round(short - ITERS_SHORT * mi, 4),
                      ms_forward=round(mf, 4), over_products=round(mi / (2 * mf), 3), ms_above_products=round(mi - 2 * mf, 4),
                      bytes_vectors=int(bytes_vectors), vector_gbps=round(bytes_vectors / max(mi - 2 * mf, 1e-9) / 1e6, 1), launches_per_iter=7,
                      rounds_short=[round(v, 4) for v in ms_s], rounds_long=[round(v, 4) for v in ms_l], rounds_forward=[round(v, 4) for v in ms_f]))
        del A, b, x, xf, yf
    if out:
        out.close()


if __name__ == "__main__":
    main()
