#!/usr/bin/env python3
"""One GMRES(30) iteration (spmv_gmres) against the forward product it is built on, and whole solves of spmv_gmres beside
spmv_bicgstab: where an iteration's time goes beyond its product - the two Gram-Schmidt passes - and whether half the products and
preconditioner applications per iteration pay on the clock.

Part 1, one JSON line per (shape, precond) with "part": "iteration" - tools/bench_bicgstab.py's method.  The median over --rounds
rounds of
  ms_iter        one iteration of spmv_gmres: the difference of a solve of ITERS_LONG and one of ITERS_SHORT iterations over the
                 difference of the counts, both inside ONE cycle of m = 30 (rel_tol = 0, one look of the host at the end, from
                 x = 0, set again before every solve and outside the timed window; a window is one whole call between two device
                 synchronisations).  The iterations between the two counts are the columns j = ITERS_SHORT .. ITERS_LONG - 1;
  ms_short, ms_long   the two solves themselves (the short one's columns are narrower than those between the counts, so no set-up
                 time is derived from them: both hold the work vectors, their clearing, the first residual and the update of x);
  ms_forward     spmv_apply_timed (REPS products between two device events);
the two interleaved in the same process after a warm-up.  over_product = ms_iter / ms_forward.
bytes_ortho: what the five vector kernels of column j must move (csrc/solver_gmres.hip): 8 nrow (4 (j + 1) + 2 ceil((j + 1) / 8) + 6)
bytes (Jacobi: + 2 nrow words in the normalisation), averaged over the columns between the two counts; ortho_gbps is that over
ms_iter - ms_forward.

Part 2, one JSON line per shape with "part": "solves": from x = 0 to rel_tol = 1e-8 (a look of the host every 10 iterations; the wall
time of the whole call), iterations / ms / reported residual of spmv_gmres (m = 30) and spmv_bicgstab with none, jacobi and
multicolour ilu0.  A solver that ends in an error leaves its message in place of the figures.  A line per solve goes to stderr as
it ends.

Shapes: c2_band (CSR 10M x 10M x 32, columns in a band of 65536) and lap2d_2048 (the 5-point Laplacian on 2048^2 points) for part 1;
lap3d_160 and convdiff3d_160 (tools/bench_ilu0.py's 160^3 stencils) for part 2.

  python tools/bench_gmres.py [--iteration-shapes c2_band,lap2d_2048] [--solve-shapes lap3d_160,convdiff3d_160] [--out profiles/r13_bench_gmres.jsonl]
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
sys.path[:0] = [str(ROOT), str(ROOT / "tools")]
from __graft_entry__ import load_package  # noqa: E402

capi = load_package().capi
RESTART = 30
ITERS_SHORT, ITERS_LONG = 10, 26
REPS = 20
REL_TOL = 1e-8
MAX_ITER = 20000
TILE = 8  # csrc/solver_gmres.hip: kGmresTile


def ortho_words(j, jacobi):
    """8-byte words per row the five vector kernels of column j move"""
    return 4 * (j + 1) + 2 * -(-(j + 1) // TILE) + 6 + (2 if jacobi else 0)


def make_iteration_shape(ctx, shape):
    if shape == "c2_band":
        n = 10_000_000
        return ctx.gen_csr_uniform(0, n, n, 32, 65536, seed=3)
    if shape == "lap2d_2048":
        from bench_bicgstab import laplacian_2d

        n, rp, cc, cv = laplacian_2d(2048)
        return ctx.csr(n, n, rp, cc, cv)
    raise SystemExit(f"unknown shape {shape}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iteration-shapes", default="c2_band,lap2d_2048")
    ap.add_argument("--solve-shapes", default="lap3d_160,convdiff3d_160")
    ap.add_argument("--preconds", default="0,1", help="part 1: 0 plain, 1 Jacobi")
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

    for shape in [s for s in a.iteration_shapes.split(",") if s]:
        A = make_iteration_shape(ctx, shape)
        info = A.info
        nrow = int(info.nrow)
        b, x = ctx.gen_vector(nrow, seed=5), ctx.vector(nrow)
        xf, yf = ctx.gen_vector(nrow, seed=6), ctx.vector(nrow)
        yf.fill(0.0)
        ctx.sync()
        for precond in (int(s) for s in a.preconds.split(",")):
            base = dict(part="iteration", shape=shape, nrow=nrow, nnz=int(info.nnz), precond=precond, restart=RESTART, iters_short=ITERS_SHORT,
                        iters_long=ITERS_LONG)

            def solve(iters):
                x.fill(0.0)
                ctx.sync()
                t = time.perf_counter()
                done, res = ctx.gmres(A, b, x, restart=RESTART, max_iter=iters, rel_tol=0.0, check_every=iters, precond=precond)
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
            words = float(np.mean([ortho_words(j, precond == 1) for j in range(ITERS_SHORT, ITERS_LONG)]))
            bytes_ortho = 8.0 * nrow * words
            emit(dict(base, forward_kernel=int(A.info.kernel), rel_resid_long=res_l, ms_iter=round(mi, 4), ms_short=round(short, 4), ms_long=round(long_, 4),
                      ms_forward=round(mf, 4), over_product=round(mi / mf, 3), ms_above_product=round(mi - mf, 4), words_per_row=round(words, 2),
                      bytes_ortho=int(bytes_ortho), ortho_gbps=round(bytes_ortho / max(mi - mf, 1e-9) / 1e6, 1), launches_per_iter=6,
                      rounds_short=[round(v, 4) for v in ms_s], rounds_long=[round(v, 4) for v in ms_l], rounds_forward=[round(v, 4) for v in ms_f]))
        del A, b, x, xf, yf

    from bench_ilu0 import SHAPES, stencil

    for shape in [s for s in a.solve_shapes.split(",") if s]:
        m, dims, convection = SHAPES[shape]
        n, rp, cc, cv = stencil(m, dims, convection)
        A = ctx.csr(n, n, rp, cc, cv)
        del rp, cc, cv
        A.set_param("ilu0_order", 1)
        b, x = ctx.gen_vector(n, seed=5), ctx.vector(n)
        rec = dict(part="solves", shape=shape, nrow=n, nnz=int(A.info.nnz), rel_tol=REL_TOL, restart=RESTART, ilu0_order=1)
        runs = [(solver, name, p) for name, p in (("none", capi.PRECOND_NONE), ("jacobi", capi.PRECOND_JACOBI), ("ilu0", capi.PRECOND_ILU0))
                for solver in ("gmres", "bicgstab")]
        ctx.ilu0_setup(A)  # outside every window, for both solvers alike
        for solver, name, p in runs:
            x.fill(0.0)
            ctx.sync()
            t = time.perf_counter()
            try:
                if solver == "gmres":
                    iters, res = ctx.gmres(A, b, x, restart=RESTART, max_iter=MAX_ITER, rel_tol=REL_TOL, check_every=10, precond=p)
                else:
                    iters, res = ctx.bicgstab(A, b, x, max_iter=MAX_ITER, rel_tol=REL_TOL, check_every=10, precond=p)
                ctx.sync()
                rec[f"{solver}_{name}"] = dict(iters=iters, ms=round((time.perf_counter() - t) * 1e3, 2), rel_resid=float(f"{res:.3e}"))
            except capi.SpmvError as e:
                rec[f"{solver}_{name}"] = dict(error=str(e))
            print(f"# {shape} {solver}_{name}: {rec[f'{solver}_{name}']}", file=sys.stderr, flush=True)
        emit(rec)
        del A, b, x
    if out:
        out.close()


if __name__ == "__main__":
    main()
