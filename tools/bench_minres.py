#!/usr/bin/env python3
"""One MINRES iteration (spmv_minres) against the forward product it is built on, and whole solves beside the solvers that took these
systems before: what the three vector kernels of an iteration cost beyond the product, what a shift inside the spectrum costs each
solver, and what MINRES loses to spmv_cg where the matrix is positive definite after all.

Part 1, one JSON line per (shape, precond) with "part": "iteration" - tools/bench_gmres.py's method.  The median over --rounds rounds of
  ms_iter        one iteration of spmv_minres: the difference of a solve of ITERS_LONG and one of ITERS_SHORT iterations over the
                 difference of the counts (rel_tol = 0, one look of the host at the end, from x = 0, set again before every solve and
                 outside the timed window; a window is one whole call between two device synchronisations);
  ms_forward     spmv_apply_timed (REPS products between two device events);
the two interleaved in the same process after a warm-up.  over_product = ms_iter / ms_forward.
bytes_vectors: what the three vector kernels of an iteration must move (csrc/solver_minres.hip): 15 doubles per row - launch 2 reads
q, v and r1 and writes q; launch 3 reads q and r2 and writes q; launch 4 reads v, w1, w2, y and x and writes w, x and v - and 17 with
Jacobi (dinv in, y out); vectors_gbps is that over ms_iter - ms_forward.
Shapes: lap2d_2048 (the 5-point Laplacian on 2048^2 points), lap3d_160 (the 7-point one on 160^3) and c2_band (CSR 10M x 10M x 32,
columns in a band of 65536: not symmetric, so timing only - the recurrence runs whatever the matrix is).

Part 2, one JSON line with "part": "shifted_solves": the 2048^2 Laplacian with a shift in the widest gap between its 11th and 40th
eigenvalues, from x = 0 to rel_tol = 1e-8 within MAX_ITER iterations (a look of the host every 10; the wall time of the whole call):
spmv_minres without a preconditioner and with P = the Laplacian under FSAI, Chebyshev and AMG (their set-up outside every window),
beside spmv_gmres(30) and spmv_bicgstab without a preconditioner on A - shift I built on the host.  The preconditioned solves stop on
the M^-1 norm of the residual, the others on its 2-norm.  A solver that ends in an error leaves its message in place of the figures.

Part 3, one JSON line with "part": "spd_solves": the unshifted Laplacian, spmv_minres beside spmv_cg, plain and Jacobi.

  python tools/bench_minres.py [--iteration-shapes lap2d_2048,lap3d_160,c2_band] [--out FILE]
Without --out the lines go to the next free profiles/rNN_bench_minres.jsonl.  Needs a GPU; there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import re
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tools")]
from __graft_entry__ import load_package  # noqa: E402

capi = load_package().capi
ITERS_SHORT, ITERS_LONG = 20, 60
REPS = 20
REL_TOL = 1e-8
MAX_ITER = 20000
RESTART = 30
WORDS = {capi.PRECOND_NONE: 15, capi.PRECOND_JACOBI: 17}  # doubles per row the vector kernels move


def next_free_out():
    taken = [int(m.group(1)) for f in (ROOT / "profiles").iterdir() if (m := re.match(r"r(\d+)[a-z]?_", f.name))]
    return ROOT / "profiles" / f"r{max(taken, default=0) + 1:02d}_bench_minres.jsonl"


def laplacian_2d(m):
    from bench_bicgstab import laplacian_2d as build

    return build(m)


def make_iteration_shape(ctx, shape):
    if shape == "c2_band":
        n = 10_000_000
        return ctx.gen_csr_uniform(0, n, n, 32, 65536, seed=3)
    if shape == "lap2d_2048":
        n, rp, cc, cv = laplacian_2d(2048)
        return ctx.csr(n, n, rp, cc, cv)
    if shape == "lap3d_160":
        from bench_ilu0 import SHAPES, stencil

        m, dims, convection = SHAPES[shape]
        n, rp, cc, cv = stencil(m, dims, convection)
        return ctx.csr(n, n, rp, cc, cv)
    raise SystemExit(f"unknown shape {shape}")


def shift_in_the_spectrum(m):
    """a shift in the widest gap between the 11th and the 40th eigenvalue of the 5-point Laplacian on an m x m grid"""
    a = 4 * np.sin(np.arange(1, 12) * np.pi / (2 * (m + 1))) ** 2
    lam = np.sort((a[:, None] + a[None, :]).ravel())[:40]
    at = 10 + int(np.argmax(np.diff(lam[10:])))
    return float((lam[at] + lam[at + 1]) / 2), at + 1, float(lam[at + 1] - lam[at])


def timed(ctx, x, run):
    x.fill(0.0)
    ctx.sync()
    t = time.perf_counter()
    try:
        iters, res = run()[:2]
        ctx.sync()
        out = dict(iters=int(iters), ms=round((time.perf_counter() - t) * 1e3, 2), rel_resid=float(f"{res:.3e}"))
        if iters > 0:
            out["ms_per_iter"] = round(out["ms"] / iters, 4)
        return out
    except capi.SpmvError as e:
        return dict(error=str(e))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iteration-shapes", default="lap2d_2048,lap3d_160,c2_band")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="the file the JSON lines are appended to (default: the next free profiles/rNN_bench_minres.jsonl)")
    a = ap.parse_args()
    ctx = capi.Context(0)
    out = open(a.out or next_free_out(), "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
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
        for precond in (capi.PRECOND_NONE,) if shape == "c2_band" else (capi.PRECOND_NONE, capi.PRECOND_JACOBI):
            base = dict(part="iteration", shape=shape, nrow=nrow, nnz=int(info.nnz), precond=precond, shift=0.5, iters_short=ITERS_SHORT, iters_long=ITERS_LONG)

            def solve(iters):
                x.fill(0.0)
                ctx.sync()
                t = time.perf_counter()
                done, res = ctx.minres(A, b, x, shift=0.5, max_iter=iters, rel_tol=0.0, check_every=iters, precond=precond)
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
            bytes_vectors = 8.0 * nrow * WORDS[precond]
            emit(dict(base, forward_kernel=int(A.info.kernel), rel_resid_long=res_l, ms_iter=round(mi, 4), ms_short=round(short, 4), ms_long=round(long_, 4),
                      ms_forward=round(mf, 4), over_product=round(mi / mf, 3), ms_above_product=round(mi - mf, 4), words_per_row=WORDS[precond],
                      bytes_vectors=int(bytes_vectors), vectors_gbps=round(bytes_vectors / max(mi - mf, 1e-9) / 1e6, 1), launches_per_iter=4,
                      rounds_short=[round(v, 4) for v in ms_s], rounds_long=[round(v, 4) for v in ms_l], rounds_forward=[round(v, 4) for v in ms_f]))
        del A, b, x, xf, yf

    m = 2048
    n, rp, cc, cv = laplacian_2d(m)
    shift, below, gap = shift_in_the_spectrum(m)
    A = ctx.csr(n, n, rp, cc, cv)
    rows = np.repeat(np.arange(n), np.diff(rp))
    S = ctx.csr(n, n, rp, cc, np.where(rows == cc, cv - shift, cv))  # A - shift I, for the solvers that take no shift
    del rows
    b, x = ctx.gen_vector(n, seed=5), ctx.vector(n)
    rec = dict(part="shifted_solves", shape=f"lap2d_{m}", nrow=n, nnz=int(A.info.nnz), shift=shift, eigenvalues_below=below, gap=gap, rel_tol=REL_TOL,
               max_iter=MAX_ITER, restart=RESTART)
    P = {name: ctx.csr(n, n, rp, cc, cv) for name in ("fsai", "chebyshev", "amg")}  # a handle of its own for each preconditioner's state
    ctx.fsai_setup(P["fsai"])
    ctx.chebyshev_setup(P["chebyshev"])
    ctx.amg_setup(P["amg"])
    codes = dict(fsai=capi.PRECOND_FSAI, chebyshev=capi.PRECOND_CHEBYSHEV, amg=capi.PRECOND_AMG)
    runs = [("minres_none", lambda: ctx.minres(A, b, x, shift=shift, max_iter=MAX_ITER, rel_tol=REL_TOL, check_every=10))]
    for name in P:
        runs.append((f"minres_{name}", lambda name=name: ctx.minres(A, b, x, shift=shift, P=P[name], max_iter=MAX_ITER, rel_tol=REL_TOL, check_every=10,
                                                                    precond=codes[name])))
    runs.append(("gmres_none", lambda: ctx.gmres(S, b, x, restart=RESTART, max_iter=MAX_ITER, rel_tol=REL_TOL, check_every=10)))
    runs.append(("bicgstab_none", lambda: ctx.bicgstab(S, b, x, max_iter=MAX_ITER, rel_tol=REL_TOL, check_every=10)))
    for name, run in runs:
        rec[name] = timed(ctx, x, run)
        print(f"# shifted {name}: {rec[name]}", file=sys.stderr, flush=True)
    emit(rec)
    del S, P
    rec = dict(part="spd_solves", shape=f"lap2d_{m}", nrow=n, nnz=int(A.info.nnz), rel_tol=REL_TOL, max_iter=MAX_ITER)
    for pname, p in (("none", capi.PRECOND_NONE), ("jacobi", capi.PRECOND_JACOBI)):
        rec[f"minres_{pname}"] = timed(ctx, x, lambda: ctx.minres(A, b, x, max_iter=MAX_ITER, rel_tol=REL_TOL, check_every=10, precond=p))
        rec[f"cg_{pname}"] = timed(ctx, x, lambda: ctx.cg(A, b, x, max_iter=MAX_ITER, rel_tol=REL_TOL, check_every=10, precond=p))
        print(f"# spd {pname}: minres {rec[f'minres_{pname}']}, cg {rec[f'cg_{pname}']}", file=sys.stderr, flush=True)
    emit(rec)
    out.close()


if __name__ == "__main__":
    main()
