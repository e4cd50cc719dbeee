#!/usr/bin/env python3
"""Aggregation AMG (spmv_amg_setup / spmv_amg_solve; SPMV_PRECOND_AMG) measured, on the method of tools/bench_chebyshev.py: what the
set-up costs and builds, what one cycle costs next to the fine level's products, and what the cycle buys the three solvers for square
systems on the clock.

One JSON line per measurement, printed as it is made, every figure from this one process:
  {"kind": "setup", ...}   spmv_amg_setup with the defaults (the second of two calls: the first warms up): ms, levels, rows and entries
                           per level, MIS rounds, bytes, launches per application
  {"kind": "apply", ...}   one application (REPS of them between two device synchronisations) against 2 d + 2 products of the fine
                           handle - the products of level 0 in one cycle - (spmv_apply_timed), interleaved after a warm-up round, the
                           median over --rounds rounds: ms_amg, ms_products, ratio
  {"kind": "solve", ...}   iterations, wall time of the whole call and reported residual from x = 0 to rel_tol = 1e-8 (a look of the
                           host every 10 iterations; every iteration under AMG, whose counts are small) of spmv_cg (symmetric
                           systems), spmv_bicgstab and spmv_gmres(30) under none, chebyshev of degree 4, ilu0 (multicolour order) and
                           amg; set-ups outside the window
A solver that ends in an error leaves its message in place of the figures.

Systems (tools/bench_ilu0.py's stencils): lap2d_2048, lap3d_160, convdiff3d_160 (first-order upwind convection added).

  python tools/bench_amg.py [--systems lap2d_2048,...] [--solvers cg,bicgstab,gmres] [--max-iter N] [--out profiles/r15_bench_amg.jsonl]
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
sys.path.insert(0, str(ROOT / "tools"))
from bench_ilu0 import SHAPES, capi, stencil  # noqa: E402

REPS = 10
REL_TOL = 1e-8
SYSTEMS = ("lap2d_2048", "lap3d_160", "convdiff3d_160")
CHEBY_DEGREE = 4


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--systems", default=",".join(SYSTEMS))
    ap.add_argument("--solvers", default="cg,bicgstab,gmres")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=20000)
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

    for system in a.systems.split(","):
        m, dims, convection = SHAPES[system]
        n, rp, cc, cv = stencil(m, dims, convection)
        A = ctx.csr(n, n, rp, cc, cv)
        del rp, cc, cv
        b, x, z, y = ctx.gen_vector(n, seed=5), ctx.vector(n), ctx.vector(n), ctx.vector(n)
        y.fill(0.0)
        base = dict(system=system, nrow=n, nnz=int(A.info.nnz), forward_kernel=int(A.info.kernel))

        # ---- the set-up
        def amg_setup():
            ctx.sync()
            t = time.perf_counter()
            ctx.amg_setup(A)
            return (time.perf_counter() - t) * 1e3

        amg_setup()  # (warm-up: the context's scratch, the sort's first call)
        ms_setup = amg_setup()
        levels, rows, nnz = ctx.amg_info(A)
        degree = int(A.get_param("cheby_degree"))
        emit(dict(kind="setup", **base, ms=round(ms_setup, 2), levels=levels, level_rows=rows.tolist(), level_nnz=nnz.tolist(),
                  mis_rounds=int(A.get_param("amg_mis_rounds")), bytes=int(A.get_param("amg_bytes")), launches=int(A.get_param("amg_launches")),
                  smooth_degree=degree))

        # ---- one cycle next to the fine level's products
        products = 2 * degree + 2
        ms = {"amg": [], "products": []}
        for rnd in range(a.rounds + 1):  # round 0 warms up
            ctx.sync()
            t = time.perf_counter()
            for _ in range(REPS):
                ctx.amg_solve(A, b, z)
            ctx.sync()
            t_amg = (time.perf_counter() - t) * 1e3 / REPS
            t_products = ctx.apply_timed(A, b, y, REPS * products) * products
            if rnd:
                ms["amg"].append(t_amg)
                ms["products"].append(t_products)
        t_a, t_p = float(np.median(ms["amg"])), float(np.median(ms["products"]))
        emit(dict(kind="apply", **base, reps=REPS, products=products, ms_amg=round(t_a, 4), ms_products=round(t_p, 4), ratio=round(t_a / t_p, 3)))

        # ---- the solvers
        A.set_param("ilu0_order", 1)
        preconds = [("none", capi.PRECOND_NONE), ("chebyshev", capi.PRECOND_CHEBYSHEV), ("ilu0", capi.PRECOND_ILU0), ("amg", capi.PRECOND_AMG)]
        solvers = [s for s in a.solvers.split(",") if not (s == "cg" and convection)]
        for solver in solvers:
            call = {"cg": ctx.cg, "bicgstab": ctx.bicgstab, "gmres": ctx.gmres}[solver]
            for name, code in preconds:
                rec = dict(kind="solve", **base, solver=solver + ("(30)" if solver == "gmres" else ""), precond=name, rel_tol=REL_TOL)
                # set-ups outside the window; the AMG set-up replaces the handle's Chebyshev state and the other way round
                if code == capi.PRECOND_CHEBYSHEV:
                    ctx.chebyshev_setup(A, CHEBY_DEGREE)
                    rec.update(degree=CHEBY_DEGREE)
                if code == capi.PRECOND_ILU0:
                    ctx.ilu0_setup(A)
                if code == capi.PRECOND_AMG:
                    ctx.amg_setup(A)
                x.fill(0.0)
                ctx.sync()
                t = time.perf_counter()
                try:
                    iters, res = call(A, b, x, max_iter=a.max_iter, rel_tol=REL_TOL, check_every=1 if code == capi.PRECOND_AMG else 10, precond=code)
                    ctx.sync()
                    rec.update(iters=iters, ms=round((time.perf_counter() - t) * 1e3, 2), rel_resid=float(f"{res:.3e}"))
                except capi.SpmvError as e:
                    rec.update(error=str(e))
                emit(rec)
        del A, b, x, z, y
    if out:
        out.close()


if __name__ == "__main__":
    main()
