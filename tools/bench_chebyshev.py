#!/usr/bin/env python3
"""The Chebyshev polynomial preconditioner (spmv_chebyshev_setup / spmv_chebyshev_solve; SPMV_PRECOND_CHEBYSHEV) measured, on the
method of tools/bench_ilu0.py: what a term costs above its product, and what the polynomial buys the three solvers for square systems.

One JSON line per measurement, printed as it is made:
  {"kind": "apply", ...}   one application at degree 1, 2, 4, 8 (REPS of them between two device synchronisations) against that many
                           products of the same handle (spmv_apply_timed), interleaved in the same process after a warm-up round, the
                           median over --rounds rounds: ms_cheby, ms_products, and over_products = (ms_cheby - ms_products) / degree,
                           what one term costs above its product - the number a fused product-and-update kernel would attack
  {"kind": "setup", ...}   spmv_chebyshev_setup per bound source: "row" the row bound alone, "lanczos" with "cheby_lanczos_steps" 16
                           (the smaller of the row bound and 1.05 ritz_max); ms, lmin, lmax, where lmax came from
  {"kind": "solve", ...}   iterations, wall time of the whole call and reported residual from x = 0 to rel_tol = 1e-8 (a look of the
                           host every 10 iterations) of spmv_cg (symmetric systems), spmv_bicgstab and spmv_gmres(30) under none,
                           jacobi, ilu0 (multicolour order) and chebyshev of degree 2, 4, 8 with either bound source
A solver that ends in an error leaves its message in place of the figures.  No row-order ILU(0): it takes minutes.

Systems (tools/bench_ilu0.py's stencils): lap3d_160, convdiff3d_160 (first-order upwind convection added), lap2d_2048.

  python tools/bench_chebyshev.py [--systems lap3d_160,...] [--solvers cg,bicgstab,gmres] [--max-iter N] [--out profiles/r14_bench_chebyshev.jsonl]
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
APPLY_DEGREES = (1, 2, 4, 8)
SOLVE_DEGREES = (2, 4, 8)
SYSTEMS = ("lap3d_160", "convdiff3d_160", "lap2d_2048")
LANCZOS_STEPS = 16


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

        # ---- a term above its product
        for degree in APPLY_DEGREES:
            ctx.chebyshev_setup(A, degree)
            ms = {"cheby": [], "products": []}
            for rnd in range(a.rounds + 1):  # round 0 warms up
                ctx.sync()
                t = time.perf_counter()
                for _ in range(REPS):
                    ctx.chebyshev_solve(A, b, z)
                ctx.sync()
                t_cheby = (time.perf_counter() - t) * 1e3 / REPS
                t_products = ctx.apply_timed(A, b, y, REPS * degree) * degree
                if rnd:
                    ms["cheby"].append(t_cheby)
                    ms["products"].append(t_products)
            t_c, t_p = float(np.median(ms["cheby"])), float(np.median(ms["products"]))
            emit(dict(kind="apply", **base, degree=degree, reps=REPS, launches=int(A.get_param("cheby_launches")), bytes=int(A.get_param("cheby_bytes")),
                      ms_cheby=round(t_c, 4), ms_products=round(t_p, 4), over_products=round((t_c - t_p) / degree, 4)))

        # ---- the solvers
        def setup(source, degree):
            A.set_param("cheby_lanczos_steps", LANCZOS_STEPS if source == "lanczos" else 0)
            ctx.sync()
            t = time.perf_counter()
            ctx.chebyshev_setup(A, degree)
            ms_setup = (time.perf_counter() - t) * 1e3
            _, _, lmin, lmax = ctx.chebyshev_info(A)
            return dict(ms=round(ms_setup, 3), lmin=lmin, lmax=lmax, lmax_source=int(A.get_param("cheby_lmax_source")))

        for source in ("row", "lanczos"):
            setup(source, 4)  # (warm-up)
            emit(dict(kind="setup", **base, bounds=source, degree=4, **setup(source, 4)))
        A.set_param("ilu0_order", 1)
        preconds = [("none", capi.PRECOND_NONE, 0, None), ("jacobi", capi.PRECOND_JACOBI, 0, None), ("ilu0", capi.PRECOND_ILU0, 0, None)]
        preconds += [("chebyshev", capi.PRECOND_CHEBYSHEV, d, src) for d in SOLVE_DEGREES for src in ("row", "lanczos")]
        solvers = [s for s in a.solvers.split(",") if not (s == "cg" and convection)]
        for solver in solvers:
            call = {"cg": ctx.cg, "bicgstab": ctx.bicgstab, "gmres": ctx.gmres}[solver]
            for name, code, degree, source in preconds:
                rec = dict(kind="solve", **base, solver=solver + ("(30)" if solver == "gmres" else ""), precond=name, rel_tol=REL_TOL)
                if code == capi.PRECOND_CHEBYSHEV:
                    rec.update(degree=degree, bounds=source, lmax=setup(source, degree)["lmax"])
                if code == capi.PRECOND_ILU0:
                    ctx.ilu0_setup(A)  # (outside the window, as the polynomial's)
                x.fill(0.0)
                ctx.sync()
                t = time.perf_counter()
                try:
                    iters, res = call(A, b, x, max_iter=a.max_iter, rel_tol=REL_TOL, check_every=10, precond=code)
                    ctx.sync()
                    rec.update(iters=iters, ms=round((time.perf_counter() - t) * 1e3, 2), rel_resid=float(f"{res:.3e}"))
                    if code == capi.PRECOND_CHEBYSHEV:
                        rec.update(products=iters * (degree + 1) * (2 if solver == "bicgstab" else 1))
                except capi.SpmvError as e:
                    rec.update(error=str(e))
                emit(rec)
        del A, b, x, z, y
    if out:
        out.close()


if __name__ == "__main__":
    main()
