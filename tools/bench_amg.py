#!/usr/bin/env python3
"""Aggregation AMG (spmv_amg_setup / spmv_amg_setup_smoothed / spmv_amg_solve; SPMV_PRECOND_AMG) measured, on the method of
tools/bench_chebyshev.py: what the set-up costs and builds, what one cycle costs next to the fine level's products, and what the cycle
buys the three solvers for square systems on the clock - the plain hierarchy and the smoothed one side by side, on two handles of the
same matrix, interleaved in one process.

One JSON line per measurement, printed as it is made, every figure from this one process ("hierarchy": "plain" or "smoothed"):
  {"kind": "setup", ...}     the set-up with the defaults (the second of two interleaved calls: the first warms up): ms, levels, rows
                             and entries per level, MIS rounds, bytes, launches per application; smoothed: the entries of P and the
                             lanes a row of P and R takes per level
  {"kind": "apply", ...}     one application (REPS of them between two device synchronisations) against 2 d + 2 products of the fine
                             handle - the products of level 0 in one cycle - (spmv_apply_timed), interleaved after a warm-up round, the
                             median over --rounds rounds: ms_amg, ms_products, ratio
  {"kind": "transfer", ...}  the smoothed hierarchy's restriction and prolongation of one level by themselves (spmv_amg_transfer_timed,
                             REPS calls between two events, interleaved, the median over --rounds rounds): the cycle's fused kernel
                             with the lanes the set-up chose, the same step as a vector pass and a product through the handle of R or
                             P, and the fused kernel under every number of lanes 1 .. 64 (the measurement behind amg_sa_settings.hpp)
  {"kind": "solve", ...}     iterations, wall time of the whole call and reported residual from x = 0 to rel_tol = 1e-8 (a look of the
                             host every 10 iterations; every iteration under AMG, whose counts are small) of spmv_cg (symmetric
                             systems), spmv_bicgstab and spmv_gmres(30) under none, chebyshev of degree 4, ilu0 (multicolour order),
                             amg (plain) and amg_sa (smoothed); set-ups outside the window
A solver that ends in an error leaves its message in place of the figures.

Systems (tools/bench_ilu0.py's stencils): lap2d_2048, lap3d_160, convdiff3d_160 (first-order upwind convection added).

  python tools/bench_amg.py [--systems lap2d_2048,...] [--solvers cg,bicgstab,gmres] [--preconds none,chebyshev,ilu0,amg,amg_sa]
                            [--max-iter N] [--out profiles/r17_bench_amg_sa.jsonl]
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
    ap.add_argument("--preconds", default="none,chebyshev,ilu0,amg,amg_sa")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=20000)
    ap.add_argument("--transfer-levels", type=int, default=2, help="levels whose restriction and prolongation are timed by themselves")
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
        handles = {"plain": ctx.csr(n, n, rp, cc, cv), "smoothed": ctx.csr(n, n, rp, cc, cv)}
        setups = {"plain": ctx.amg_setup, "smoothed": ctx.amg_setup_smoothed}
        del rp, cc, cv
        A = handles["plain"]
        b, x, z, y = ctx.gen_vector(n, seed=5), ctx.vector(n), ctx.vector(n), ctx.vector(n)
        y.fill(0.0)
        base = dict(system=system, nrow=n, nnz=int(A.info.nnz), forward_kernel=int(A.info.kernel))

        # ---- the set-ups, interleaved (round 0 warms up: the context's scratch, the sort's first call)
        ms_setup = {}
        for rnd in range(2):
            for name, H in list(handles.items()):
                ctx.sync()
                t = time.perf_counter()
                try:
                    setups[name](H)
                except capi.SpmvError as e:  # (a hierarchy that cannot be built leaves its message and the rest of its figures out)
                    emit(dict(kind="setup", hierarchy=name, **base, error=str(e)))
                    del handles[name]
                    continue
                ms_setup[name] = (time.perf_counter() - t) * 1e3
        degree = int(A.get_param("cheby_degree"))
        for name, H in handles.items():
            levels, rows, nnz = ctx.amg_info(H)
            rec = dict(kind="setup", hierarchy=name, **base, ms=round(ms_setup[name], 2), levels=levels, level_rows=rows.tolist(),
                       level_nnz=nnz.tolist(), mis_rounds=int(H.get_param("amg_mis_rounds")), bytes=int(H.get_param("amg_bytes")),
                       launches=int(H.get_param("amg_launches")), smooth_degree=degree)
            if name == "smoothed":
                rec.update(p_nnz=[len(ctx.amg_prolongator(H, l)[1]) for l in range(levels - 1)],
                           lanes_p=[int(H.get_param(f"amg_lanes_p{l}")) for l in range(levels - 1)],
                           lanes_r=[int(H.get_param(f"amg_lanes_r{l}")) for l in range(levels - 1)])
            emit(rec)

        # ---- one cycle of each next to the fine level's products
        products = 2 * degree + 2
        ms = {"plain": [], "smoothed": [], "products": []}
        for rnd in range(a.rounds + 1):  # round 0 warms up
            took = {}
            for name, H in handles.items():
                ctx.sync()
                t = time.perf_counter()
                for _ in range(REPS):
                    ctx.amg_solve(H, b, z)
                ctx.sync()
                took[name] = (time.perf_counter() - t) * 1e3 / REPS
            took["products"] = ctx.apply_timed(A, b, y, REPS * products) * products
            if rnd:
                for k, v in took.items():
                    ms[k].append(v)
        t_p = float(np.median(ms["products"]))
        for name in handles:
            t_a = float(np.median(ms[name]))
            emit(dict(kind="apply", hierarchy=name, **base, reps=REPS, products=products, ms_amg=round(t_a, 4), ms_products=round(t_p, 4),
                      ratio=round(t_a / t_p, 3)))

        # ---- the smoothed hierarchy's transfers by themselves
        S = handles.get("smoothed")
        levels, rows, _ = ctx.amg_info(S) if S is not None else (0, [], [])
        for level in range(min(a.transfer_levels, levels - 1)):
            v = ctx.vector(int(rows[level]))
            v.fill(0.0)
            variants = [("restrict_fused", capi.AMG_RESTRICT_FUSED, 0), ("restrict_unfused", capi.AMG_RESTRICT_UNFUSED, 0),
                        ("prolong_fused", capi.AMG_PROLONG_FUSED, 0), ("prolong_unfused", capi.AMG_PROLONG_UNFUSED, 0)]
            variants += [(f"restrict_lanes{g}", capi.AMG_RESTRICT_FUSED, g) for g in (1, 2, 4, 8, 16, 32, 64)]
            variants += [(f"prolong_lanes{g}", capi.AMG_PROLONG_FUSED, g) for g in (1, 2, 4, 8, 16, 32, 64)]
            ms = {name: [] for name, _, _ in variants}
            for rnd in range(a.rounds + 1):
                for name, what, lanes in variants:
                    t = ctx.amg_transfer_timed(S, level, what, v, REPS, lanes)
                    if rnd:
                        ms[name].append(t)
            emit(dict(kind="transfer", **base, level=level, level_rows=int(rows[level]), coarse_rows=int(rows[level + 1]),
                      p_nnz=len(ctx.amg_prolongator(S, level)[1]), lanes_p=int(S.get_param(f"amg_lanes_p{level}")),
                      lanes_r=int(S.get_param(f"amg_lanes_r{level}")), reps=REPS,
                      ms={name: round(float(np.median(t)), 5) for name, t in ms.items()}))
            del v

        # ---- the solvers
        A.set_param("ilu0_order", 1)
        preconds = [("none", capi.PRECOND_NONE, A), ("chebyshev", capi.PRECOND_CHEBYSHEV, A), ("ilu0", capi.PRECOND_ILU0, A),
                    ("amg", capi.PRECOND_AMG, A), ("amg_sa", capi.PRECOND_AMG, S)]
        preconds = [p for p in preconds if p[0] in a.preconds.split(",") and p[2] is not None]
        solvers = [s for s in a.solvers.split(",") if not (s == "cg" and convection)]
        for solver in solvers:
            call = {"cg": ctx.cg, "bicgstab": ctx.bicgstab, "gmres": ctx.gmres}[solver]
            for name, code, H in preconds:
                rec = dict(kind="solve", **base, solver=solver + ("(30)" if solver == "gmres" else ""), precond=name, rel_tol=REL_TOL)
                # set-ups outside the window; the AMG set-up replaces the handle's Chebyshev state and the other way round
                if code == capi.PRECOND_CHEBYSHEV:
                    ctx.chebyshev_setup(H, CHEBY_DEGREE)
                    rec.update(degree=CHEBY_DEGREE)
                if code == capi.PRECOND_ILU0:
                    ctx.ilu0_setup(H)
                if name == "amg":
                    ctx.amg_setup(H)
                x.fill(0.0)
                ctx.sync()
                t = time.perf_counter()
                try:
                    iters, res = call(H, b, x, max_iter=a.max_iter, rel_tol=REL_TOL, check_every=1 if code == capi.PRECOND_AMG else 10, precond=code)
                    ctx.sync()
                    rec.update(iters=iters, ms=round((time.perf_counter() - t) * 1e3, 2), rel_resid=float(f"{res:.3e}"))
                except capi.SpmvError as e:
                    rec.update(error=str(e))
                emit(rec)
        del A, S, handles, b, x, z, y
    if out:
        out.close()


if __name__ == "__main__":
    main()
