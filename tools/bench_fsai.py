#!/usr/bin/env python3
"""FSAI (spmv_fsai_setup / spmv_fsai_solve; SPMV_PRECOND_FSAI) measured: what the set-up costs and where, what one application costs
beside one product of A and one multicolour ILU(0) application of the same handle, and what it does to whole conjugate-gradient
solves beside the preconditioners the engine already had.

One JSON line per measurement, all from one process:
  kind "setup"   per (system, level): the wall time of spmv_fsai_setup (ms, the second of two calls) and its split by phase as the
                 handle reports it ("fsai_setup_us_*": pattern - the sparse products, the cut, offsets and columns; rows - the row
                 kernel; handles - the analysis of G, the transpose and its analysis), entries of G over entries of A, the longest
                 row, bytes, the kernels AUTO chose for G and G^T where the handle tells; a refused level leaves its message
  kind "apply"   per (system, level): one spmv_fsai_solve, one spmv_apply of A and one multicolour spmv_ilu0_solve, interleaved, REPS
                 calls between two device synchronisations (spmv_apply: between two device events), the median over --rounds rounds
                 after a warm-up; the two ratios
  kind "solve"   per (system, preconditioner): spmv_cg from x = 0 to rel_tol 1e-8 under none, ILU(0) (multicolour), Chebyshev of
                 degree 4, AMG, and FSAI of level 1, 2, 3 - iterations, the wall time of the whole call (set-ups outside the window; the
                 host looks every 10 iterations, every iteration under AMG as tools/bench_amg.py does), the reported residual
Systems: lap3d_160 (7-point Laplacian on 160^3 points) and lap2d_2048 (5-point, 2048^2), as tools/bench_ilu0.py builds them.

  python tools/bench_fsai.py [--systems lap3d_160,lap2d_2048] [--levels 1,2,3] [--out profiles/r21_bench_fsai.jsonl]
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
from __graft_entry__ import load_package  # noqa: E402
from bench_ilu0 import SHAPES, stencil  # noqa: E402

capi = load_package().capi
REPS = 10
REL_TOL = 1e-8
CHEBY_DEGREE = 4


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--systems", default="lap3d_160,lap2d_2048")
    ap.add_argument("--levels", default="1,2,3")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=20000)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    levels = [int(s) for s in a.levels.split(",")]
    ctx = capi.Context(0)
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def window(op):
        ctx.sync()
        t = time.perf_counter()
        for _ in range(REPS):
            op()
        ctx.sync()
        return (time.perf_counter() - t) * 1e3 / REPS

    for system in a.systems.split(","):
        m, dims, convection = SHAPES[system]
        n, rp, cc, cv = stencil(m, dims, convection)
        A = ctx.csr(n, n, rp, cc, cv)
        del rp, cc, cv
        b, x, z, y = ctx.gen_vector(n, seed=5), ctx.vector(n), ctx.vector(n), ctx.vector(n)
        y.fill(0.0)
        base = dict(system=system, nrow=n, nnz=int(A.info.nnz), forward_kernel=int(A.info.kernel))
        A.set_param("ilu0_order", 1)
        ctx.ilu0_setup(A)
        built = []
        for level in levels:
            rec = dict(kind="setup", **base, level=level)
            try:
                ctx.fsai_setup(A, level)  # (warms up: the context's scratch, the sort's first call)
                ctx.sync()
                t = time.perf_counter()
                ctx.fsai_setup(A, level)
                rec.update(ms=round((time.perf_counter() - t) * 1e3, 2))
            except capi.SpmvError as e:
                emit(dict(**rec, error=str(e)))
                continue
            built.append(level)
            _, g_nnz, longest = ctx.fsai_info(A)
            rec.update({f"ms_{k}": round(A.get_param(f"fsai_setup_us_{k}") / 1e3, 2) for k in ("pattern", "rows", "handles")},
                       g_nnz=g_nnz, g_over_a=round(g_nnz / A.info.nnz, 3), max_row=longest, bytes=int(A.get_param("fsai_bytes")))
            emit(rec)
            ms = {"fsai": [], "apply": [], "ilu0": []}
            for rnd in range(a.rounds + 1):  # round 0 warms up
                took = dict(fsai=window(lambda: ctx.fsai_solve(A, b, z)), apply=ctx.apply_timed(A, b, y, REPS),
                            ilu0=window(lambda: ctx.ilu0_solve(A, b, z)))
                if rnd:
                    for k, v in took.items():
                        ms[k].append(v)
            med = {k: float(np.median(v)) for k, v in ms.items()}
            emit(dict(kind="apply", **base, level=level, reps=REPS, ms_fsai=round(med["fsai"], 4), ms_apply=round(med["apply"], 4),
                      ms_ilu0=round(med["ilu0"], 4), fsai_over_apply=round(med["fsai"] / med["apply"], 2),
                      fsai_over_ilu0=round(med["fsai"] / med["ilu0"], 2), ilu0_launches=int(A.get_param("ilu0_launches"))))
        preconds = [("none", capi.PRECOND_NONE, 0), ("ilu0", capi.PRECOND_ILU0, 0), ("chebyshev", capi.PRECOND_CHEBYSHEV, 0),
                    ("amg", capi.PRECOND_AMG, 0)] + [(f"fsai{level}", capi.PRECOND_FSAI, level) for level in built]
        for name, code, level in preconds:
            rec = dict(kind="solve", **base, solver="cg", precond=name, rel_tol=REL_TOL)
            try:  # set-ups outside the window; the AMG set-up replaces the handle's Chebyshev state
                if code == capi.PRECOND_CHEBYSHEV:
                    ctx.chebyshev_setup(A, CHEBY_DEGREE)
                if code == capi.PRECOND_AMG:
                    ctx.amg_setup(A)
                if code == capi.PRECOND_FSAI:
                    ctx.fsai_setup(A, level)
                x.fill(0.0)
                ctx.sync()
                t = time.perf_counter()
                iters, res = ctx.cg(A, b, x, max_iter=a.max_iter, rel_tol=REL_TOL, check_every=1 if code == capi.PRECOND_AMG else 10, precond=code)
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
