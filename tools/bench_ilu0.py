#!/usr/bin/env python3
"""ILU(0) (spmv_ilu0_setup / spmv_ilu0_solve; SPMV_PRECOND_ILU0) measured: what the set-up costs, what one application costs beside
one product and beside one Gauss-Seidel sweep of the same handle, and what it buys the two solvers for square systems.

One JSON line per (shape, order); order 0 is the matrix's own row order, 1 the multicolour order.  The median over --rounds rounds,
the operations interleaved in the same process after a warm-up:
  ms_setup       spmv_ilu0_setup (synchronous: order, symbolic, levels, numeric), forced by switching "ilu0_order" there and back
  ms_solve       one spmv_ilu0_solve: REPS applications between two device synchronisations
  ms_apply       one spmv_apply of the same handle (spmv_apply_timed, REPS products between two device events)
  ms_symgs       one spmv_symgs sweep in the same order ("symgs_order" = order) from the x it is given: the preconditioner's sweep
                 from z = 0 saves the first product of the general scheme and nothing of the fused one
  solve_over_apply, solve_over_symgs   the two ratios
  launches, levels_forward, levels_backward, colours, bytes   what the handle reports ("ilu0_*")
and, once each from x = 0 to rel_tol = 1e-8 (a look of the host every 10 iterations; the wall time of the whole call),
  cg_<precond>        iterations / ms / reported residual of spmv_cg with none, jacobi, symgs, ilu0 - on the symmetric shapes
  bicgstab_<precond>  the same of spmv_bicgstab with none, jacobi, ilu0
A solver that ends in an error leaves its message in place of the figures.

Shapes: lap3d_160 (7-point Laplacian on 160^3 points), lap2d_2048 (5-point, 2048^2), and convdiff3d_160 / convdiff2d_2048, the same
stencils with first-order upwind convection (velocity 1.5, 0.5(, 0.25)) added: nonsymmetric M-matrices with a constant diagonal.

  python tools/bench_ilu0.py [--shapes lap3d_160,...] [--orders 0,1] [--out profiles/r12_bench_ilu0.jsonl]
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
REPS = 10
REL_TOL = 1e-8
MAX_ITER = 20000
VELOCITY = (1.5, 0.5, 0.25)


def stencil(m, dims, convection):
    """(n, row_ptr, col, val) of the (2 dims + 1)-point diffusion stencil on an m^dims grid, Dirichlet boundary, plus (convection)
    first-order upwind convection: -(1 + c_d) towards the lower neighbour of dimension d, -1 towards the upper one, the diagonal
    2 dims + sum c_d.  Rows and columns ascending, built in that order"""
    n = m**dims
    i = np.arange(n, dtype=np.int64)
    c = [VELOCITY[d] if convection else 0.0 for d in range(dims)]
    cols, vals, ok = [], [], []
    for d in reversed(range(dims)):  # the lower neighbours, farthest first
        stride = m**d
        cols.append(i - stride)
        vals.append(np.full(n, -(1.0 + c[d])))
        ok.append((i // stride) % m > 0)
    cols.append(i)
    vals.append(np.full(n, 2.0 * dims + sum(c)))
    ok.append(np.ones(n, bool))
    for d in range(dims):
        stride = m**d
        cols.append(i + stride)
        vals.append(np.full(n, -1.0))
        ok.append((i // stride) % m < m - 1)
    cols, vals, ok = np.stack(cols, 1), np.stack(vals, 1), np.stack(ok, 1)
    rp = np.concatenate([[0], np.cumsum(ok.sum(1))]).astype(np.int32)
    return n, rp, cols[ok].astype(np.int32), vals[ok]


SHAPES = {"lap3d_160": (160, 3, False), "lap2d_2048": (2048, 2, False), "convdiff3d_160": (160, 3, True), "convdiff2d_2048": (2048, 2, True)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--orders", default="1,0")
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

    for shape in a.shapes.split(","):
        m, dims, convection = SHAPES[shape]
        n, rp, cc, cv = stencil(m, dims, convection)
        A = ctx.csr(n, n, rp, cc, cv)
        del rp, cc, cv
        b, x, z, y = ctx.gen_vector(n, seed=5), ctx.vector(n), ctx.vector(n), ctx.vector(n)
        y.fill(0.0)
        for order in (int(s) for s in a.orders.split(",")):
            rec = dict(shape=shape, nrow=n, nnz=int(A.info.nnz), order=order, reps=REPS, rel_tol=REL_TOL)
            A.set_param("symgs_order", order)
            ctx.symgs_order(A)  # the sweep's set-up, outside every window
            ms = {"setup": [], "solve": [], "apply": [], "symgs": []}

            def window(op):
                ctx.sync()
                t = time.perf_counter()
                for _ in range(REPS):
                    op()
                ctx.sync()
                return (time.perf_counter() - t) * 1e3 / REPS

            for rnd in range(a.rounds + 1):  # round 0 warms up
                A.set_param("ilu0_order", 1 - order)
                ctx.ilu0_setup(A)
                A.set_param("ilu0_order", order)
                ctx.sync()
                t = time.perf_counter()
                ctx.ilu0_setup(A)
                t_setup = (time.perf_counter() - t) * 1e3
                t_solve = window(lambda: ctx.ilu0_solve(A, b, z))
                t_apply = ctx.apply_timed(A, b, y, REPS)
                x.fill(0.0)
                t_symgs = window(lambda: ctx.symgs(A, b, x, 1))
                if rnd:
                    for k, v in (("setup", t_setup), ("solve", t_solve), ("apply", t_apply), ("symgs", t_symgs)):
                        ms[k].append(v)
            med = {k: float(np.median(v)) for k, v in ms.items()}
            rec.update({f"ms_{k}": round(v, 4) for k, v in med.items()})
            rec.update(solve_over_apply=round(med["solve"] / med["apply"], 2), solve_over_symgs=round(med["solve"] / med["symgs"], 2),
                       forward_kernel=int(A.info.kernel), **{k: int(A.get_param(f"ilu0_{k}")) for k in ("launches", "levels_forward", "levels_backward", "colours", "bytes")},
                       symgs_launches=int(A.get_param("symgs_launches")), symgs_fused=int(A.get_param("symgs_fused")))
            runs = [("bicgstab", ctx.bicgstab, "none", dict(precond=capi.PRECOND_NONE)), ("bicgstab", ctx.bicgstab, "jacobi", dict(precond=capi.PRECOND_JACOBI)),
                    ("bicgstab", ctx.bicgstab, "ilu0", dict(precond=capi.PRECOND_ILU0))]
            if not convection:
                runs = [("cg", ctx.cg, name, dict(precond=p)) for name, p in (("none", capi.PRECOND_NONE), ("jacobi", capi.PRECOND_JACOBI),
                                                                                ("symgs", capi.PRECOND_SYMGS), ("ilu0", capi.PRECOND_ILU0))] + runs
            for solver, call, name, kw in runs:
                if order == 0 and name in ("none", "jacobi"):
                    continue  # (no sweep order in them: measured once, with order 1)
                x.fill(0.0)
                ctx.sync()
                t = time.perf_counter()
                try:
                    iters, res = call(A, b, x, max_iter=MAX_ITER, rel_tol=REL_TOL, check_every=10, **kw)
                    ctx.sync()
                    rec[f"{solver}_{name}"] = dict(iters=iters, ms=round((time.perf_counter() - t) * 1e3, 2), rel_resid=float(f"{res:.3e}"))
                except capi.SpmvError as e:
                    rec[f"{solver}_{name}"] = dict(error=str(e))
                # (a sign of life per solve: in row order on 2048^2 points one of them takes minutes)
                print(f"# {shape} order {order} {solver}_{name}: {rec[f'{solver}_{name}']}", file=sys.stderr, flush=True)
            emit(rec)
        del A, b, x, z, y
    if out:
        out.close()


if __name__ == "__main__":
    main()
