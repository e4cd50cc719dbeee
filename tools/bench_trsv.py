#!/usr/bin/env python3
"""Triangular solves with a caller's matrix (spmv_trsv_solve / spmv_trsv_solve_multi) measured on the ILU(0) factors of the 160^3
Laplacian, by the method of tools/bench_ilu0.py: interleaved windows of REPS calls between two device synchronisations, medians of
`--rounds` rounds (one more warms up).

One JSON line per sweep order (0 the matrix's own row order, 1 multicolour).  The factors come from spmv_ilu0_factors of the handle
in that order; for the multicolour order the matrix is permuted symmetrically into sweep order first, so that ILU(0) in that order
IS the row-order factorisation of the permuted matrix and its combined LU array splits by row and column index.

  ms_lower_unit, ms_upper   one spmv_trsv_solve with TRSV_LOWER | TRSV_UNIT and with TRSV_UPPER over the combined LU array
  ms_ilu0                   one spmv_ilu0_solve (both triangles) on the handle the factors came from
  ms_apply                  one spmv_apply of that handle
  trsv_over_ilu0            (ms_lower_unit + ms_upper) / ms_ilu0
  levels, lanes, launches   per triangle, from spmv_trsv_info
  multi                     per k in 1, 4, 8, 16, 32: ms of one spmv_trsv_solve_multi (lower unit), its launches, and
                            k_singles_over_multi = k * ms_lower_unit / ms: above 1, the k columns at once win
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
from bench_ilu0 import capi, stencil  # noqa: E402

REPS = 10
KS = (1, 4, 8, 16, 32)
LOWER_UNIT, UPPER = capi.TRSV_LOWER | capi.TRSV_UNIT, capi.TRSV_UPPER


def permuted(n, rp, cc, cv, seq):
    """P A P^T with row k of the result row seq[k] of A; columns renumbered, the order inside a row kept"""
    pos = np.empty(n, np.int64)
    pos[seq] = np.arange(n)
    cnt = np.diff(rp)[seq]
    rp2 = np.concatenate([[0], np.cumsum(cnt)])
    src = np.repeat(rp[:-1][seq] - rp2[:-1], cnt) + np.arange(rp2[-1])
    return rp2.astype(np.int32), pos[cc[src]].astype(np.int32), cv[src]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", type=int, default=160)
    ap.add_argument("--orders", default="0,1")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    ctx = capi.Context(0)
    out = open(a.out, "a") if a.out else None

    def window(op):
        ctx.sync()
        t = time.perf_counter()
        for _ in range(REPS):
            op()
        ctx.sync()
        return (time.perf_counter() - t) * 1e3 / REPS

    n, rp, cc, cv = stencil(a.grid, 3, False)
    for order in (int(s) for s in a.orders.split(",")):
        if order:
            A0 = ctx.csr(n, n, rp, cc, cv)
            A0.set_param("ilu0_order", 1)
            rp_o, cc_o, cv_o = permuted(n, rp, cc, cv, ctx.ilu0_order(A0).astype(np.int64))
            del A0
        else:
            rp_o, cc_o, cv_o = rp, cc, cv
        A = ctx.csr(n, n, rp_o, cc_o, cv_o)
        A.set_param("ilu0_order", 0)  # (of the permuted matrix: the multicolour sweep)
        F = ctx.csr(n, n, rp_o, cc_o, ctx.ilu0_factors(A))
        for flags in (LOWER_UNIT, UPPER):
            ctx.trsv_setup(F, flags)
        info = {"lower_unit": ctx.trsv_info(F, LOWER_UNIT), "upper": ctx.trsv_info(F, UPPER)}
        b, x, z, y = ctx.gen_vector(n, seed=5), ctx.vector(n), ctx.vector(n), ctx.vector(n)
        y.fill(0.0)
        vec = {k: (ctx.gen_vector(n * k, seed=6), ctx.vector(n * k)) for k in KS}
        ops = {"lower_unit": lambda: ctx.trsv_solve(F, b, x, LOWER_UNIT), "upper": lambda: ctx.trsv_solve(F, b, x, UPPER),
               "ilu0": lambda: ctx.ilu0_solve(A, b, z), "apply": lambda: ctx.apply(A, b, y)}
        for k in KS:
            ops[f"multi_{k}"] = lambda k=k: ctx.trsv_solve_multi(F, vec[k][0], vec[k][1], k, LOWER_UNIT)
        ms = {name: [] for name in ops}
        for rnd in range(a.rounds + 1):  # round 0 warms up; interleaved
            for name, op in ops.items():
                t = window(op)
                if rnd:
                    ms[name].append(t)
        med = {name: float(np.median(v)) for name, v in ms.items()}
        rec = dict(bench="trsv", grid=a.grid, nrow=n, nnz=int(A.info.nnz), order=order, reps=REPS, rounds=a.rounds,
                   ms_lower_unit=round(med["lower_unit"], 4), ms_upper=round(med["upper"], 4), ms_ilu0=round(med["ilu0"], 4),
                   ms_apply=round(med["apply"], 4), trsv_over_ilu0=round((med["lower_unit"] + med["upper"]) / med["ilu0"], 3),
                   ilu0_launches=int(A.get_param("ilu0_launches")), info=info, multi={})
        for k in KS:
            ctx.trsv_solve_multi(F, vec[k][0], vec[k][1], k, LOWER_UNIT)
            rec["multi"][str(k)] = dict(ms=round(med[f"multi_{k}"], 4), launches=int(F.get_param("trsv_multi_launches")),
                                        level_launches=int(F.get_param("trsv_multi_level_launches")),
                                        k_singles_over_multi=round(k * med["lower_unit"] / med[f"multi_{k}"], 2))
        ctx.sync()
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        del A, F, b, x, z, y, vec
    # the case of tests/test_gpu_trsv_perf.py: the Laplacian's own lower triangle on a 64^3 grid, 190 levels, k = 8 against 8 solves
    n, rp, cc, cv = stencil(64, 3, False)
    A = ctx.csr(n, n, rp, cc, cv)
    ctx.trsv_setup(A, capi.TRSV_LOWER)
    b, x, B, X = ctx.gen_vector(n, seed=5), ctx.vector(n), ctx.gen_vector(n * 8, seed=6), ctx.vector(n * 8)
    ops = {"single": lambda: ctx.trsv_solve(A, b, x, capi.TRSV_LOWER), "multi_8": lambda: ctx.trsv_solve_multi(A, B, X, 8, capi.TRSV_LOWER)}
    ms = {name: [] for name in ops}
    for rnd in range(a.rounds + 1):
        for name, op in ops.items():
            t = window(op)
            if rnd:
                ms[name].append(t)
    med = {name: float(np.median(v)) for name, v in ms.items()}
    line = json.dumps(dict(bench="trsv_lap64_lower", nrow=n, info=ctx.trsv_info(A, capi.TRSV_LOWER), ms_single=round(med["single"], 4),
                           ms_multi_8=round(med["multi_8"], 4), multi_launches=int(A.get_param("trsv_multi_launches")),
                           eight_singles_over_multi=round(8 * med["single"] / med["multi_8"], 2)))
    print(line, flush=True)
    if out:
        out.write(line + "\n")


if __name__ == "__main__":
    main()
