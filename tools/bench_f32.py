#!/usr/bin/env python3
"""Single-precision value storage (format 6) against fp64 CSR: the product, and refinement against plain conjugate gradients.

One JSON line per workload.  Products (`kind: "apply"`):
  ms_f32, ms_csr_auto, ms_csr_vector   spmv_apply of the format-6 handle, of the CSR AUTO handle of the same matrix and of a CSR
                    handle forced to VECTOR at the format-6 handle's lanes, interleaved in rounds after a warm-up, each round a
                    window of `reps` products timed by the host clock between two device synchronisations; the medians of 3 rounds;
  ratio_auto, ratio_vector   ms_csr_* / ms_f32 (above 1: format 6 is faster);
  gbs_*             bytes_alg / ms: 8 (format 6) or 12 (CSR) bytes per entry and the row pointer, plus x read once and y read and written;
  ms_by_lanes       the format-6 product under every lane count;
  f32_info          what the rounding did (inexact, underflow, max_rel_err); setup_csr_to_f32_s: the conversion, wall clock.
Solves (`kind: "solve"`, the two Laplacians scaled D L D with D = diag(uniform(0.5, 2))): spmv_refine (inner CG on the format-6
handle, inner tolerance 1e-4) against spmv_cg on the fp64 handle, both to 1e-10, interleaved, medians of 3 rounds: the seconds,
the outer steps and inner iterations, the iterations of plain CG, the residuals both report.  A solve that ends in an error (the
rounded matrix of an ill-conditioned system need not be positive definite) is recorded with the error's text.

Workloads: lap2d (5-point, 2048^2), lap3d (7-point, 160^3), grid27 (27-point, 100^3), band (10M x 32 in a band of 65536), uniform
(10M x 32, uniform-random columns).  --scale divides the rows (the grids' edge by its root) for a quick look.

  python tools/bench_f32.py [--workloads lap2d,lap3d,grid27,band,uniform] [--out profiles/r22_bench_f32.jsonl]
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

pkg = load_package()
capi = pkg.capi
VECTOR = 1
LANES = (1, 2, 4, 8, 16, 32, 64)


def stencil(name, scale):
    """(n, row_ptr, col, val, spd) of a grid pattern with columns ascending; the Laplacians scaled D L D"""
    dim = 2 if name == "lap2d" else 3
    edge = max(4, int(round((2048 if dim == 2 else (160 if name == "lap3d" else 100)) / scale ** (1.0 / dim))))
    idx = np.indices((edge,) * dim).reshape(dim, -1)
    if name == "grid27":
        steps = [tuple(np.array(s) - 1) for s in np.ndindex((3,) * dim)]
    else:
        steps = [tuple(0 for _ in range(dim))] + [tuple(sgn if a == d else 0 for a in range(dim)) for d in range(dim) for sgn in (-1, 1)]
    n = edge**dim
    cols, ok, centre = [], [], []
    for s in steps:
        nb = idx + np.array(s)[:, None]
        ok.append(np.all((nb >= 0) & (nb < edge), axis=0))
        cols.append(np.ravel_multi_index(np.clip(nb, 0, edge - 1), (edge,) * dim))
        centre.append(np.full(n, all(v == 0 for v in s)))
    cols, ok, centre = np.stack(cols, axis=1), np.stack(ok, axis=1), np.stack(centre, axis=1)
    big = np.iinfo(np.int64).max
    key = np.where(ok, cols, big)
    order = np.argsort(key, axis=1, kind="stable")
    key = np.take_along_axis(key, order, axis=1)
    centre = np.take_along_axis(centre, order, axis=1)
    keep = key != big
    col = key[keep].astype(np.int32)
    rp = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32)
    rows = np.repeat(np.arange(n), np.diff(rp))
    rng = np.random.default_rng(7)
    if name == "grid27":
        val = rng.uniform(0.5, 1.5, size=len(col))
        return n, rp, col, val, False
    d = rng.uniform(0.5, 2.0, size=n)
    val = np.where(centre[keep], 2.0 * dim, -1.0) * d[rows] * d[col]
    return n, rp, col, val, True


def window(ctx, fn, reps) -> float:
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3 / reps


def bench_apply(ctx, name, n, C, V, L, rounds):
    nnz = int(L.info.nnz)
    lanes = int(L.info.lanes_per_row)
    V.set_kernel(VECTOR, lanes)
    x, yl, yc, yv = ctx.gen_vector(n, seed=5), ctx.vector(n), ctx.vector(n), ctx.vector(n)
    for y in (yl, yc, yv):
        y.fill(0.0)
    fns = dict(f32=lambda: ctx.apply(L, x, yl), csr_auto=lambda: ctx.apply(C, x, yc), csr_vector=lambda: ctx.apply(V, x, yv))
    reps = {}
    for k, f in fns.items():
        t = max(window(ctx, f, 1), window(ctx, f, 1))  # warm-up
        reps[k] = max(1, min(200, int(50 / max(t, 1e-3))))
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            ms[k].append(window(ctx, f, reps[k]))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    by_lanes = {}
    for l in LANES:
        L.set_kernel(VECTOR, l)
        window(ctx, fns["f32"], 1)
        by_lanes[str(l)] = round(window(ctx, fns["f32"], reps["f32"]), 4)
    L.set_kernel(VECTOR, lanes)
    bytes_f32 = nnz * 8 + 4 * (n + 1) + 8 * n + 16 * n
    bytes_csr = nnz * 12 + 4 * (n + 1) + 8 * n + 16 * n
    inexact, under, rel = L.f32_info()
    return dict(kind="apply", workload=name, nrow=n, nnz=nnz, lanes_per_row=lanes, csr_auto_kernel=int(C.info.kernel), ms_f32=round(med["f32"], 4),
                ms_csr_auto=round(med["csr_auto"], 4), ms_csr_vector=round(med["csr_vector"], 4), ratio_auto=round(med["csr_auto"] / med["f32"], 3),
                ratio_vector=round(med["csr_vector"] / med["f32"], 3), bytes_f32=int(bytes_f32), bytes_csr=int(bytes_csr),
                gbs_f32=round(bytes_f32 / med["f32"] / 1e6, 1), gbs_csr_auto=round(bytes_csr / med["csr_auto"] / 1e6, 1),
                gbs_csr_vector=round(bytes_csr / med["csr_vector"] / 1e6, 1), ms_by_lanes=by_lanes, f32_info=[inexact, under, rel],
                rounds={k: [round(t, 4) for t in v] for k, v in ms.items()})


def bench_solve(ctx, name, n, C, L, rounds, max_iter):
    b = ctx.gen_vector(n, seed=9)

    def timed(fn):
        x = ctx.vector(n)
        x.fill(0.0)
        ctx.sync()
        t0 = time.perf_counter()
        try:
            out = fn(x)
        except capi.SpmvError as err:
            out = str(err)
        ctx.sync()
        return time.perf_counter() - t0, out

    refine = lambda x: ctx.refine(C, L, b, x, solver=capi.REFINE_CG, max_outer=30, inner_max_iter=max_iter, inner_tol=1e-4, rel_tol=1e-10)  # noqa: E731
    plain = lambda x: ctx.cg(C, b, x, max_iter=max_iter, rel_tol=1e-10)  # noqa: E731
    timed(lambda x: ctx.refine(C, L, b, x, max_outer=1, inner_max_iter=5))  # warm-up
    timed(lambda x: ctx.cg(C, b, x, max_iter=5))
    t_r, t_c, out_r, out_c = [], [], None, None
    for _ in range(rounds):
        t, out_r = timed(refine)
        t_r.append(t)
        t, out_c = timed(plain)
        t_c.append(t)
    rec = dict(kind="solve", workload=name, nrow=n, nnz=int(L.info.nnz), rel_tol=1e-10, inner_tol=1e-4, s_refine=round(float(np.median(t_r)), 4),
               s_cg=round(float(np.median(t_c)), 4), ratio=round(float(np.median(t_c)) / float(np.median(t_r)), 3), csr_kernel=int(C.info.kernel),
               rounds_refine=[round(t, 4) for t in t_r], rounds_cg=[round(t, 4) for t in t_c])
    if isinstance(out_r, str):
        rec["refine_error"] = out_r
    else:
        rec.update(outer=out_r[0], inner_total=out_r[1], resid_refine=out_r[2])
    if isinstance(out_c, str):
        rec["cg_error"] = out_c
    else:
        rec.update(cg_iters=out_c[0], resid_cg=out_c[1])
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="lap2d,lap3d,grid27,band,uniform")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--max-iter", type=int, default=20000, help="iterations of plain CG and of every inner solve, at the most")
    ap.add_argument("--no-solve", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r22_bench_f32.jsonl"), help="JSON lines are appended here too")
    a = ap.parse_args()
    ctx = capi.Context(0)
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for name in a.workloads.split(","):
        spd = False
        if name in ("band", "uniform"):
            n = 10_000_000 // a.scale
            make = lambda: ctx.gen_csr_uniform(0, n, n, 32, band=65536 if name == "band" else 0, seed=3)  # noqa: E731
        elif name in ("lap2d", "lap3d", "grid27"):
            n, rp, col, val, spd = stencil(name, a.scale)
            make = lambda: ctx.csr(n, n, rp, col, val)  # noqa: E731
        else:
            raise SystemExit(f"unknown workload {name}")
        C, V = make(), make()
        ctx.sync()
        t0 = time.perf_counter()
        L = ctx.csr_to_f32(C)
        ctx.sync()
        to_f32_s = time.perf_counter() - t0
        rec = bench_apply(ctx, name, n, C, V, L, a.rounds)
        rec["setup_csr_to_f32_s"] = round(to_f32_s, 3)
        emit(rec)
        del V
        if spd and not a.no_solve:
            emit(bench_solve(ctx, name, n, C, L, a.rounds, a.max_iter))
        del C, L
    if out:
        out.close()


if __name__ == "__main__":
    main()
