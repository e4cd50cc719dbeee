#!/usr/bin/env python3
"""k conjugate-gradient solves in one loop (spmv_cg_multi) against k calls of spmv_cg on the same handle.

One JSON line per (system, preconditioner, k): the median over --rounds rounds of
  ms_multi       one cg_multi on B, X row-major (n x k);
  ms_separate    k spmv_cg on k separate vectors b_c, x_c (the same handle, its AUTO kernel, the two-launch iteration);
the two interleaved in the same process after a warm-up.  Both sides run a fixed 50 iterations (rel_tol = 0, check_every = 50) from
x = 0, which is set again before every solve and outside the timed window; a window is one whole call between two device
synchronisations, so it holds the call's own set-up (work vectors, the first residual, Jacobi's diagonal) on both sides.
us_iter_multi / us_iter_separate: the window over the 50 iterations; speedup = ms_separate / ms_multi (per column: the same number).
bytes_iter_multi: what one iteration of the k-column loop must move - the product 12*nnz + 4*(n+1) + 16*n*k, the column dots
16*n*k, the fused update 72*n*k (Jacobi: 88*n*k + 8*n); bytes_iter_separate: k times spmv_cg's 12*nnz + 4*(n+1) + 16*n + 72*n
(Jacobi: + 24*n).  frac_8tbs = bytes_iter_multi / us_iter_multi over 8 TB/s.

Systems: the 5-point Laplacian on 2048^2 points, the 7-point Laplacian on 160^3 points, and a 5-point Laplacian of 10^4 rows (100^2
points: the launch-bound end); plain and Jacobi.

  python tools/bench_cg_multi.py [--systems lap2d_2048,lap3d_160,lap2d_100] [--ks 1,4,8,16,32] [--out profiles/r09_bench_cg_multi.jsonl]
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
PEAK = 8e12
ITERS = 50


def laplacian(shape):
    """(n, row_ptr, col, val) of the 5-point (2-D) or 7-point (3-D) Laplacian on a grid, Dirichlet boundary, columns ascending"""
    n = int(np.prod(shape))
    idx = np.arange(n, dtype=np.int64).reshape(shape)
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [np.full(n, 2.0 * len(shape))]
    for ax in range(len(shape)):
        lo = np.take(idx, np.arange(shape[ax] - 1), axis=ax).ravel()
        hi = np.take(idx, np.arange(1, shape[ax]), axis=ax).ravel()
        rows += [lo, hi]
        cols += [hi, lo]
        vals += [np.full(lo.size, -1.0)] * 2
    r, c, v = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    o = np.argsort(r * n + c, kind="stable")
    r, c, v = r[o], c[o], v[o]
    rp = np.searchsorted(r, np.arange(n + 1)).astype(np.int32)
    return n, rp, c.astype(np.int32), v


SYSTEMS = {"lap2d_2048": (2048, 2048), "lap3d_160": (160, 160, 160), "lap2d_100": (100, 100)}


def window(ctx, prepare, fn) -> float:
    prepare()
    ctx.sync()
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--systems", default="lap2d_2048,lap3d_160,lap2d_100")
    ap.add_argument("--ks", default="1,4,8,16,32")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    ks = [int(s) for s in a.ks.split(",")]
    ctx = capi.Context(0)
    out = open(a.out, "a") if a.out else None
    for system in a.systems.split(","):
        n, rp, cc, cv = laplacian(SYSTEMS[system])
        nnz = int(cc.size)
        A = ctx.csr(n, n, rp, cc, cv)
        kmax = max(ks)
        bs = [ctx.gen_vector(n, seed=100 + c) for c in range(kmax)]
        xs = [ctx.vector(n) for _ in range(kmax)]
        for jacobi in (False, True):
            for k in ks:
                B = ctx.gen_vector(n * k, seed=7)
                X = ctx.vector(n * k)

                def multi():
                    iters, _ = ctx.cg_multi(A, B, X, k, max_iter=ITERS, rel_tol=0.0, check_every=ITERS, jacobi=jacobi)
                    assert np.all(iters == ITERS), iters

                def separate():
                    for c in range(k):
                        it, _ = ctx.cg(A, bs[c], xs[c], max_iter=ITERS, rel_tol=0.0, check_every=ITERS, jacobi=jacobi)
                        assert it == ITERS, it

                def zero_multi():
                    X.fill(0.0)

                def zero_separate():
                    for c in range(k):
                        xs[c].fill(0.0)

                window(ctx, zero_multi, multi)  # warm-up
                window(ctx, zero_separate, separate)
                ms_m, ms_s = [], []
                for _ in range(a.rounds):
                    ms_m.append(window(ctx, zero_multi, multi))
                    ms_s.append(window(ctx, zero_separate, separate))
                m, s = float(np.median(ms_m)), float(np.median(ms_s))
                mat = 12 * nnz + 4 * (n + 1)
                bytes_m = mat + (16 + 16 + (88 if jacobi else 72)) * n * k + (8 * n if jacobi else 0)
                bytes_s = k * (mat + (16 + 72 + (24 if jacobi else 0)) * n)
                rec = dict(system=system, n=n, nnz=nnz, precond="jacobi" if jacobi else "none", k=k, iters=ITERS,
                           auto_kernel=int(A.info.kernel), ms_multi=round(m, 4), ms_separate=round(s, 4), speedup=round(s / m, 3),
                           us_iter_multi=round(m * 1e3 / ITERS, 2), us_iter_separate=round(s * 1e3 / ITERS, 2),
                           bytes_iter_multi=int(bytes_m), bytes_iter_separate=int(bytes_s),
                           frac_8tbs=round(bytes_m / (m * 1e-3 / ITERS) / PEAK, 4),
                           rounds_multi=[round(v, 4) for v in ms_m], rounds_separate=[round(v, 4) for v in ms_s])
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
                del B, X
        del A, bs, xs
    if out:
        out.close()


if __name__ == "__main__":
    main()
