#!/usr/bin/env python3
"""The transposed product y += A^T x (spmv_apply_transpose) against the forward product y += A x of the same handle.

One JSON line per workload:
  ms_forward     spmv_apply with the handle's AUTO kernel;
  ms_transpose   spmv_apply_transpose (the companion's AUTO kernel, or the DIA transposed kernel);
  setup_s        spmv_mat_transpose_setup, wall clock (synchronous; the companion's analysis and trial included);
  transpose_bytes, transpose_kernel: what the transposed state holds and which kernel its companion's AUTO picked
                 (kernel ids of include/spmv_abi.h; for a DIA handle 1 = the transposed DIA kernel); transpose_rowgrouped_kernel:
                 the CSR kernel of the companion's row-grouped copy where it runs from one (kernel 4), else 0;
the two products interleaved in rounds after a warm-up, each round a window of `reps` products timed by the host clock between two
device synchronisations; the medians are reported.  bytes_alg: the bytes one product must move (matrix arrays once, x read, y
read and written), so frac_8tbs_* = bytes_alg / ms over 8 TB/s.

Workloads: c2 (10M x 32 uniform columns), band (the same, columns in a band of 65536), c3_ell (ELL 4M x 64 circulant band),
c4_coo (COO 2M x 2M power-law rows up to 4096), dia (DIA 4M x 64 band), csc (CSC 2M x 2M, 32 uniform rows per column).

  python tools/bench_transpose.py [--workloads c2,band,c3_ell,c4_coo,dia,csc] [--out profiles/r08_bench_transpose.jsonl]
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
PEAK = 8e12


def make(ctx, name):
    """(handle, matrix bytes read once by a product)"""
    if name in ("c2", "band"):
        n = 10_000_000
        return ctx.gen_csr_uniform(0, n, n, 32, 65536 if name == "band" else 0, seed=3), 12 * n * 32 + 4 * (n + 1)
    if name == "c3_ell":
        n = 4_000_000
        return ctx.gen_ell_banded(n, n, 64, seed=3), 12 * n * 64
    if name == "c4_coo":
        A = ctx.gen_coo_powerlaw(2_000_000, 2_000_000, 4096, seed=3)
        return A, 16 * int(A.info.nnz)
    if name == "dia":
        n = 4_000_000
        return ctx.gen_dia_banded(n, 64, seed=3), 8 * n * 64 + 4 * 64
    if name == "csc":
        n = 2_000_000
        cp, ri, v = pkg.synth.csr_uniform(0, n, n, 32, seed=3)  # (the CSR arrays of a matrix read as the CSC arrays of another)
        return ctx.csc(n, n, cp, ri, v), 12 * n * 32 + 4 * (n + 1)
    raise SystemExit(f"unknown workload {name}")


def window(ctx, fn, reps) -> float:
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="c2,band,c3_ell,c4_coo,dia,csc")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r08_bench_transpose.jsonl"), help="JSON lines are appended here too")
    a = ap.parse_args()
    ctx = capi.Context(0)
    out = open(a.out, "a") if a.out else None
    for name in a.workloads.split(","):
        A, mat_bytes = make(ctx, name)
        info = A.info
        nrow, ncol = int(info.nrow), int(info.ncol)
        x, y = ctx.gen_vector(ncol, seed=5), ctx.vector(nrow)
        xt, yt = ctx.gen_vector(nrow, seed=6), ctx.vector(ncol)
        y.fill(0.0)
        yt.fill(0.0)
        ctx.sync()
        t0 = time.perf_counter()
        A.transpose_setup()
        setup_s = time.perf_counter() - t0
        fwd = lambda: ctx.apply(A, x, y)  # noqa: E731
        tr = lambda: ctx.apply_transpose(A, xt, yt)  # noqa: E731
        t_f = max(window(ctx, fwd, 1), window(ctx, fwd, 1))  # warm-up
        t_t = max(window(ctx, tr, 1), window(ctx, tr, 1))
        reps_f = max(1, min(200, int(50 / max(t_f, 1e-3))))
        reps_t = max(1, min(200, int(50 / max(t_t, 1e-3))))
        ms_f, ms_t = [], []
        for _ in range(a.rounds):
            ms_f.append(window(ctx, fwd, reps_f))
            ms_t.append(window(ctx, tr, reps_t))
        mf, mt = float(np.median(ms_f)), float(np.median(ms_t))
        bytes_alg = mat_bytes + 8 * max(nrow, ncol) + 16 * max(nrow, ncol)
        rec = dict(workload=name, format=int(info.format), nrow=nrow, ncol=ncol, nnz=int(info.nnz), forward_kernel=int(info.kernel),
                   transpose_kernel=A.get_param("transpose_kernel"),
                   transpose_rowgrouped_kernel=A.get_param("transpose_rowgrouped_kernel"), transpose_bytes=A.get_param("transpose_bytes"),
                   device_bytes=int(info.device_bytes), setup_s=round(setup_s, 3), ms_forward=round(mf, 4), ms_transpose=round(mt, 4),
                   ratio=round(mt / mf, 3), bytes_alg=int(bytes_alg), frac_8tbs_forward=round(bytes_alg / (mf * 1e-3) / PEAK, 4),
                   frac_8tbs_transpose=round(bytes_alg / (mt * 1e-3) / PEAK, 4), rounds_forward=[round(v, 4) for v in ms_f],
                   rounds_transpose=[round(v, 4) for v in ms_t])
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        del A, x, y, xt, yt
    if out:
        out.close()


if __name__ == "__main__":
    main()
