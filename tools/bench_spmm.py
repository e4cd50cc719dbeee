#!/usr/bin/env python3
"""Y += A*X for k vectors at once (spmv_apply_multi) against k separate spmv_apply calls of the handle's AUTO kernel.

One JSON line per (shape, k): the median over --rounds rounds of
  ms_multi       one apply_multi (X, Y row-major, ncol x k and nrow x k);
  ms_separate    k spmv_apply on k separate vectors x_c, y_c (the same handle, its AUTO kernel);
the two interleaved in the same process after a warm-up, each round a window of `reps` products timed by the host clock between
two device synchronisations.  bytes_alg = 12*nnz + 4*(nrow+1) + 8*ncol*k + 16*nrow*k (ELL: 12*nrow*slots instead of the CSR
arrays), the bytes one product must move; bytes_tile_rereads = the matrix arrays once more per extra column tile (counted apart:
they may come from the caches); frac_8tbs = bytes_alg / ms_multi over 8 TB/s.  `lanes` / `tiles`: the kernel variant
(kernels_spmm.hip: T lanes per row, ceil(k / T) column tiles).  --lanes-ab adds rows for k = 32 with 32-lane groups (one tile)
next to the default 16-lane groups (two tiles), from a child process with SPMV_SPMM_LANES=32 (the engine reads that A/B switch
once per process), after the parent's rows.

  python tools/bench_spmm.py [--shapes band,uniform,square1M,ell_c3,arrow] [--ks 1,2,4,8,16,32] [--out FILE]
Needs a GPU; there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from __graft_entry__ import load_package  # noqa: E402

capi = load_package().capi
PEAK = 8e12


def arrow(n):
    """diagonal + a dense first row + a dense first column (tools/sweep_structures.py: arrow): one row of n entries"""
    i = np.arange(n, dtype=np.int64)
    r = np.concatenate((i, np.zeros(n - 1, np.int64), i[1:]))
    c = np.concatenate((i, i[1:], np.zeros(n - 1, np.int64)))
    key = np.unique(r * n + c)
    r, c = key // n, (key % n).astype(np.int32)
    rp = np.searchsorted(r, np.arange(n + 1)).astype(np.int32)
    v = np.random.default_rng(9).uniform(-1.0, 1.0, c.size)
    return rp, c, v


def make(ctx, shape):
    """(handle, nrow, ncol, matrix bytes read once: value + index arrays and row offsets)"""
    if shape == "band":  # 10M x 32, columns uniform in a band of 65536 around the diagonal
        n = 10_000_000
        return ctx.gen_csr_uniform(0, n, n, 32, 65536, seed=3), n, n, 12 * n * 32 + 4 * (n + 1)
    if shape == "uniform":  # C2: 10M x 32, uniform columns
        n = 10_000_000
        return ctx.gen_csr_uniform(0, n, n, 32, 0, seed=3), n, n, 12 * n * 32 + 4 * (n + 1)
    if shape == "square1M":  # 1M x 1M, 32 uniform columns per row
        n = 1_000_000
        return ctx.gen_csr_uniform(0, n, n, 32, 0, seed=3), n, n, 12 * n * 32 + 4 * (n + 1)
    if shape == "ell_c3":  # C3: ELL 4M x 64, circulant band
        n = 4_000_000
        return ctx.gen_ell_banded(n, n, 64, seed=3), n, n, 12 * n * 64
    if shape == "arrow":  # 1M rows, row 0 holds 1M entries
        n = 1_000_000
        rp, c, v = arrow(n)
        return ctx.csr(n, n, rp, c, v), n, n, 12 * c.size + 4 * (n + 1)
    raise SystemExit(f"unknown shape {shape}")


def lanes_for(k: int) -> int:
    """the kernel's rule (kernels_spmm.hip: spmm_lanes): the next power of two >= k, capped at 16, or at SPMV_SPMM_LANES = 32 / 64"""
    cap = {"32": 32, "64": 64}.get(os.environ.get("SPMV_SPMM_LANES", ""), 16)
    t = 1
    while t < k and t < cap:
        t *= 2
    return t


def window(ctx, fn, reps) -> float:
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3 / reps


def measure(ctx, A, nrow, ncol, k, rounds, xs, ys, X, Y):
    multi = lambda: ctx.apply_multi(A, X, Y, k)  # noqa: E731

    def separate():
        for c in range(k):
            ctx.apply(A, xs[c], ys[c])

    # warm-up, and reps for windows of ~50 ms (one product at least)
    t_m = max(window(ctx, multi, 1), window(ctx, multi, 1))
    t_s = max(window(ctx, separate, 1), window(ctx, separate, 1))
    reps_m = max(1, min(200, int(50 / max(t_m, 1e-3))))
    reps_s = max(1, min(200, int(50 / max(t_s, 1e-3))))
    ms_m, ms_s = [], []
    for _ in range(rounds):
        ms_m.append(window(ctx, multi, reps_m))
        ms_s.append(window(ctx, separate, reps_s))
    return float(np.median(ms_m)), float(np.median(ms_s)), ms_m, ms_s


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="band,uniform,square1M,ell_c3,arrow")
    ap.add_argument("--ks", default="1,2,4,8,16,32")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lanes-ab", action="store_true", help="k = 32 also with 32-lane groups (SPMV_SPMM_LANES=32)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    ks = [int(s) for s in a.ks.split(",")]
    ctx = capi.Context(0)
    out = open(a.out, "a") if a.out else None
    for shape in a.shapes.split(","):
        A, nrow, ncol, mat_bytes = make(ctx, shape)
        info = A.info
        kmax = max(ks)
        xs = [ctx.gen_vector(ncol, seed=100 + c) for c in range(kmax)]
        ys = [ctx.vector(nrow) for _ in range(kmax)]
        for y in ys:
            y.fill(0.0)
        for k in ks:
            X = ctx.gen_vector(ncol * k, seed=7)
            Y = ctx.vector(nrow * k)
            Y.fill(0.0)
            lanes = lanes_for(k)
            tiles = -(-k // lanes)
            ms_m, ms_s, all_m, all_s = measure(ctx, A, nrow, ncol, k, a.rounds, xs, ys, X, Y)
            bytes_alg = mat_bytes + 8 * ncol * k + 16 * nrow * k
            rec = dict(shape=shape, k=k, nrow=nrow, ncol=ncol, nnz=int(info.nnz), format=int(info.format),
                       auto_kernel=int(info.kernel), lanes=lanes, tiles=tiles, ms_multi=round(ms_m, 4),
                       ms_separate=round(ms_s, 4), speedup=round(ms_s / ms_m, 3), bytes_alg=int(bytes_alg),
                       bytes_tile_rereads=int((tiles - 1) * mat_bytes), frac_8tbs=round(bytes_alg / (ms_m * 1e-3) / PEAK, 4),
                       rounds_multi=[round(v, 4) for v in all_m], rounds_separate=[round(v, 4) for v in all_s])
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
            del X, Y
        del A, xs, ys
    if out:
        out.close()
    if a.lanes_ab and 32 in ks and os.environ.get("SPMV_SPMM_LANES") is None:
        # the engine reads SPMV_SPMM_LANES once per process: k = 32 with 32-lane groups is measured by a child of its own
        del ctx
        cmd = [sys.executable, __file__, "--shapes", a.shapes, "--ks", "32", "--rounds", str(a.rounds)]
        if a.out:
            cmd += ["--out", a.out]
        subprocess.run(cmd, env=dict(os.environ, SPMV_SPMM_LANES="32"), check=True)


if __name__ == "__main__":
    main()
