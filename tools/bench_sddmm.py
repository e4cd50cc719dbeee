#!/usr/bin/env python3
"""The sampled dense-dense product (spmv_sddmm) against the bytes it must move and against torch's gather formulation.

One JSON line per (shape, k, beta): the median over --rounds rounds of
  ms_sddmm    one spmv_sddmm, out = U V^T sampled on the pattern (+ beta * out);
  ms_torch    (U[rows] * V[cols]).sum(1) (+ beta * out) on the same tensors, which materialises two nnz x k gathers (null where
              torch runs out of memory);
  ms_spmm     on the arrow shape only: spmv_apply_multi of the same handle at the same k, whose long row is one serial chain;
interleaved in the same process after a warm-up, each round a window of `reps` calls timed by the host clock between two device
synchronisations.  bytes_alg = 4 nnz + 4 (nrow + 1) + 8 nnz (16 nnz with beta != 0) + 8 nrow k + 8 ncol k, the bytes one call must
move; frac_8tbs = bytes_alg / ms_sddmm over 8 TB/s.  `lanes`: the lanes that make one entry (sddmm_settings.hpp: the next power of two
>= k).

  python tools/bench_sddmm.py [--shapes uniform,band,laplace2048,arrow] [--ks 1,8,16,64] [--betas 0,1] [--out FILE]
Needs a GPU; there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
torch.zeros(1, device=dev)  # torch initialises its HIP runtime before the engine's library is loaded (as bench.py does)

import numpy as np  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from __graft_entry__ import load_package  # noqa: E402

capi = load_package().capi
PEAK = 8e12
DEFAULT_OUT = ROOT / "profiles" / "r25_bench_sddmm.jsonl"


def arrow(n):
    """diagonal + a dense first row + a dense first column (tools/bench_spmm.py: arrow): one row of n entries"""
    i = np.arange(n, dtype=np.int64)
    r = np.concatenate((i, np.zeros(n - 1, np.int64), i[1:]))
    c = np.concatenate((i, i[1:], np.zeros(n - 1, np.int64)))
    key = np.unique(r * n + c)
    r, c = key // n, (key % n).astype(np.int32)
    return np.searchsorted(r, np.arange(n + 1)).astype(np.int32), c


def laplace(side):
    """the 5-point stencil on a side x side grid"""
    i = np.arange(side * side, dtype=np.int64)
    x, y = i % side, i // side
    cand = np.stack([i - side, i - 1, i, i + 1, i + side], axis=1)
    ok = np.stack([y > 0, x > 0, np.ones_like(x, bool), x < side - 1, y < side - 1], axis=1)
    rp = np.zeros(side * side + 1, np.int32)
    rp[1:] = np.cumsum(ok.sum(axis=1))
    return rp, cand[ok].astype(np.int32)


def make(ctx, shape):
    """(handle, nrow, ncol)"""
    if shape == "uniform":  # 10M x 32, uniform columns
        n = 10_000_000
        return ctx.gen_csr_uniform(0, n, n, 32, 0, seed=3), n, n
    if shape == "band":  # 10M x 32, columns uniform in a band of 65536 around the diagonal
        n = 10_000_000
        return ctx.gen_csr_uniform(0, n, n, 32, 65536, seed=3), n, n
    if shape == "laplace2048":
        n = 2048 * 2048
        rp, c = laplace(2048)
        return ctx.csr(n, n, rp, c, np.ones(c.size)), n, n
    if shape == "arrow":  # 1M rows, row 0 holds 1M entries
        n = 1_000_000
        rp, c = arrow(n)
        return ctx.csr(n, n, rp, c, np.ones(c.size)), n, n
    raise SystemExit(f"unknown shape {shape}")


def lanes_for(k: int) -> int:
    t = 1
    while t < k:
        t *= 2
    return t


def window(fn, reps) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def reps_for(ms: float) -> int:
    return max(1, min(200, int(50 / max(ms, 1e-3))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="uniform,band,laplace2048,arrow")
    ap.add_argument("--ks", default="1,8,16,64")
    ap.add_argument("--betas", default="0,1")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=str(DEFAULT_OUT), help="the JSON lines are appended to this file")
    a = ap.parse_args()
    ks = [int(s) for s in a.ks.split(",")]
    betas = [float(s) for s in a.betas.split(",")]
    ctx = capi.Context(0, stream=torch.cuda.current_stream(0).cuda_stream)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    out = open(a.out, "a")
    for shape in a.shapes.split(","):
        A, nrow, ncol = make(ctx, shape)
        info = A.info
        nnz = int(info.nnz)
        rp, col, _ = A.download()
        rows = torch.repeat_interleave(torch.arange(nrow, device=dev), torch.from_numpy(np.diff(rp).astype(np.int64)).to(dev))
        cols = torch.from_numpy(col.astype(np.int64)).to(dev)
        del rp, col
        for k in ks:
            g = torch.Generator(device=dev).manual_seed(7 + k)
            U = torch.rand((nrow, k), dtype=torch.float64, device=dev, generator=g)
            V = torch.rand((ncol, k), dtype=torch.float64, device=dev, generator=g)
            res = torch.rand(nnz, dtype=torch.float64, device=dev, generator=g)
            vU, vV, vO = ctx.wrap_vector(U), ctx.wrap_vector(V), ctx.wrap_vector(res)
            for beta in betas:
                ours = lambda: ctx.sddmm(A, vU, vV, k, vO, alpha=1.0, beta=beta)  # noqa: E731

                def theirs():
                    r = (U[rows] * V[cols]).sum(1)
                    return r if beta == 0.0 else r + beta * res

                t_o = max(window(ours, 1), window(ours, 1))
                try:
                    t_t = max(window(theirs, 1), window(theirs, 1))
                except torch.OutOfMemoryError:
                    t_t = None
                    torch.cuda.empty_cache()
                ms_o, ms_t = [], []
                for _ in range(a.rounds):
                    ms_o.append(window(ours, reps_for(t_o)))
                    if t_t is not None:
                        ms_t.append(window(theirs, reps_for(t_t)))
                m_o = float(np.median(ms_o))
                m_t = float(np.median(ms_t)) if ms_t else None
                bytes_alg = 4 * nnz + 4 * (nrow + 1) + (8 if beta == 0.0 else 16) * nnz + 8 * nrow * k + 8 * ncol * k
                rec = dict(shape=shape, k=k, beta=beta, nrow=nrow, ncol=ncol, nnz=nnz, lanes=lanes_for(k), ms_sddmm=round(m_o, 4),
                           ms_torch=None if m_t is None else round(m_t, 4), speedup_vs_torch=None if m_t is None else round(m_t / m_o, 3),
                           bytes_alg=int(bytes_alg), ms_at_8tbs=round(bytes_alg / PEAK * 1e3, 4),
                           frac_8tbs=round(bytes_alg / (m_o * 1e-3) / PEAK, 4), rounds_sddmm=[round(v, 4) for v in ms_o],
                           rounds_torch=[round(v, 4) for v in ms_t])
                if shape == "arrow" and beta == 0.0:
                    X, Y = ctx.wrap_vector(V), ctx.wrap_vector(torch.zeros((nrow, k), dtype=torch.float64, device=dev))
                    spmm = lambda: ctx.apply_multi(A, X, Y, k, overwrite=True)  # noqa: E731
                    window(spmm, 1)
                    rec["ms_spmm"] = round(float(np.median([window(spmm, 1) for _ in range(a.rounds)])), 4)
                line = json.dumps(rec)
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()
            del U, V, res, vU, vV, vO
            torch.cuda.empty_cache()
        del A, rows, cols
        torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
