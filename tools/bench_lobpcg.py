#!/usr/bin/env python3
"""The block kernels of spmv_lobpcg by themselves (spmv_block_gram, spmv_block_combine) beside torch.matmul on the same device blocks
(rocBLAS: the baseline; the engine does not link it), and whole solves of spmv_lobpcg on the 2048^2 Laplacian.

Part "kernels", one JSON line per shape: n = 4M rows; Gram with p = q in {8, 16, 24, 48}, V another block and V = U; combine with
p = 48 -> q = 32.  Interleaved after a warm-up, the median over --rounds rounds of REPS calls each:
  ms_engine   wall time of a call between two device synchronisations (block_gram is synchronous: its read of G is inside);
  ms_torch    torch.matmul on the same memory (U^T V as (p, n) x (n, q); S C as (q, p) x (p, n)), between two device events;
  bytes       what the call must move: 8 n (p + q) (U = V: 8 n p; combine: 8 n (p + q));  frac_8tbs = bytes / ms against 8 TB/s;
  gflops      2 n p q / ms, to be set against the 78 TFLOP/s vector peak where a shape turns out compute-bound.

Part "solves", one JSON line per preconditioner: the 5-point Laplacian on 2048^2 points, k = 8, nev = 6, tol = 1e-6 ||A||_inf, the
start block gen_vector(seed 1), under none (capped at 200 iterations: it is expected NOT to converge, and the line says whether it
did), jacobi, chebyshev (degree 4), amg and amg_sa.  iterations, ms of the whole call, ms_iter = ms / iterations, and the split of one
iteration BY PARTS, each part timed by itself at the iteration's shapes (all k columns active, P in use) and multiplied by its count:
  products (k x spmv_apply), preconditioner (k x the engine's own application), gram (X^T W twice, W^T W, P^T P, S^T S, S^T AS, each
  with its read), combine (the seven of an iteration), host = ms_iter minus those (the small dense problems, copies of coefficients,
  launch gaps; negative where columns converged early and the parts overstate the iteration).

  python tools/bench_lobpcg.py [--parts kernels,solves] [--rounds 5] [--out profiles/r18_bench_lobpcg.jsonl]
Needs a GPU; there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch  # (before the engine's library: torch initialises its HIP runtime first)

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tools")]
from __graft_entry__ import load_package  # noqa: E402

capi = load_package().capi
N_KERNELS = 4 << 20
REPS = 10
K, NEV = 8, 6


def wall(ctx, f, reps):
    ctx.sync()
    t = time.perf_counter()
    for _ in range(reps):
        f()
    ctx.sync()
    return (time.perf_counter() - t) * 1e3 / reps


def torch_ms(f, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def kernels(ctx, emit, rounds):
    n = N_KERNELS
    dev = torch.device("cuda:0")
    for what, p, q in [("gram", c, c) for c in (8, 16, 24, 48)] + [("gram_same", c, c) for c in (8, 16, 24, 48)] + [("combine", 48, 32)]:
        g = torch.Generator(device=dev).manual_seed(p + q)
        U = torch.rand((p, n), dtype=torch.float64, device=dev, generator=g)  # row c = column c of the block: ld = n
        V = U if what == "gram_same" else torch.rand((q, n), dtype=torch.float64, device=dev, generator=g)
        Cm = np.random.default_rng(1).standard_normal((p, q))
        Ct = torch.from_numpy(Cm.T.copy()).to(dev)
        O = torch.empty((q, n), dtype=torch.float64, device=dev)
        G = torch.empty((p, q), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        dU, dV, dO = ctx.wrap_vector(U), ctx.wrap_vector(V), ctx.wrap_vector(O)
        if what == "combine":
            ours = lambda: ctx.block_combine(n, p, dU, n, q, Cm, dO, n)  # noqa: E731
            theirs = lambda: torch.matmul(Ct, U, out=O)  # noqa: E731
            nbytes = 8 * n * (p + q)
        else:
            ours = lambda: ctx.block_gram(n, p, dU, n, q, dV, n)  # noqa: E731
            theirs = lambda: torch.matmul(U, V.T, out=G)  # noqa: E731
            nbytes = 8 * n * (p if what == "gram_same" else p + q)
        ours(), theirs()
        torch.cuda.synchronize()
        ms_e, ms_t = [], []
        for _ in range(rounds):
            ms_e.append(wall(ctx, ours, REPS))
            ms_t.append(torch_ms(theirs, REPS))
        e, t = float(np.median(ms_e)), float(np.median(ms_t))
        emit(dict(part="kernels", what=what, n=n, p=p, q=q, ms_engine=round(e, 4), ms_torch=round(t, 4), engine_over_torch=round(e / t, 3), bytes=nbytes,
                  frac_8tbs=round(nbytes / (e * 1e-3) / 8e12, 4), frac_8tbs_torch=round(nbytes / (t * 1e-3) / 8e12, 4),
                  gflops=round(2.0 * n * p * q / (e * 1e-3) / 1e9, 1), rounds_engine=[round(v, 4) for v in ms_e], rounds_torch=[round(v, 4) for v in ms_t]))
        del dU, dV, dO, U, V, O


def solves(ctx, emit, rounds):
    from bench_bicgstab import laplacian_2d

    n, rp, cc, cv = laplacian_2d(2048)
    tol = 1e-6 * 8.0
    k = K
    for name in ("none", "jacobi", "chebyshev", "amg", "amg_sa"):
        A = ctx.csr(n, n, rp, cc, cv)
        code, apply, max_iter = capi.PRECOND_NONE, None, 200
        if name == "jacobi":
            code, max_iter = capi.PRECOND_JACOBI, 2000
        elif name == "chebyshev":
            ctx.chebyshev_setup(A, 4, True)
            code, apply, max_iter = capi.PRECOND_CHEBYSHEV, ctx.chebyshev_solve, 2000
        elif name in ("amg", "amg_sa"):
            (ctx.amg_setup_smoothed if name == "amg_sa" else ctx.amg_setup)(A)
            code, apply, max_iter = capi.PRECOND_AMG, ctx.amg_solve, 500
        rec = dict(part="solves", shape="lap2d_2048", nrow=n, k=k, nev=NEV, tol=tol, precond=name, max_iter=max_iter)
        try:
            X = ctx.gen_vector(n * k, seed=1)
            ctx.lobpcg(A, X, k, nev=NEV, max_iter=2, tol=tol, precond=code)  # warm-up
            X = ctx.gen_vector(n * k, seed=1)
            ctx.sync()
            t = time.perf_counter()
            theta, resid, iters = ctx.lobpcg(A, X, k, nev=NEV, max_iter=max_iter, tol=tol, precond=code)
            ms = (time.perf_counter() - t) * 1e3
        except capi.SpmvError as e:
            emit(dict(rec, error=str(e)))
            continue
        rec.update(iterations=iters, converged=bool(np.all(resid[:NEV] <= tol)), ms=round(ms, 2), ms_iter=round(ms / max(iters, 1), 4),
                   theta=[float(f"{v:.12e}") for v in theta[:NEV]], resid_max=float(f"{resid[:NEV].max():.3e}"))
        # one iteration by parts, at k active columns with P in use
        ld, m = n, 3 * k
        S, AS = ctx.gen_vector(ld * m, seed=2), ctx.gen_vector(ld * m, seed=3)
        x1, y1 = ctx.gen_vector(n, seed=4), ctx.vector(n)
        W = ctx.wrap_vector(S.device_ptr + 8 * ld * 2 * k, ld * k)
        P = ctx.wrap_vector(S.device_ptr + 8 * ld * k, ld * k)
        AP = ctx.wrap_vector(AS.device_ptr + 8 * ld * k, ld * k)
        T = ctx.vector(ld * m)
        ckk, cmk, cm2k = np.eye(k), np.ones((m, k)) / m, np.ones((m, 2 * k)) / m
        gram = lambda: (ctx.block_gram(n, k, S, ld, k, W, ld), ctx.block_gram(n, k, S, ld, k, W, ld), ctx.block_gram(n, k, W, ld, k, W, ld),  # noqa: E731
                        ctx.block_gram(n, k, P, ld, k, P, ld), ctx.block_gram(n, m, S, ld, m, S, ld), ctx.block_gram(n, m, S, ld, m, AS, ld))
        comb = lambda: (ctx.block_combine(n, m, S, ld, k, cmk, T, ld), ctx.block_combine(n, m, S, ld, k, cmk, T, ld),  # noqa: E731
                        ctx.block_combine(n, k, W, ld, k, ckk, W, ld), ctx.block_combine(n, k, P, ld, k, ckk, P, ld),
                        ctx.block_combine(n, k, AP, ld, k, ckk, AP, ld), ctx.block_combine(n, m, S, ld, 2 * k, cm2k, T, ld),
                        ctx.block_combine(n, m, AS, ld, 2 * k, cm2k, T, ld))
        parts = {"products": lambda: [ctx.apply(A, x1, y1) for _ in range(k)], "gram": gram, "combine": comb}
        if apply is not None:
            parts["preconditioner"] = lambda: [apply(A, x1, y1) for _ in range(k)]
        elif name == "jacobi":
            parts["preconditioner"] = lambda: [ctx.axpby(1.0, x1, 0.0, x1, y1) for _ in range(k)]  # (a stand-in of the same bytes: one read, one write)
        split = {}
        for part, f in parts.items():
            f()
            split[part] = round(float(np.median([wall(ctx, f, 3) for _ in range(rounds)])), 4)
        split.setdefault("preconditioner", 0.0)
        split["host"] = round(rec["ms_iter"] - sum(split.values()), 4)
        rec.update(split_ms=split, ms_product=round(split["products"] / k, 4), iteration_over_its_products=round(rec["ms_iter"] / max(split["products"], 1e-9), 2))
        emit(rec)
        del A, X, S, AS, W, P, AP, T, x1, y1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parts", default="kernels,solves")
    ap.add_argument("--rounds", type=int, default=5)
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

    for part in a.parts.split(","):
        {"kernels": kernels, "solves": solves}[part](ctx, emit, a.rounds)
    if out:
        out.close()


if __name__ == "__main__":
    main()
