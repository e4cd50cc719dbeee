#!/usr/bin/env python3
"""The block CSR product (spmv_apply on a BSR handle) against the CSR AUTO handle of the same matrix (spmv_bsr_to_csr).

One JSON line per workload:
  ms_bsr, ms_csr    the two products, interleaved in rounds after a warm-up, each round a window of `reps` products timed by the
                    host clock between two device synchronisations; the medians of 3 rounds;
  ratio             ms_csr / ms_bsr (above 1: BSR is faster);
  gbs_bsr, gbs_csr  bytes_alg / ms: (8 + 4 / bs^2) bytes per stored value and the block row pointer for BSR, 12 per entry and the
                    row pointer for CSR, plus x read once and y read and written;
  ms_by_lanes       the BSR product under every number of lanes per block row (spmv_mat_set_kernel(VECTOR, lanes));
  setup_bsr_to_csr_s, setup_csr_to_bsr_s   the two conversions, wall clock (synchronous; the new handle's analysis included);
  csr_kernel        what AUTO picked for the CSR handle (kernel ids of include/spmv_abi.h).

Workloads: uniform (bs 4, 2.5M block rows x 8 blocks with uniform-random block columns: scalar 10M x 32), band (the same in a band
of 16384 blocks), grid27 (bs 3 on the 27-point pattern of a 100^3 grid: 3M rows of 81), grid5 (bs 2 on the 5-point pattern of a
2048^2 grid).  --scale divides the number of block rows (the grids' edge by its root) for a quick look.

  python tools/bench_bsr.py [--workloads uniform,band,grid27,grid5] [--out profiles/r20_bench_bsr.jsonl]
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


def structure(name, scale):
    """(bs, mb, brow_ptr, bcol) with block columns ascending inside a block row"""
    rng = np.random.default_rng(3)
    if name in ("uniform", "band"):
        bs, mb, per = 4, 2_500_000 // scale, 8
        if name == "uniform":
            bc = rng.integers(0, mb - per + 1, size=(mb, per))
        else:
            bc = np.clip(np.arange(mb)[:, None] + rng.integers(-8192, 8192 - per, size=(mb, per)), 0, mb - per)
        bc = np.sort(bc, axis=1) + np.arange(per)  # (distinct inside a block row: the k-th smallest moved up by k)
        return bs, mb, (per * np.arange(mb + 1)).astype(np.int32), bc.astype(np.int32).reshape(-1)
    if name in ("grid27", "grid5"):
        dim = 3 if name == "grid27" else 2
        bs = 3 if name == "grid27" else 2
        edge = max(4, int(round((100 if dim == 3 else 2048) / scale ** (1.0 / dim))))
        idx = np.indices((edge,) * dim).reshape(dim, -1)
        steps = [s for s in np.ndindex((3,) * dim)] if dim == 3 else [(1, 1), (0, 1), (1, 0), (1, 2), (2, 1)]
        cols, ok = [], []
        for s in steps:
            nb = idx + (np.array(s)[:, None] - 1)
            ok.append(np.all((nb >= 0) & (nb < edge), axis=0))
            cols.append(np.ravel_multi_index(np.clip(nb, 0, edge - 1), (edge,) * dim))
        cols, ok = np.stack(cols, axis=1), np.stack(ok, axis=1)
        cols = np.where(ok, cols, np.iinfo(np.int64).max)
        cols.sort(axis=1)
        counts = ok.sum(axis=1)
        return bs, edge**dim, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), cols[cols != np.iinfo(np.int64).max].astype(np.int32)
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
    ap.add_argument("--workloads", default="uniform,band,grid27,grid5")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r20_bench_bsr.jsonl"), help="JSON lines are appended here too")
    a = ap.parse_args()
    ctx = capi.Context(0)
    out = open(a.out, "a") if a.out else None
    for name in a.workloads.split(","):
        bs, mb, bp, bc = structure(name, a.scale)
        n, nnzb = bs * mb, len(bc)
        val = np.resize(np.random.default_rng(4).uniform(0.5, 1.5, size=1 << 20), nnzb * bs * bs)  # (no zeros: the CSR form keeps every position)
        A = ctx.bsr(n, n, bs, bp, bc, val)
        del val
        ctx.sync()
        t0 = time.perf_counter()
        C = ctx.bsr_to_csr(A)
        ctx.sync()
        to_csr_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        B = ctx.csr_to_bsr(C, bs)
        ctx.sync()
        to_bsr_s = time.perf_counter() - t0
        assert (B.info.nnz, B.info.ell_k) == (A.info.nnz, bs) and C.info.nnz == A.info.nnz
        del B
        x, ya, yc = ctx.gen_vector(n, seed=5), ctx.vector(n), ctx.vector(n)
        ya.fill(0.0)
        yc.fill(0.0)
        f_bsr = lambda: ctx.apply(A, x, ya)  # noqa: E731
        f_csr = lambda: ctx.apply(C, x, yc)  # noqa: E731
        t_b = max(window(ctx, f_bsr, 1), window(ctx, f_bsr, 1))  # warm-up
        t_c = max(window(ctx, f_csr, 1), window(ctx, f_csr, 1))
        reps_b = max(1, min(200, int(50 / max(t_b, 1e-3))))
        reps_c = max(1, min(200, int(50 / max(t_c, 1e-3))))
        ms_b, ms_c = [], []
        for _ in range(a.rounds):
            ms_b.append(window(ctx, f_bsr, reps_b))
            ms_c.append(window(ctx, f_csr, reps_c))
        mb_ms, mc_ms = float(np.median(ms_b)), float(np.median(ms_c))
        chosen = int(A.info.lanes_per_row)
        slots = 64 // (bs * bs)
        by_lanes = {}
        for g in [g for g in range(1, slots + 1) if slots % g == 0]:
            A.set_kernel(VECTOR, g * bs * bs)
            window(ctx, f_bsr, 1)
            by_lanes[str(g * bs * bs)] = round(window(ctx, f_bsr, reps_b), 4)
        A.set_kernel(VECTOR, chosen)
        nnz = nnzb * bs * bs
        bytes_bsr = nnz * 8 + nnzb * 4 + 4 * (mb + 1) + 8 * n + 16 * n
        bytes_csr = nnz * 12 + 4 * (n + 1) + 8 * n + 16 * n
        rec = dict(workload=name, bs=bs, nrow=n, block_rows=mb, blocks=nnzb, nnz=nnz, lanes_per_block_row=chosen, csr_kernel=int(C.info.kernel),
                   ms_bsr=round(mb_ms, 4), ms_csr=round(mc_ms, 4), ratio=round(mc_ms / mb_ms, 3), bytes_bsr=int(bytes_bsr), bytes_csr=int(bytes_csr),
                   gbs_bsr=round(bytes_bsr / mb_ms / 1e6, 1), gbs_csr=round(bytes_csr / mc_ms / 1e6, 1), ms_by_lanes=by_lanes,
                   setup_bsr_to_csr_s=round(to_csr_s, 3), setup_csr_to_bsr_s=round(to_bsr_s, 3), rounds_bsr=[round(v, 4) for v in ms_b],
                   rounds_csr=[round(v, 4) for v in ms_c])
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
        del A, C, x, ya, yc
    if out:
        out.close()


if __name__ == "__main__":
    main()
