#!/usr/bin/env python3
"""Reordering measured: what a reverse Cuthill-McKee renumbering (spmv_perm_rcm, spmv_csr_permute) gives back of the locality that a
bad numbering took, and what it costs.

One JSON line per family, printed as it is made, every figure from this one process.  Per family three handles under AUTO:
  (a) the matrix as generated, (b) the same matrix under a random symmetric shuffle (spmv_csr_permute with a random permutation),
  (c) the shuffled one after spmv_perm_rcm and spmv_csr_permute.
Their spmv_apply times (spmv_apply_timed) are taken interleaved, one measurement each per round, after a warm-up round; the figures
are medians over --rounds rounds.  The yardstick for (c) is (a) of the same process.  spmv_perm_rcm and spmv_csr_permute are timed
once per round as the wall time of the whole synchronous call (the handle's analysis included; SPMV_PANEL_TRIAL=0 is set for the
run, so no timing launches fall into it) and given in ms and in products of (a).  spmv_vec_permute is timed per direction over 20
launches between two synchronisations; GB/s is given against 24 n bytes (8 n read, 8 n written, 4 n of indices, and 4 n for the
lines of the scattered side that are fetched only in part).

Families: band (n x 32, columns random in a band of 65536 around the diagonal, bench.py's seeds; --band-rows, default 10M),
lap2d (the 5-point Laplacian on a 2048 x 2048 grid; --grid), rmat (an R-MAT graph of scale 22, 8 edges a vertex; --rmat-scale).

  python tools/bench_reorder.py [--families band,lap2d,rmat] [--rounds 3] [--out profiles/r19_bench_reorder.jsonl]
Needs a GPU; there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

os.environ["SPMV_PANEL_TRIAL"] = "0"
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from bench_ilu0 import capi, stencil  # noqa: E402
from bench_spgemm import rmat  # noqa: E402

FAMILIES = ("band", "lap2d", "rmat")
REPS_APPLY = 20
REPS_VEC = 20
COUNTERS = ("rcm_isolated", "rcm_components", "rcm_levels", "rcm_bfs", "rcm_launches", "rcm_transient_bytes")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--families", default=",".join(FAMILIES))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--band-rows", type=int, default=10_000_000)
    ap.add_argument("--grid", type=int, default=2048)
    ap.add_argument("--rmat-scale", type=int, default=22)
    ap.add_argument("--seed", type=int, default=1)
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

    def timed(call):
        ctx.sync()
        t = time.perf_counter()
        result = call()
        ctx.sync()
        return (time.perf_counter() - t) * 1e3, result

    for name in a.families.split(","):
        if name == "band":
            n = a.band_rows
            A = ctx.gen_csr_uniform(0, n, n, 32, band=65536, seed=a.seed)
        elif name == "lap2d":
            n, rp, cc, cv = stencil(a.grid, 2, False)
            A = ctx.csr(n, n, rp, cc, cv)
            del rp, cc, cv
        else:
            n, rp, cc, cv = rmat(a.rmat_scale, 8, seed=a.seed)
            A = ctx.csr(n, n, rp, cc, cv)
            del rp, cc, cv
        rec = dict(family=name, nrow=n, nnz=int(A.info.nnz))
        try:
            shuffle = ctx.perm(np.random.default_rng(a.seed).permutation(n).astype(np.int32))
            S = ctx.csr_permute(A, shuffle, shuffle)
            x, y, z = ctx.gen_vector(n, seed=a.seed), ctx.vector(n), ctx.vector(n)
            y.fill(0.0)
            ms = {"generated": [], "shuffled": [], "rcm": []}
            ms_rcm, ms_permute, ms_vec = [], [], {False: [], True: []}
            p = B = None
            for rnd in range(a.rounds + 1):  # round 0 warms up
                del p, B
                t_rcm, p = timed(lambda: ctx.perm_rcm(S))
                t_permute, B = timed(lambda: ctx.csr_permute(S, p, p))
                for key, M in (("generated", A), ("shuffled", S), ("rcm", B)):
                    t = ctx.apply_timed(M, x, y, REPS_APPLY)
                    if rnd:
                        ms[key].append(t)
                for back in (False, True):
                    t, _ = timed(lambda: [ctx.vec_permute(p, x, z, back=back) for _ in range(REPS_VEC)])
                    if rnd:
                        ms_vec[back].append(t / REPS_VEC)
                if rnd:
                    ms_rcm.append(t_rcm)
                    ms_permute.append(t_permute)
            med = lambda v: float(np.median(v))
            t_a, t_b, t_c = med(ms["generated"]), med(ms["shuffled"]), med(ms["rcm"])
            rec.update(ms_apply_generated=round(t_a, 4), ms_apply_shuffled=round(t_b, 4), ms_apply_rcm=round(t_c, 4),
                       rcm_over_generated=round(t_c / t_a, 3), shuffled_over_rcm=round(t_b / t_c, 3),
                       kernel_generated=int(A.info.kernel), kernel_shuffled=int(S.info.kernel), kernel_rcm=int(B.info.kernel),
                       bandwidth_generated=ctx.csr_bandwidth(A)[0], bandwidth_shuffled=ctx.csr_bandwidth(S)[0], bandwidth_rcm=ctx.csr_bandwidth(B)[0],
                       ms_perm_rcm=round(med(ms_rcm), 2), perm_rcm_in_applies=round(med(ms_rcm) / t_a, 1),
                       ms_csr_permute=round(med(ms_permute), 2), csr_permute_in_applies=round(med(ms_permute) / t_a, 1),
                       ms_vec_gather=round(med(ms_vec[False]), 4), ms_vec_scatter=round(med(ms_vec[True]), 4),
                       gbs_vec_gather=round(24 * n / med(ms_vec[False]) / 1e6, 1), gbs_vec_scatter=round(24 * n / med(ms_vec[True]) / 1e6, 1),
                       **{c: p.info(c) for c in COUNTERS})
            del p, B, S, shuffle, x, y, z
        except capi.SpmvError as e:
            rec.update(error=str(e))
        emit(rec)
        del A
    if out:
        out.close()


if __name__ == "__main__":
    main()
