"""Child of tests/test_gpu_exact.py: the multi-vector product with SPMV_SPMM_LANES = 32 or 64 (the engine reads it once per
process), on exact poisoned inputs for k = 17..64, CSR and ELL; with 64 lanes also the grid-stride case.  Prints one line
"T=<lanes> k=<k>" per k (the lane count from the kernel's rule) and SPMM_LANES_OK <cap> when every check passed."""
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import numpy as np  # noqa: E402

import exact as ex  # noqa: E402
import test_gpu_exact as tge  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402


def main():
    cap = int(os.environ["SPMV_SPMM_LANES"])
    assert cap in (32, 64), cap
    capi = load_package().capi
    ctx = capi.Context(0)
    base = tge.BASE
    for seed in (3, 7):  # empty rows and rows of 40000 entries; one of the fuzz shapes (first rows only)
        nrow, ncol, rp, cc = tge._csr_shape(seed)
        r1 = int(np.searchsorted(rp, 200_000, side="right")) - 1
        if r1 < nrow:
            nrow, rp, cc = max(r1, 1), rp[: max(r1, 1) + 1].copy(), cc[: rp[max(r1, 1)]].copy()
        rng = np.random.default_rng(base + 19_000 + seed)
        lens = np.diff(rp)
        bits, e = ex.choose_bits(int(lens.max(initial=0)), tge.REPS)
        cv = ex.dyadic(rng, len(cc), bits, e)
        ks = range(17, 65)
        A = ctx.csr(nrow, ncol, rp, cc, cv)
        tge._check_multi(ctx, A, rng, nrow, ncol, ex.csr_entries(rp, cc, cv), cc, ks, f"lanes {cap}, seed {seed}: CSR", bits, e)
        k = int(lens.max(initial=0))
        if k and nrow * k <= 4_000_000:
            slot = np.arange(len(cc)) - np.repeat(rp[:-1].astype(np.int64), lens)
            rows = np.repeat(np.arange(nrow), lens)
            ec, ev = np.zeros((k, nrow), np.int32), np.zeros((k, nrow))
            ec[slot, rows], ev[slot, rows] = cc, cv
            E = ctx.ell(nrow, ncol, k, len(cc), ec.ravel(), ev.ravel())
            tge._check_multi(ctx, E, rng, nrow, ncol, ex.ell_entries(nrow, k, ec.ravel(), ev.ravel()), ec.ravel(), ks,
                             f"lanes {cap}, seed {seed}: ELL", bits, e)
        print(f"seed {seed}: {nrow} x {ncol}, {len(cc)} entries: k = 17..64 exact", flush=True)
    for k in range(17, 65):
        print(f"T={tge.spmm_lanes(k, cap)} k={k}")
    if cap == 64:
        T, nvb = tge.grid_stride_case(ctx, cap)
        assert T == 64, T
        print(f"grid-stride T={T}: virtual blocks {nvb} (> {1 << 20})", flush=True)
    ctx.close()
    print(f"SPMM_LANES_OK {cap}")


if __name__ == "__main__":
    main()
