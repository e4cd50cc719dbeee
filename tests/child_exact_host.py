"""Child of tests/test_gpu_exact.py: spmv_apply_host on exact poisoned inputs in a fresh context, so that SPMV_HOST_STORES (read
once per context) takes effect.  Vectors under 1 MB together (the small-vector path); CSR under several kernels, COO, CSC and ELL
handles; 1 and 3 calls.  Prints host_stores=<what the context found> and EXACT_HOST_OK when every check passed."""
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import numpy as np  # noqa: E402

import exact as ex  # noqa: E402
import oracle_lib as ol  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

REPS = 3


def main():
    capi = load_package().capi
    orc = ol.load_oracle()
    ctx = capi.Context(0)
    print(f"host_stores={ctx.get_param('host_stores')}", flush=True)
    base = int(os.environ.get("SPMV_FUZZ_BASE", "0"))
    rng = np.random.default_rng(base + 19_500)
    nrow, ncol = 30_000, 25_000
    lens = np.where(rng.random(nrow) < 0.2, 0, rng.integers(1, 14, nrow))
    lens[[3, 20_000]] = [12_000, 5000]  # a hub row: SPLIT and SEGSCAN add into y with device atomics
    rp = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
    cc = ex.avoid_columns(rng.integers(0, ncol, int(rp[-1])), ncol, (20_000, 7_000))
    bits, e = ex.choose_bits(int(lens.max()), REPS)
    cv = ex.dyadic(rng, len(cc), bits, e)
    x, y0 = ex.dyadic(rng, ncol, bits, e), ex.dyadic(rng, nrow, bits, e)
    ent = ex.csr_entries(rp, cc, cv)
    want1 = ex.exact_product(nrow, *ent, x, e, y0=y0)
    wantr = ex.exact_product(nrow, *ent, x, e, y0=y0, reps=REPS)
    xp = ex.poison(x, cc)
    assert 8 * (nrow + ncol) < (1 << 20)

    def check(M, what):
        y = y0.copy()
        ctx.apply_host(M, xp.copy(), y)
        assert np.array_equal(y, want1), f"{what}: 1 call"
        for _ in range(REPS - 1):
            ctx.apply_host(M, xp.copy(), y)
        assert np.array_equal(y, wantr), f"{what}: {REPS} calls"
        print(f"{what}: exact", flush=True)

    A = ctx.csr(nrow, ncol, rp, cc, cv)
    check(A, f"CSR auto (kernel {A.info.kernel})")
    for kernel in (capi.CSR_VECTOR, capi.CSR_SCALAR, capi.CSR_PANEL, capi.CSR_TWOPHASE, capi.CSR_SEGSCAN, capi.CSR_SPLIT):
        A.set_kernel(kernel)
        check(A, f"CSR kernel {kernel}")
    row = ol.i32(ent[0])
    for kernel in (capi.CSR_VECTOR, capi.CSR_PANEL):
        C = ctx.coo(nrow, ncol, row, cc, cv)
        C.set_kernel(kernel)
        check(C, f"COO kernel {kernel}")
        S = ctx.csc(nrow, ncol, *ol.coo_to_csc(orc, ncol, row, cc, cv))
        S.set_kernel(kernel)
        check(S, f"CSC kernel {kernel}")
    ctx.close()
    print("EXACT_HOST_OK")


if __name__ == "__main__":
    main()
