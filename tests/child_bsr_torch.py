"""Child of tests/test_gpu_bsr.py: block CSR over torch's device memory.  torch initialises its HIP runtime before the engine's
library is loaded (as bench.py does).  Prints BSR_TORCH_OK <case> when every check passed.

  exact     every block size, 37 block rows of 0 / 1 / S / S + 1 / 1000 blocks, every number of lanes per block row, forward and
            transposed, bit for bit; y is spmv_vec_wrap_device over the first n entries of a torch tensor of n + 1, the last one a
            guard that must stay as it was
  validate  spmv_bsr_wrap_device over torch tensors, then spmv_mat_validate after a block column and a pointer entry were changed
            under the handle
"""
import sys
from pathlib import Path

import torch

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
torch.zeros(1, device=dev)

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import numpy as np  # noqa: E402

import test_gpu_bsr as T  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402


def torch_guarded(ctx, host):
    t = torch.from_numpy(np.concatenate([host, [T.GUARD]])).to(dev)
    torch.cuda.synchronize()
    v = ctx.wrap_vector(t, n=len(host))

    def read():
        torch.cuda.synchronize()
        return t.cpu().numpy()

    return v, read


def exact(ctx, capi):
    for bs in range(2, 9):
        T.check_exact(ctx, bs, [m for m in T._exact_matrices(bs) if m[0] == "mb37"], torch_guarded)


def validate(ctx, capi):
    rng = np.random.default_rng(41)
    nrow, ncol, bs, bp, bc, bv = T._small(rng)
    nbc = -(-ncol // bs)
    k = int(np.flatnonzero(np.diff(bp) > 0)[0]) + 1  # the first pointer entry behind a block: lowering it makes the pointer decrease
    assert bp[k] > 0 and k < len(bp) - 1
    d_bp, d_bc, d_bv = torch.from_numpy(bp).to(dev), torch.from_numpy(bc).to(dev), torch.from_numpy(bv).to(dev)
    torch.cuda.synchronize()
    W = ctx.wrap_bsr(nrow, ncol, bs, d_bp, d_bc, d_bv)
    W.validate()
    assert W.info.device_bytes == 0 and W.info.nnz == len(bv) and W.info.format == 5

    def refused(needle):
        torch.cuda.synchronize()
        try:
            W.validate()
        except capi.SpmvError as err:
            assert needle in str(err), err
        else:
            raise AssertionError(f"spmv_mat_validate took a handle with {needle}")

    d_bc[len(bc) // 2] = nbc
    refused("index out of range")
    d_bc[len(bc) // 2] = 0
    d_bp[k] = int(bp[k - 1]) - 1 if bp[k - 1] > 0 else int(bp[k + 1]) + 1
    refused("offsets decrease")
    d_bp[k] = int(bp[k])
    torch.cuda.synchronize()
    W.validate()
    del W


if __name__ == "__main__":
    case = sys.argv[1]
    pkg = load_package()
    ctx = pkg.capi.Context(0)
    {"exact": exact, "validate": validate}[case](ctx, pkg.capi)
    ctx.sync()
    ctx.close()
    print(f"BSR_TORCH_OK {case}")
