"""Child of tests/test_gpu_cgls.py: SparseOperator.lstsq against Context.cgls on the same stream, bit for bit.  torch initialises
its HIP runtime before the engine's library is loaded (as bench.py does).  Prints CGLS_TORCH_OK when every check passed."""
import sys
from pathlib import Path

import torch

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
torch.zeros(1, device=dev)

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import importlib  # noqa: E402

import numpy as np  # noqa: E402

import cgls_ref as cr  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

if __name__ == "__main__":
    load_package()
    tops = importlib.import_module("arm_spmv_amd.torch_ops")
    ctx = tops.context_on_current_stream(0)
    (m, n), ent, b, x0, ks = cr.problem("r33x17")
    rp, cc, cv = cr.csr_arrays(m, *ent)
    A = ctx.csr(m, n, rp, cc, cv)
    # A solve is as reproducible as the handle's two products, and bits are compared here: the transposed side runs from the CSC
    # companion's row-grouped copy (fixed order of additions), not from its scatter (atomic adds in arrival order, AUTO's pick at
    # this size); the forward side from the one-lane-per-row kernel
    A.set_kernel(3)
    A.set_param("transpose_kernel", 4)
    op = tops.SparseOperator(ctx, A)
    tb, tx0 = torch.from_numpy(b).to(dev), torch.from_numpy(x0).to(dev)
    for kw in (dict(max_iter=13, rel_tol=0.0), dict(max_iter=200, rel_tol=1e-10, damp=0.5, check_every=3)):
        for start in (tx0, None):
            got = op.lstsq(tb, start, **kw)
            assert got.shape == (n,) and got.device == dev and got.dtype == torch.float64 and not got.requires_grad
            assert start is None or (got.data_ptr() != start.data_ptr() and torch.equal(start.cpu(), torch.from_numpy(x0))), "x0 was written"
            x = ctx.vector_from(x0 if start is not None else np.zeros(n))
            stats = ctx.cgls(op.A, ctx.vector_from(b), x, **kw)
            assert stats == op.last_lstsq and stats[0] > 0, (stats, op.last_lstsq)
            assert got.cpu().numpy().tobytes() == x.download().tobytes(), (kw, "lstsq and Context.cgls differ")
    try:
        op.lstsq(torch.zeros(n, dtype=torch.float64, device=dev))
    except ValueError:
        pass
    else:
        raise AssertionError("lstsq took a right-hand side of the wrong length")
    torch.cuda.synchronize()
    ctx.close()
    print("CGLS_TORCH_OK")
