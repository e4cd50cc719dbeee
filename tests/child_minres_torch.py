"""Child of tests/test_gpu_minres.py: SparseOperator.solve_symmetric against Context.minres on the same stream, bit for bit.  torch
initialises its HIP runtime before the engine's library is loaded (as bench.py does).  Prints MINRES_TORCH_OK when every check
passed."""
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

import minres_ref as mr  # noqa: E402
from cgls_ref import rect  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402


def _csr(ctx, n, entries):
    row, col, val = entries
    o = np.argsort(row, kind="stable")
    return ctx.csr(n, n, *mr.csr_arrays(n, row[o], col[o], val[o]))


if __name__ == "__main__":
    load_package()
    tops = importlib.import_module("arm_spmv_amd.torch_ops")
    ctx = tops.context_on_current_stream(0)
    p = mr.problem("saddle")
    n, b, x0 = p.n, p.b, p.x0
    A, P = _csr(ctx, n, p.entries), _csr(ctx, n, p.p_entries)
    # A solve is as reproducible as the handle's product, and bits are compared here: the one-lane-per-row kernel
    A.set_kernel(3)
    op = tops.SparseOperator(ctx, A)
    tb, tx0 = torch.from_numpy(b).to(dev), torch.from_numpy(x0).to(dev)
    cases = (dict(max_iter=9, rel_tol=0.0), dict(max_iter=9, rel_tol=0.0, shift=0.375),
             dict(max_iter=500, rel_tol=1e-10, precond=1, check_every=3, M=P, shift=-0.25))
    for kw in cases:
        for start in (tx0, None):
            got = op.solve_symmetric(tb, start, **kw)
            assert got.shape == (n,) and got.device == dev and got.dtype == torch.float64 and not got.requires_grad
            assert start is None or (got.data_ptr() != start.data_ptr() and torch.equal(start.cpu(), torch.from_numpy(x0))), "x0 was written"
            x = ctx.vector_from(x0 if start is not None else np.zeros(n))
            direct = {("P" if k == "M" else k): v for k, v in kw.items()}
            stats = ctx.minres(op.A, ctx.vector_from(b), x, **direct)
            assert stats == op.last_solve and stats[0] > 0, (stats, op.last_solve)
            assert got.cpu().numpy().tobytes() == x.download().tobytes(), (kw, "solve_symmetric and Context.minres differ")
    try:
        op.solve_symmetric(torch.zeros(n + 1, dtype=torch.float64, device=dev))
    except ValueError:
        pass
    else:
        raise AssertionError("solve_symmetric took a right-hand side of the wrong length")
    # a non-square operator is refused before the engine is called
    rp, cc, cv = mr.csr_arrays(33, *rect(33, 17, 6, 7))
    rect_op = tops.SparseOperator(ctx, ctx.csr(33, 17, rp, cc, cv))
    try:
        rect_op.solve_symmetric(torch.zeros(33, dtype=torch.float64, device=dev))
    except ValueError as e:
        assert "square" in str(e)
    else:
        raise AssertionError("solve_symmetric took a 33 x 17 operator")
    torch.cuda.synchronize()
    ctx.close()
    print("MINRES_TORCH_OK")
