"""Child of tests/test_gpu_gmres.py: SparseOperator.solve(method="gmres") against Context.gmres on the same stream, bit for bit, and
solve() without a method against Context.bicgstab.  torch initialises its HIP runtime before the engine's library is loaded (as
bench.py does).  Prints GMRES_TORCH_OK when every check passed."""
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

import gmres_ref as gr  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

if __name__ == "__main__":
    load_package()
    tops = importlib.import_module("arm_spmv_amd.torch_ops")
    ctx = tops.context_on_current_stream(0)
    n, ent, b, x0, ks = gr.problem("r33")
    rp, cc, cv = gr.csr_arrays(n, *ent)
    A = ctx.csr(n, n, rp, cc, cv)
    # A solve is as reproducible as the handle's product, and bits are compared here: the one-lane-per-row kernel
    A.set_kernel(3)
    op = tops.SparseOperator(ctx, A)
    tb, tx0 = torch.from_numpy(b).to(dev), torch.from_numpy(x0).to(dev)
    for kw in (dict(max_iter=9, rel_tol=0.0), dict(restart=4, max_iter=9, rel_tol=0.0), dict(restart=8, max_iter=200, rel_tol=1e-10, precond=1, check_every=3)):
        for start in (tx0, None):
            got = op.solve(tb, start, method="gmres", **kw)
            assert got.shape == (n,) and got.device == dev and got.dtype == torch.float64 and not got.requires_grad
            assert start is None or (got.data_ptr() != start.data_ptr() and torch.equal(start.cpu(), torch.from_numpy(x0))), "x0 was written"
            x = ctx.vector_from(x0 if start is not None else np.zeros(n))
            stats = ctx.gmres(op.A, ctx.vector_from(b), x, **kw)
            assert stats == op.last_solve and stats[0] > 0, (stats, op.last_solve)
            assert got.cpu().numpy().tobytes() == x.download().tobytes(), (kw, "solve(method='gmres') and Context.gmres differ")
    # without a method (and with method="bicgstab") solve is BiCGSTAB's bits, as before
    for extra in ({}, {"method": "bicgstab"}):
        got = op.solve(tb, tx0, max_iter=9, rel_tol=0.0, **extra)
        x = ctx.vector_from(x0)
        stats = ctx.bicgstab(op.A, ctx.vector_from(b), x, max_iter=9, rel_tol=0.0)
        assert stats == op.last_solve and got.cpu().numpy().tobytes() == x.download().tobytes(), "solve() is no longer Context.bicgstab"
    xg = ctx.vector_from(x0)
    ctx.gmres(op.A, ctx.vector_from(b), xg, max_iter=9, rel_tol=0.0)
    assert xg.download().tobytes() != x.download().tobytes(), "GMRES and BiCGSTAB iterates coincide: the method is not passed on"
    for bad in (dict(method="cg"), dict(restart=4)):
        try:
            op.solve(tb, **bad)
        except ValueError:
            pass
        else:
            raise AssertionError(f"solve took {bad}")
    try:
        op.solve(torch.zeros(n + 1, dtype=torch.float64, device=dev), method="gmres")
    except ValueError:
        pass
    else:
        raise AssertionError("solve took a right-hand side of the wrong length")
    torch.cuda.synchronize()
    ctx.close()
    print("GMRES_TORCH_OK")
