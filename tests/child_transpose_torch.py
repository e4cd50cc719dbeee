"""Child of tests/test_gpu_transpose.py: the torch operator over the transposed product.  torch initialises its HIP runtime
before the engine's library is loaded (as bench.py does).  Prints TRANSPOSE_TORCH_OK <case> when every check passed."""
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

import oracle_lib as ol  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402


def _random_coo(nrow, ncol, nnz, seed):
    rng = np.random.default_rng(seed)
    return (ol.i32(rng.integers(0, nrow, size=nnz)), ol.i32(rng.integers(0, ncol, size=nnz)), rng.uniform(-1, 1, size=nnz))


def gradcheck(ctx, orc, tops):
    """d/dx of spmv(op, x) on a 200 x 150 CSR matrix, fp64: the backward pass (A^T grad) against finite differences"""
    nrow, ncol = 200, 150
    row, col, val = _random_coo(nrow, ncol, 1500, 3)
    rp, cc, cv = ol.coo_to_csr(orc, nrow, row, col, val)
    op = tops.SparseOperator(ctx, ctx.csr(nrow, ncol, rp, cc, cv))
    x = torch.rand(ncol, dtype=torch.float64, device=dev, requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: tops.spmv(op, t), (x,), eps=1e-6, atol=1e-9, rtol=1e-7)
    # and the gradient itself against dense A^T g
    dense = torch.zeros((nrow, ncol), dtype=torch.float64)
    dense.index_put_((torch.from_numpy(row).long(), torch.from_numpy(col).long()), torch.from_numpy(val), accumulate=True)
    y = tops.spmv(op, x)
    g = torch.rand(nrow, dtype=torch.float64, device=dev)
    (y * g).sum().backward()
    assert torch.allclose(x.grad.cpu(), dense.T @ g.cpu(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(y.detach().cpu(), dense @ x.detach().cpu(), rtol=1e-12, atol=1e-12)


def rmatvec(ctx, orc, tops):
    """rmatvec on a CSC handle against dense A.T @ y"""
    nrow, ncol = 700, 450
    row, col, val = _random_coo(nrow, ncol, 6000, 4)
    cp, cr, cv = ol.coo_to_csc(orc, ncol, row, col, val)
    op = tops.SparseOperator(ctx, ctx.csc(nrow, ncol, cp, cr, cv))
    dense = torch.zeros((nrow, ncol), dtype=torch.float64)
    dense.index_put_((torch.from_numpy(row).long(), torch.from_numpy(col).long()), torch.from_numpy(val), accumulate=True)
    y = torch.rand(nrow, dtype=torch.float64, device=dev) - 0.5
    got = op.rmatvec(y)
    assert got.shape == (ncol,) and got.device == dev
    assert torch.allclose(got.cpu(), dense.T @ y.cpu(), rtol=1e-12, atol=1e-12)
    try:
        op.rmatvec(torch.zeros(ncol, dtype=torch.float64, device=dev))
    except ValueError:
        pass
    else:
        raise AssertionError("rmatvec took a vector of the wrong length")


if __name__ == "__main__":
    case = sys.argv[1]
    pkg = load_package()
    tops = importlib.import_module("arm_spmv_amd.torch_ops")
    ctx = tops.context_on_current_stream(0)
    {"gradcheck": gradcheck, "rmatvec": rmatvec}[case](ctx, ol.load_oracle(), tops)
    torch.cuda.synchronize()
    ctx.close()
    print(f"TRANSPOSE_TORCH_OK {case}")
