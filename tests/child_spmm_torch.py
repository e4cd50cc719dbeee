"""Child of tests/test_gpu_spmm.py: the multi-vector product with torch tensors.  torch initialises its HIP runtime before the
engine's library is loaded (as bench.py does).  Prints SPMM_TORCH_OK <case> when every check passed."""
import sys
from pathlib import Path

import torch

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
torch.zeros(1, device=dev)

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import numpy as np  # noqa: E402

import oracle_lib as ol  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402


def _oracle_columns(spmv, X, Y0):
    Y = np.empty_like(Y0)
    for c in range(X.shape[1]):
        y = Y0[:, c].copy()
        spmv(np.ascontiguousarray(X[:, c]), y)
        Y[:, c] = y
    return Y


def wrapped(ctx, orc, pkg):
    synth = pkg.synth
    n, ncol, per_row, k = 30_000, 25_000, 12, 13
    rp, cc, cv = synth.csr_uniform(0, n, ncol, per_row, seed=44)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(7)
    X = torch.rand((ncol, k), dtype=torch.float64, device=dev, generator=g)
    Y0 = torch.rand((n, k), dtype=torch.float64, device=dev, generator=g) - 0.5
    t_rp = torch.from_numpy(rp).to(dev)
    t_cc = torch.from_numpy(cc).to(dev)
    t_cv = torch.from_numpy(cv).to(dev)
    torch.cuda.synchronize()

    whole = ctx.csr(n, ncol, rp, cc, cv)
    vX = ctx.wrap_vector(X)
    Yw = Y0.clone()
    torch.cuda.synchronize()
    ctx.apply_multi(whole, vX, ctx.wrap_vector(Yw), k)
    ctx.sync()
    ref = _oracle_columns(lambda x, y: ol.csr_spmv(orc, rp, cc, cv, x, y, fma=True), X.cpu().numpy(), Y0.cpu().numpy())
    assert np.array_equal(Yw.cpu().numpy(), ref)

    wrapped = ctx.wrap_csr(n, ncol, t_rp, t_cc, t_cv)
    Yv = Y0.clone()
    torch.cuda.synchronize()
    ctx.apply_multi(wrapped, vX, ctx.wrap_vector(Yv), k)
    ctx.sync()
    assert torch.equal(Yv, Yw)

    rp64 = rp.astype(np.int64)
    for b, e in ((0, 7_001), (7_001, 19_999), (19_999, n)):
        S = ctx.csr_shard(b, e, ncol, rp64, cc, cv)
        Ys = Y0[b:e].clone()
        torch.cuda.synchronize()
        ctx.apply_multi(S, vX, ctx.wrap_vector(Ys), k)
        ctx.sync()
        assert torch.equal(Ys, Yw[b:e]), f"shard [{b}, {e})"


def c2(ctx, orc, pkg):
    capi = pkg.capi
    n, per_row, k = 10_000_000, 32, 8
    A = ctx.gen_csr_uniform(0, n, n, per_row, 0, seed=2)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(11)
    X = torch.rand((n, k), dtype=torch.float64, device=dev, generator=g)
    Y = torch.rand((n, k), dtype=torch.float64, device=dev, generator=g)
    Y0 = Y.clone()
    torch.cuda.synchronize()
    ctx.apply_multi(A, ctx.wrap_vector(X), ctx.wrap_vector(Y), k)
    ctx.sync()
    A.set_kernel(capi.CSR_SCALAR)
    for c in range(k):
        x = X[:, c].contiguous()
        y = Y0[:, c].contiguous()
        torch.cuda.synchronize()
        ctx.apply(A, ctx.wrap_vector(x), ctx.wrap_vector(y))
        ctx.sync()
        assert torch.equal(Y[:, c], y), f"column {c}"


if __name__ == "__main__":
    case = sys.argv[1]
    pkg = load_package()
    ctx = pkg.capi.Context(0)
    {"wrapped": wrapped, "c2": c2}[case](ctx, ol.load_oracle(), pkg)
    ctx.close()
    print(f"SPMM_TORCH_OK {case}")
