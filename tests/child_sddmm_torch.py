"""Child of tests/test_gpu_sddmm.py: the sampled dense-dense product with torch tensors.  torch initialises its HIP runtime before
the engine's library is loaded (as bench.py does).  Prints SDDMM_TORCH_OK <case> when every check passed."""
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

import exact  # noqa: E402
import sddmm_ref as sr  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402


def wrapped(ctx, tops):
    """every pattern as wrap_csr over torch tensors (the values tensor NaN: never read), U, V and out wrapped torch tensors:
    bit for bit the int64 twin, for every k and scaling; SparseOperator.sddmm on top"""
    rng = np.random.default_rng(17)
    for name, (nrow, ncol, rp, col) in sr.patterns().items():
        t_rp, t_col = torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)
        t_val = torch.full((len(col),), float("nan"), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        A = ctx.wrap_csr(nrow, ncol, t_rp, t_col, t_val)
        op = tops.SparseOperator(ctx, A)
        for k in sr.KS:
            U, V, out0, e = sr.dyadic_inputs(rng, nrow, ncol, len(col), k)
            tU, tV = torch.from_numpy(U).to(dev), torch.from_numpy(V).to(dev)
            for alpha, beta in sr.SCALINGS:
                want = sr.sddmm_exact(rp, col, U, V, e, alpha, beta, out0)
                out = torch.from_numpy(out0).to(dev) if beta != 0.0 else torch.full((len(col),), float("nan"), dtype=torch.float64, device=dev)
                ctx.sddmm(A, ctx.wrap_vector(tU), ctx.wrap_vector(tV), k, ctx.wrap_vector(out), alpha=alpha, beta=beta)
                got = out.cpu().numpy()
                assert np.array_equal(got, want), f"{name} k={k} alpha={alpha} beta={beta}: {int(np.sum(got != want))} entries differ"
            fresh = op.sddmm(tU, tV)
            assert fresh.shape == (len(col),) and fresh.dtype == torch.float64 and fresh.device == dev
            assert np.array_equal(fresh.cpu().numpy(), sr.sddmm_exact(rp, col, U, V, e)), f"{name} k={k}: SparseOperator.sddmm"
            if k == 1:  # 1-D tensors mean k = 1
                assert torch.equal(op.sddmm(tU[:, 0].contiguous(), tV[:, 0].contiguous()), fresh)
        for bad in (lambda: op.sddmm(tU[:, :3], tV), lambda: op.sddmm(tU.float(), tV.float()), lambda: op.sddmm(tU[1:], tV)):
            try:
                bad()
            except ValueError:
                pass
            else:
                raise AssertionError("SparseOperator.sddmm took tensors it should refuse")


def gradients(ctx, tops):
    """loss = (W * Y).sum() with dyadic W, values, x / X on the 300 x 257 pattern: the gradients in values and in x / X against those
    torch computes for the same loss through a dense matrix built with index_put.  Every sum is exact, so: bit for bit"""
    nrow, ncol, rp, col = sr.patterns()["rand300x257"]
    rows = sr.entry_rows(rp)
    rng = np.random.default_rng(23)
    b, e = exact.choose_bits(terms=512)  # at most 300 two-factor products per gradient entry, 40 per output
    val = exact.dyadic(rng, len(col), b, e)
    A = ctx.csr(nrow, ncol, rp, col, val)
    op = tops.SparseOperator(ctx, A)
    t_rows, t_cols = torch.from_numpy(rows), torch.from_numpy(col.astype(np.int64))

    def dense_grads(Xh, Wh):
        v = torch.from_numpy(val).requires_grad_(True)
        X = torch.from_numpy(Xh).requires_grad_(True)
        dense = torch.zeros((nrow, ncol), dtype=torch.float64).index_put((t_rows, t_cols), v)
        Y = dense @ X
        (torch.from_numpy(Wh) * Y).sum().backward()
        return Y.detach(), v.grad, X.grad

    for k in (1, 5, 16):
        Xh, Wh = exact.dyadic(rng, (ncol, k), b, e), exact.dyadic(rng, (nrow, k), b, e)
        Yd, gv, gX = dense_grads(Xh, Wh)
        v = torch.from_numpy(val).to(dev).requires_grad_(True)
        X = torch.from_numpy(Xh).to(dev).requires_grad_(True)
        W = torch.from_numpy(Wh).to(dev)
        Y = tops.spmm(op, X, v)
        (W * Y).sum().backward()
        assert torch.equal(Y.detach().cpu(), Yd), f"spmm k={k}: forward"
        assert torch.equal(v.grad.cpu(), gv), f"spmm k={k}: gradient in values"
        assert torch.equal(X.grad.cpu(), gX), f"spmm k={k}: gradient in X"
        # without values: the same gradient in X, none for anything else
        X2 = torch.from_numpy(Xh).to(dev).requires_grad_(True)
        (W * tops.spmm(op, X2)).sum().backward()
        assert torch.equal(X2.grad, X.grad)
        # values alone
        v3 = torch.from_numpy(val).to(dev).requires_grad_(True)
        (W * tops.spmm(op, X.detach(), v3)).sum().backward()
        assert torch.equal(v3.grad, v.grad)
    assert getattr(op, "_At", None) is not None  # the transposed handle was built once, at the first backward, and kept

    xh, wh = exact.dyadic(rng, ncol, b, e), exact.dyadic(rng, nrow, b, e)
    Yd, gv, gx = dense_grads(xh.reshape(-1, 1), wh.reshape(-1, 1))
    v = torch.from_numpy(val).to(dev).requires_grad_(True)
    x = torch.from_numpy(xh).to(dev).requires_grad_(True)
    w = torch.from_numpy(wh).to(dev)
    y = tops.spmv(op, x, v)
    (w * y).sum().backward()
    assert torch.equal(y.detach().cpu(), Yd[:, 0]) and torch.equal(v.grad.cpu(), gv) and torch.equal(x.grad.cpu(), gx[:, 0])
    # without values spmv is what it was: dL/dx = A^T g from the transposed product
    x2 = torch.from_numpy(xh).to(dev).requires_grad_(True)
    y2 = tops.spmv(op, x2)
    (w * y2).sum().backward()
    assert torch.equal(y2.detach(), y.detach()) and torch.equal(x2.grad, op.rmatvec(w)) and torch.equal(x2.grad, x.grad)
    for bad in (v.detach()[:-1], v.detach().float(), v.detach().reshape(-1, 1)):
        try:
            tops.spmv(op, x, bad)
        except ValueError:
            pass
        else:
            raise AssertionError("spmv took a values tensor it should refuse")
    # a value update: a new operator over the same pattern and a torch tensor of values, nothing copied
    new_val = exact.dyadic(rng, len(col), b, e)
    t_new = torch.from_numpy(new_val).to(dev)
    torch.cuda.synchronize()
    op_new = tops.SparseOperator(ctx, ctx.csr_with_values(A, ctx.wrap_vector(t_new)))
    want = exact.exact_product(nrow, rows, col, new_val, xh, e)
    assert np.array_equal(tops.spmv(op_new, x.detach()).cpu().numpy(), want)


def perf(ctx, tops):
    """k = 8 on the banded 10M x 32 pattern: spmv_sddmm against torch's (U[rows] * V[cols]).sum(1) on the same tensors; medians of 3
    interleaved rounds.  Prints SDDMM_PERF <ours ms> <torch ms>"""
    n, per_row, k, band = 10_000_000, 32, 8, 65536
    g = torch.Generator(device=dev).manual_seed(5)
    rows = torch.arange(n, device=dev, dtype=torch.int32).repeat_interleave(per_row)
    cols = (rows + torch.randint(-band // 2, band // 2, (n * per_row,), device=dev, dtype=torch.int32, generator=g)).clamp_(0, n - 1)
    t_rp = torch.arange(0, n * per_row + 1, per_row, device=dev, dtype=torch.int32)
    U = torch.rand((n, k), dtype=torch.float64, device=dev, generator=g)
    V = torch.rand((n, k), dtype=torch.float64, device=dev, generator=g)
    out = torch.empty(n * per_row, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    A = ctx.wrap_csr(n, n, t_rp, cols, out)  # (a pattern: the values are never read, so they may be the output's storage)
    vU, vV, vO = ctx.wrap_vector(U), ctx.wrap_vector(V), ctx.wrap_vector(torch.empty_like(out))
    rows64, cols64 = rows.long(), cols.long()

    def torch_ms():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = (U[rows64] * V[cols64]).sum(1)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), r

    ctx.sddmm_timed(A, vU, vV, k, vO, 2)
    _, ref = torch_ms()
    ctx.sddmm(A, vU, vV, k, vO)
    torch.cuda.synchronize()
    got = vO._keep
    assert torch.allclose(got, ref, rtol=1e-13, atol=0.0)
    del ref, got
    ours, theirs = [], []
    for _ in range(3):
        ours.append(ctx.sddmm_timed(A, vU, vV, k, vO, 5))
        theirs.append(torch_ms()[0])
    print(f"SDDMM_PERF {float(np.median(ours)):.4f} {float(np.median(theirs)):.4f}")


if __name__ == "__main__":
    case = sys.argv[1]
    pkg = load_package()
    tops = importlib.import_module("arm_spmv_amd.torch_ops")
    ctx = tops.context_on_current_stream(0)
    {"wrapped": wrapped, "gradients": gradients, "perf": perf}[case](ctx, tops)
    torch.cuda.synchronize()
    ctx.close()
    print(f"SDDMM_TORCH_OK {case}")
