"""torch view of one engine handle: y = A x and x = A^T y on CUDA tensors, and an autograd function over them.

    ctx = torch_ops.context_on_current_stream()          # the engine on torch's current stream
    op  = torch_ops.SparseOperator(ctx, ctx.csr(nrow, ncol, row_ptr, col, val))
    y   = torch_ops.spmv(op, x)                          # x.requires_grad: backward computes A^T grad (spmv_apply_transpose)

Vectors are 1-D, contiguous, float64 tensors on the context's device; they are wrapped, not copied (capi.Context.wrap_vector).
The context must run on torch's current stream: the products are then ordered with torch's own work on that stream, and the
outputs (allocated by torch) need no synchronisation.  There is no gradient with respect to the matrix values.
"""
from __future__ import annotations

import torch

from . import capi


def context_on_current_stream(device: int | None = None) -> "capi.Context":
    """an engine context on torch's current stream of `device` (default: the current device)"""
    dev = torch.cuda.current_device() if device is None else device
    return capi.Context(dev, stream=torch.cuda.current_stream(dev).cuda_stream)


class SparseOperator:
    """A (nrow x ncol) of a capi.Matrix: matvec(x) = A x, rmatvec(y) = A^T y, lstsq(b) = argmin ||b - A x||, solve(b) = A^-1 b (square A), each
    into a fresh tensor"""

    def __init__(self, ctx: "capi.Context", A: "capi.Matrix"):
        self.ctx, self.A = ctx, A
        info = A.info
        self.shape = (int(info.nrow), int(info.ncol))
        self.device = torch.device("cuda", ctx.device)

    def _check(self, t: torch.Tensor, n: int, what: str) -> None:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.dim() != 1 or not t.is_contiguous() or t.device != self.device:
            raise ValueError(f"{what}: a 1-D contiguous float64 tensor on {self.device}")
        if t.numel() != n:
            raise ValueError(f"{what}: {t.numel()} entries, expected {n}")

    def matvec(self, x: torch.Tensor) -> torch.Tensor:
        nrow, ncol = self.shape
        self._check(x, ncol, "matvec")
        y = torch.zeros(nrow, dtype=torch.float64, device=self.device)
        self.ctx.apply(self.A, self.ctx.wrap_vector(x), self.ctx.wrap_vector(y))
        return y

    def rmatvec(self, y: torch.Tensor) -> torch.Tensor:
        nrow, ncol = self.shape
        self._check(y, nrow, "rmatvec")
        x = torch.zeros(ncol, dtype=torch.float64, device=self.device)
        self.ctx.apply_transpose(self.A, self.ctx.wrap_vector(y), self.ctx.wrap_vector(x))
        return x

    def lstsq(self, b: torch.Tensor, x0: torch.Tensor | None = None, **kw) -> torch.Tensor:
        """argmin ||b - A x||^2 + damp^2 ||x||^2 by capi.Context.cgls from x0 (default 0), into a fresh tensor; kw: max_iter, rel_tol,
        check_every, damp.  (iterations, normal residual, residual) of the solve are left in self.last_lstsq.  No autograd through
        the solve"""
        nrow, ncol = self.shape
        self._check(b, nrow, "lstsq")
        if x0 is None:
            x = torch.zeros(ncol, dtype=torch.float64, device=self.device)
        else:
            self._check(x0, ncol, "lstsq x0")
            x = x0.detach().clone()
        self.last_lstsq = self.ctx.cgls(self.A, self.ctx.wrap_vector(b.detach()), self.ctx.wrap_vector(x), **kw)
        return x


    def solve(self, b: torch.Tensor, x0: torch.Tensor | None = None, method: str = "bicgstab", **kw) -> torch.Tensor:
        """x with A x = b for a square A from x0 (default 0), into a fresh tensor, by capi.Context.bicgstab (method="bicgstab", the
        default) or capi.Context.gmres (method="gmres"; kw: restart as well); kw: max_iter, rel_tol, check_every, precond.
        (iterations, residual) of the solve are left in self.last_solve.  No autograd through the solve.
        precond=capi.PRECOND_ILU0 preconditions with the ILU(0) factors of a CSR operator (set up on the first solve)"""
        if method not in ("bicgstab", "gmres"):
            raise ValueError(f"solve: method {method!r}, expected 'bicgstab' or 'gmres'")
        if method == "bicgstab" and "restart" in kw:
            raise ValueError("solve: restart belongs to method='gmres'")
        nrow, ncol = self.shape
        if nrow != ncol:
            raise ValueError(f"solve: the operator is {nrow} x {ncol}, not square (lstsq takes any shape)")
        self._check(b, nrow, "solve")
        if x0 is None:
            x = torch.zeros(ncol, dtype=torch.float64, device=self.device)
        else:
            self._check(x0, ncol, "solve x0")
            x = x0.detach().clone()
        run = self.ctx.gmres if method == "gmres" else self.ctx.bicgstab
        self.last_solve = run(self.A, self.ctx.wrap_vector(b.detach()), self.ctx.wrap_vector(x), **kw)
        return x

    def solve_symmetric(self, b: torch.Tensor, x0: torch.Tensor | None = None, shift: float = 0.0, M: "capi.Matrix | None" = None, **kw) -> torch.Tensor:
        """x with (A - shift I) x = b for a square symmetric A that need not be positive definite, from x0 (default 0), into a fresh
        tensor, by capi.Context.minres; M: the handle the preconditioner is built from (None: A); kw: max_iter, rel_tol, check_every,
        precond.  (iterations, residual) of the solve are left in self.last_solve.  No autograd through the solve"""
        nrow, ncol = self.shape
        if nrow != ncol:
            raise ValueError(f"solve_symmetric: the operator is {nrow} x {ncol}, not square (lstsq takes any shape)")
        self._check(b, nrow, "solve_symmetric")
        if x0 is None:
            x = torch.zeros(ncol, dtype=torch.float64, device=self.device)
        else:
            self._check(x0, ncol, "solve_symmetric x0")
            x = x0.detach().clone()
        self.last_solve = self.ctx.minres(self.A, self.ctx.wrap_vector(b.detach()), self.ctx.wrap_vector(x), shift=shift, P=M, **kw)
        return x

class _SpMV(torch.autograd.Function):
    @staticmethod
    def forward(fctx, op: SparseOperator, x: torch.Tensor) -> torch.Tensor:
        fctx.op = op
        return op.matvec(x)

    @staticmethod
    def backward(fctx, grad: torch.Tensor):
        return None, fctx.op.rmatvec(grad.contiguous())


def spmv(op: SparseOperator, x: torch.Tensor) -> torch.Tensor:
    """A x, differentiable in x (dL/dx = A^T dL/dy)"""
    return _SpMV.apply(op, x)
