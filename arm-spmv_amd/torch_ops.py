"""torch view of one engine handle: y = A x and x = A^T y on CUDA tensors, and an autograd function over them.

    ctx = torch_ops.context_on_current_stream()          # the engine on torch's current stream
    op  = torch_ops.SparseOperator(ctx, ctx.csr(nrow, ncol, row_ptr, col, val))
    y   = torch_ops.spmv(op, x)                          # x.requires_grad: backward computes A^T grad (spmv_apply_transpose)

Vectors are 1-D, contiguous, float64 tensors on the context's device; they are wrapped, not copied (capi.Context.wrap_vector).
The context must run on torch's current stream: the products are then ordered with torch's own work on that stream, and the
outputs (allocated by torch) need no synchronisation.

Gradients with respect to the matrix VALUES come from the sampled dense-dense product (capi.Context.sddmm): pass the values as a
tensor, spmv(op, x, values) or spmm(op, X, values), and dL/dvalues[e] = grad[row(e), :] . x[col(e), :] on the operator's pattern.
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

    def _check2(self, t: torch.Tensor, n: int, what: str) -> int:
        """a (n, k) contiguous float64 tensor on the operator's device, or a 1-D one of n entries (k = 1); returns k"""
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.dim() not in (1, 2) or not t.is_contiguous() or t.device != self.device:
            raise ValueError(f"{what}: a 2-D (or 1-D) contiguous float64 tensor on {self.device}")
        if t.shape[0] != n:
            raise ValueError(f"{what}: {t.shape[0]} rows, expected {n}")
        k = 1 if t.dim() == 1 else int(t.shape[1])
        if not 1 <= k <= 64:
            raise ValueError(f"{what}: {k} columns, expected 1 .. 64")
        return k

    @property
    def nnz(self) -> int:
        return int(self.A.info.nnz)

    def matmat(self, X: torch.Tensor) -> torch.Tensor:
        """A X for a (ncol, k) tensor (capi.Context.apply_multi), into a fresh (nrow, k) tensor"""
        nrow, ncol = self.shape
        k = self._check2(X, ncol, "matmat")
        Y = torch.empty((nrow, k), dtype=torch.float64, device=self.device)
        self.ctx.apply_multi(self.A, self.ctx.wrap_vector(X), self.ctx.wrap_vector(Y), k, overwrite=True)
        return Y

    def rmatmat(self, G: torch.Tensor) -> torch.Tensor:
        """A^T G for a (nrow, k) tensor, into a fresh (ncol, k) tensor: the product of a transposed CSR handle (capi.Context.csr_transpose)
        that is built at the first call and kept on the operator"""
        nrow, ncol = self.shape
        k = self._check2(G, nrow, "rmatmat")
        if getattr(self, "_At", None) is None:
            self._At = self.ctx.csr_transpose(self.A)
        X = torch.empty((ncol, k), dtype=torch.float64, device=self.device)
        self.ctx.apply_multi(self._At, self.ctx.wrap_vector(G), self.ctx.wrap_vector(X), k, overwrite=True)
        return X

    def sddmm(self, U: torch.Tensor, V: torch.Tensor) -> torch.Tensor:
        """U[row(e), :] . V[col(e), :] for every stored entry e of the operator's CSR pattern (capi.Context.sddmm), into a fresh tensor
        of nnz entries in the handle's entry order.  U is (nrow, k), V (ncol, k), contiguous float64; 1-D tensors mean k = 1.  The
        operator's own values take no part"""
        nrow, ncol = self.shape
        k = self._check2(U, nrow, "sddmm U")
        if self._check2(V, ncol, "sddmm V") != k:
            raise ValueError(f"sddmm: U has {k} columns, V {1 if V.dim() == 1 else V.shape[1]}")
        out = torch.empty(self.nnz, dtype=torch.float64, device=self.device)
        self.ctx.sddmm(self.A, self.ctx.wrap_vector(U), self.ctx.wrap_vector(V), k, self.ctx.wrap_vector(out))
        return out

    def _check_values(self, values: torch.Tensor, what: str) -> None:
        self._check(values, self.nnz, f"{what} values")


class _SpMV(torch.autograd.Function):
    @staticmethod
    def forward(fctx, op: SparseOperator, x: torch.Tensor) -> torch.Tensor:
        fctx.op = op
        return op.matvec(x)

    @staticmethod
    def backward(fctx, grad: torch.Tensor):
        return None, fctx.op.rmatvec(grad.contiguous())


class _SpMVValues(torch.autograd.Function):
    """y = A x with the values of A as a third argument: the forward product runs from the handle, the backward adds
    dL/dvalues = sddmm(pattern; grad, x)"""

    @staticmethod
    def forward(fctx, op: SparseOperator, x: torch.Tensor, values: torch.Tensor) -> torch.Tensor:
        fctx.op = op
        fctx.save_for_backward(x)
        return op.matvec(x)

    @staticmethod
    def backward(fctx, grad: torch.Tensor):
        (x,) = fctx.saved_tensors
        grad = grad.contiguous()
        dx = fctx.op.rmatvec(grad) if fctx.needs_input_grad[1] else None
        dv = fctx.op.sddmm(grad, x) if fctx.needs_input_grad[2] else None
        return None, dx, dv


class _SpMM(torch.autograd.Function):
    @staticmethod
    def forward(fctx, op: SparseOperator, X: torch.Tensor, values: torch.Tensor | None) -> torch.Tensor:
        fctx.op = op
        fctx.save_for_backward(X)
        return op.matmat(X)

    @staticmethod
    def backward(fctx, grad: torch.Tensor):
        (X,) = fctx.saved_tensors
        grad = grad.contiguous()
        dX = fctx.op.rmatmat(grad) if fctx.needs_input_grad[1] else None
        dv = fctx.op.sddmm(grad, X) if fctx.needs_input_grad[2] else None
        return None, dX, dv


def spmv(op: SparseOperator, x: torch.Tensor, values: torch.Tensor | None = None) -> torch.Tensor:
    """A x, differentiable in x (dL/dx = A^T dL/dy).

    With `values` (a 1-D float64 tensor of nnz entries in the handle's CSR entry order) the result is differentiable in the values
    too: dL/dvalues[e] = dL/dy[row(e)] * x[col(e)], the sampled product on the operator's pattern (CSR operators).  `values` is the
    caller's statement of what the handle holds: the forward product still runs from the HANDLE, whose set-up may have copied its
    values into layouts of its own, so changing `values` in place does not change the operator.  Build a new operator per value
    update, without a copy: SparseOperator(ctx, ctx.csr_with_values(A, ctx.wrap_vector(values)))"""
    if values is None:
        return _SpMV.apply(op, x)
    op._check_values(values, "spmv")
    return _SpMVValues.apply(op, x, values)


def spmm(op: SparseOperator, X: torch.Tensor, values: torch.Tensor | None = None) -> torch.Tensor:
    """A X for a contiguous float64 (ncol, k) tensor, 1 <= k <= 64 (CSR and ELL operators), differentiable in X: dL/dX = A^T dL/dY
    through a transposed CSR handle built at the first backward and kept on the operator (CSR operators).

    With `values` the result is differentiable in the values as well, dL/dvalues[e] = dL/dY[row(e), :] . X[col(e), :]; what
    spmv says about `values` holds here too"""
    if values is not None:
        op._check_values(values, "spmm")
    return _SpMM.apply(op, X, values)
