#!/usr/bin/env python3
"""The bits of the four deterministic solves - spmv_cg_multi, spmv_cgls, spmv_bicgstab, spmv_gmres, whose sums use the last-ticket
pattern - on small systems, for an A/B of two builds of the library: a change on the host side of a solve must leave every one of
them byte for byte.

  SPMV_HIP_SO=<library> python tools/solver_bits.py dump OUT.npz [SOLVERS]
                                                run every case (of the comma-separated solvers, e.g. cgls,gmres) on that library
                                                (default: this tree's), store x, iters and the residuals of each
  python tools/solver_bits.py compare A.npz B.npz
                                                the same cases in both, every array byte-identical; exit 1 if not

Each dump in a process of its own.  The cases: the 5-point Laplacians on 33 x 33 and 25 x 29 points (1089 and 725 rows), a random
diagonally dominant system of 4097 rows (symmetric for cg_multi, with a skew part for the other two square solves) and n = 1; x and
b 16-byte aligned and 8 bytes past it (a wrapped pointer into a larger vector), so that both access widths run; every
preconditioner the solver takes; the host looking every iteration and every fourth; runs that end at max_iter (13 iterations,
rel_tol 0) and at rel_tol 1e-10; cg_multi at k = 3, 8 and 17 with a column of b zero from the start; cgls on a 33 x 17 system with
damp 0 and 0.5, under the forward SCALAR kernel and the row-grouped transposed copy (the CSC companion's own kernel adds into y
with atomics in arrival order: two solves of ONE build differ there); gmres with restart 3 (several restarts in 13 iterations) and 64.
Needs a GPU for `dump`; there is no fallback.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def laplacian_2d(mx, my):
    """(n, row_ptr, col, val) of the 5-point Laplacian on an mx x my grid, Dirichlet boundary, columns ascending"""
    n = mx * my
    idx = np.arange(n, dtype=np.int64).reshape(mx, my)
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [np.full(n, 4.0)]
    for lo, hi in ((idx[:, :-1], idx[:, 1:]), (idx[:-1, :], idx[1:, :])):
        rows += [lo.ravel(), hi.ravel()]
        cols += [hi.ravel(), lo.ravel()]
        vals += [np.full(lo.size, -1.0)] * 2
    return _csr(n, n, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals))


def _csr(nrow, ncol, r, c, v):
    o = np.argsort(r * ncol + c, kind="stable")
    r, c, v = r[o], c[o], v[o]
    return nrow, np.searchsorted(r, np.arange(nrow + 1)).astype(np.int32), c.astype(np.int32), v


def random_dominant(n, per_row, skew, seed):
    """a random matrix with `per_row` off-diagonal pairs (i, j), (j, i) per row, entries a and a * (1 - skew) (skew 0: symmetric),
    and a diagonal above the absolute row sums: positive definite at skew 0"""
    rng = np.random.default_rng(seed)
    i = np.repeat(np.arange(n, dtype=np.int64), per_row)
    j = rng.integers(0, n, size=i.size)
    keep = i != j
    i, j = i[keep], j[keep]
    key, first = np.unique(np.minimum(i, j) * n + np.maximum(i, j), return_index=True)  # one pair per position
    i, j = i[first], j[first]
    a = rng.uniform(-1.0, 1.0, size=i.size)
    rows, cols, vals = np.concatenate([i, j]), np.concatenate([j, i]), np.concatenate([a, a * (1.0 - skew)])
    diag = np.zeros(n)
    np.add.at(diag, rows, np.abs(vals))
    d = np.arange(n, dtype=np.int64)
    return _csr(n, n, np.concatenate([rows, d]), np.concatenate([cols, d]), np.concatenate([vals, diag + 1.0 + rng.uniform(0.0, 1.0, n)]))


def random_rect(nrow, ncol, per_row, seed):
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(nrow, dtype=np.int64), per_row)
    c = np.concatenate([rng.choice(ncol, size=per_row, replace=False) for _ in range(nrow)]).astype(np.int64)
    return _csr(nrow, ncol, r, c, rng.uniform(-1.0, 1.0, size=r.size))


def dump(out, solvers):
    from __graft_entry__ import load_package

    capi = load_package().capi
    ctx = capi.Context(0)
    rng = np.random.default_rng(2024)
    results = {}

    def vectors(host, offset):
        """a device vector with `host` in it, 16-byte aligned (offset 0) or 8 bytes past it (offset 1: wrapped into a larger one)"""
        if not offset:
            return ctx.vector_from(host), None
        whole = ctx.vector(host.size + 1)
        whole.fill(0.0)
        v = ctx.wrap_vector(whole.device_ptr + 8, host.size)
        v.upload(host)
        return v, whole

    def run(name, solve, A, b_host, nx):
        if solvers and name.split("/")[0] not in solvers:
            return
        for offset in (0, 1):
            for every in (1, 4):
                for end, (max_iter, rel_tol) in (("max_iter", (13, 0.0)), ("rel_tol", (400, 1e-10))):
                    b, keep_b = vectors(b_host, offset)
                    x, keep_x = vectors(np.zeros(nx), offset)
                    try:
                        outs = solve(A, b, x, max_iter, rel_tol, every)
                    except capi.SpmvError as e:  # a breakdown is a result too: the same words from both builds
                        outs = (np.frombuffer(str(e).encode(), dtype=np.uint8),)
                    ctx.sync()
                    key = f"{name}/offset{8 * offset}/every{every}/{end}"
                    results[key + "/x"] = x.download()
                    for i, o in enumerate(outs):
                        results[f"{key}/out{i}"] = np.asarray(o)
                    del b, x, keep_b, keep_x

    square = {
        "lap33": (laplacian_2d(33, 33), laplacian_2d(33, 33)),
        "lap725": (laplacian_2d(25, 29), laplacian_2d(25, 29)),
        "rand4097": (random_dominant(4097, 6, 0.0, 7), random_dominant(4097, 6, 0.6, 7)),
        "n1": ((1, np.array([0, 1], np.int32), np.array([0], np.int32), np.array([2.0])),) * 2,
    }
    for sysname, (spd, general) in square.items():
        n = spd[0]
        A_spd, A_gen = ctx.csr(n, n, *spd[1:]), ctx.csr(n, n, *general[1:])
        b_host = rng.uniform(-1.0, 1.0, n)
        for k in (3, 8, 17):
            B = rng.uniform(-1.0, 1.0, (n, k))
            B[:, 1] = 0.0  # a column frozen from the start
            for pc in (capi.PRECOND_NONE, capi.PRECOND_JACOBI):
                run(f"cg_multi/{sysname}/k{k}/precond{pc}", lambda A, b, x, mi, tol, ev: ctx.cg_multi(A, b, x, k, mi, tol, ev, precond=pc), A_spd,
                    B.ravel(), n * k)
        for pc in (capi.PRECOND_NONE, capi.PRECOND_JACOBI, capi.PRECOND_ILU0):
            run(f"bicgstab/{sysname}/precond{pc}", lambda A, b, x, mi, tol, ev: ctx.bicgstab(A, b, x, mi, tol, ev, precond=pc), A_gen, b_host, n)
            for restart in (3, 64):
                run(f"gmres/{sysname}/restart{restart}/precond{pc}", lambda A, b, x, mi, tol, ev: ctx.gmres(A, b, x, restart, mi, tol, ev, precond=pc),
                    A_gen, b_host, n)
    nr, rp, c, v = random_rect(33, 17, 5, 11)
    A_rect = ctx.csr(33, 17, rp, c, v)
    A_rect.set_kernel(capi.CSR_SCALAR)
    A_rect.set_param("transpose_kernel", capi.CSR_PANEL)  # the row-grouped copy: sums in a fixed order
    b_rect = rng.uniform(-1.0, 1.0, 33)
    for damp in (0.0, 0.5):
        run(f"cgls/r33x17/damp{damp}", lambda A, b, x, mi, tol, ev: ctx.cgls(A, b, x, mi, tol, ev, damp=damp), A_rect, b_rect, 17)
    np.savez(out, **results)
    print(f"{len(results)} arrays of {len(results) // 3}+ solves -> {out}  (library: {capi.LIB_PATH})")


def compare(a, b):
    A, B = np.load(a), np.load(b)
    if sorted(A.files) != sorted(B.files):
        print(f"the dumps hold different cases: {len(A.files)} and {len(B.files)} arrays")
        return 1
    differ = [k for k in A.files if A[k].dtype != B[k].dtype or A[k].tobytes() != B[k].tobytes()]
    for k in differ[:20]:
        print(f"DIFFERS {k}: max |a - b| = {np.max(np.abs(A[k].astype(np.float64) - B[k].astype(np.float64))):.3e}")
    per_solver = {}
    for k in A.files:
        per_solver[k.split("/")[0]] = per_solver.get(k.split("/")[0], 0) + 1
    print(f"{len(A.files)} arrays ({', '.join(f'{s} {m}' for s, m in sorted(per_solver.items()))}): "
          + ("all byte-identical" if not differ else f"{len(differ)} differ"))
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) in (3, 4) and sys.argv[1] == "dump":
        dump(sys.argv[2], sys.argv[3].split(",") if len(sys.argv) == 4 else [])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
