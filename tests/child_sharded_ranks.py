"""Child of tests/test_gpu_sharded.py (GPU box only): the sharded solver step on real shards, three ranks over gloo on ONE GPU.

    python -m torch.distributed.run --nproc-per-node 3 child_sharded_ranks.py

Every rank builds its own shard (csr_shard), puts a dist.HipShardOps on it and runs dist.cg_sharded - plain, overlapped
(enable_overlap) and preconditioned (enable_symgs, both sweep orders) - at n = 6001 (ragged slices: the broadcast path of the
all-gather) and n = 6000 (equal slices: all_gather_into_tensor), with CUDA tensors over gloo (the staging branches of
allgather_x and reduce_transposed).  Plain and overlapped are held to the single-device spmv_cg of the whole matrix (rank 0),
the preconditioned runs to the same cg_sharded over the same group with the oracle as local operations, swept in the
sequence the engine reports for the rank's block.  Then the transposed exchange on exact inputs: product_transpose +
reduce_transposed, default and ragged column bounds, bit for bit.  A failed check ends the rank with a line naming it; the
launcher then ends the others."""
import datetime
import importlib
import sys
from pathlib import Path

import numpy as np
import torch
import torch.distributed as dist

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

REL_TOL = 1e-9  # as tests/child_sharded_cg.py
TRUE_RESIDUAL, ITER_MARGIN, SOLUTION_MARGIN = 2e-8, 2, 1e-7  # the margins child_sharded_cg.py uses at this tolerance
WHERE = {"what": "start"}


def check(cond, msg):
    if not cond:
        raise AssertionError(msg() if callable(msg) else msg)


def main():
    torch.cuda.init()  # torch's HIP runtime first, then the engine (same order as bench.py)
    dev = torch.device("cuda", 0)  # every rank on the one GPU
    from __graft_entry__ import load_package

    import exact as ex
    import oracle_lib as ol
    import sharded_ref as sr
    from test_dist_gloo import _OracleOps
    from test_gpu_solver import _spd_random

    class OrderedOracleOps(_OracleOps):
        """the CPU twin of HipShardOps with the sweep run in a given sequence (the one the engine reports for this block)"""

        order = None

        def _precondition(self, r_own, z_own):
            z = z_own.numpy()
            z[:] = 0.0
            assert self.ol.symgs(self.orc, *self.m_in, r_own.numpy(), z, self._gs_sweeps, order=self.order) == 0

    pkg = load_package()
    dmod = importlib.import_module("arm_spmv_amd.dist")
    orc = ol.load_oracle()
    ctx = pkg.capi.Context(0)
    dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=90))  # short: a rank that dies ends the others
    rank, world = dist.get_rank(), dist.get_world_size()
    report = []

    def agreed(value, what):
        """every rank holds the same value"""
        got = [None] * world
        dist.all_gather_object(got, value)
        check(all(g == got[0] for g in got), lambda: f"{what}: the ranks disagree: {got}")

    def solve(ops, b_host, lo, hi, n, cpu=False):
        b_t = torch.from_numpy(b_host[lo:hi].copy())
        x_t = torch.zeros(hi - lo, dtype=torch.float64)
        if not cpu:
            b_t, x_t = b_t.to(dev), x_t.to(dev)
            torch.cuda.synchronize()
        iters, relres = dmod.cg_sharded(ops, b_t, x_t, n, max_iter=500, rel_tol=REL_TOL)
        if not cpu:
            ctx.sync()
        sol = dmod.concatenate_y(x_t, n).cpu().numpy()  # (a CUDA tensor over gloo: the all-gather's staging branch)
        agreed((iters, relres), f"{WHERE['what']}: (iterations, residual)")
        agreed(sol.tobytes(), f"{WHERE['what']}: the gathered solution")
        return iters, relres, sol

    try:
        for n in (6001, 6000):
            n, rp, cc, cv = _spd_random(n, 6, 9)
            lo, hi = dmod.shard_rows(n, world, rank)
            b_host = np.random.default_rng(3).uniform(-1, 1, n)
            b_norm = np.linalg.norm(b_host)

            def true_residual(sol):
                ax = np.zeros(n)
                ol.csr_spmv(orc, rp, cc, cv, sol, ax)
                return float(np.linalg.norm(b_host - ax) / b_norm)

            def shard():
                A = ctx.csr_shard(lo, hi, n, rp.astype(np.int64), cc, cv)
                i = A.info
                check((i.nrow, i.ncol, i.row_begin) == (hi - lo, n, lo), f"shard info {(i.nrow, i.ncol, i.row_begin)}")
                return A

            # the single-device solve of the whole matrix (rank 0 computes, every rank receives)
            WHERE["what"] = f"n={n} single-device cg"
            single = [None]
            if rank == 0:
                A_whole = ctx.csr(n, n, rp, cc, cv)
                x1 = ctx.vector(n)
                x1.fill(0.0)
                it1, _ = ctx.cg(A_whole, ctx.vector_from(b_host), x1, max_iter=500, rel_tol=REL_TOL)
                single = [(it1, x1.download())]
            dist.broadcast_object_list(single, src=0)
            it1, sol1 = single[0]

            for variant in ("plain", "overlapped"):
                WHERE["what"] = f"n={n} {variant} cg_sharded"
                ops = dmod.HipShardOps(ctx, shard())
                if variant == "overlapped":
                    ops.enable_overlap(lo, hi)
                    check(ops.A_out.info.nnz > 0 and ops.A_in.info.nnz > 0, "both parts of the split hold entries")
                iters, relres, sol = solve(ops, b_host, lo, hi, n)
                res = true_residual(sol)
                check(relres <= REL_TOL and res <= TRUE_RESIDUAL, lambda: f"residual {relres:.3e}, true {res:.3e}")
                check(abs(iters - it1) <= ITER_MARGIN, lambda: f"{iters} iterations, single device {it1}")
                dev_ = float(np.max(np.abs(sol - sol1)) / np.max(np.abs(sol1)))
                check(dev_ <= SOLUTION_MARGIN, lambda: f"solution {dev_:.3e} from the single-device one")
                report.append(f"n={n} {variant}: {iters} iterations (single device {it1}), true residual {res:.2e}, solution {dev_:.1e}")

            for order in (1, 0):
                WHERE["what"] = f"n={n} preconditioned cg_sharded symgs_order={order}"
                ops = dmod.HipShardOps(ctx, shard())
                ops.enable_overlap(lo, hi)
                ops.A_in.set_param("symgs_order", order)
                ops.enable_symgs(lo, hi)
                ops.use_overlap = False
                seq = ctx.symgs_order(ops.A_in)
                iters, relres, sol = solve(ops, b_host, lo, hi, n)
                res = true_residual(sol)
                check(relres <= REL_TOL and res <= TRUE_RESIDUAL, lambda: f"residual {relres:.3e}, true {res:.3e}")
                # the twin: the same recurrence over the same group, the oracle's product and sweep on CPU tensors
                WHERE["what"] += " (the oracle twin)"
                twin = OrderedOracleOps(orc, ol, *sr.shard_arrays(rp, cc, cv, lo, hi))
                twin.order = seq
                twin.enable_symgs(lo, hi)
                it_t, relres_t, sol_t = solve(twin, b_host, lo, hi, n, cpu=True)
                check(relres_t <= REL_TOL, lambda: f"the twin's residual {relres_t:.3e}")
                check(abs(iters - it_t) <= ITER_MARGIN, lambda: f"{iters} iterations, the twin {it_t}")
                dev_ = float(np.max(np.abs(sol - sol_t)) / np.max(np.abs(sol_t)))
                check(dev_ <= SOLUTION_MARGIN, lambda: f"solution {dev_:.3e} from the twin's")
                check(iters < it1, lambda: f"the sweep saved nothing: {iters} iterations, plain {it1}")
                report.append(f"n={n} symgs_order={order}: {iters} iterations (twin {it_t}), true residual {res:.2e}, solution {dev_:.1e}")

        # ---- the transposed exchange on exact inputs
        P = sr.OpsProblem(sr.N_OPS, world)
        lo, hi = P.bounds[rank]
        srp, scol, sval = P.shard(rank)
        want = P.want_transpose_whole(P.y0)
        for bounds in (None, list(sr.RAGGED_COLUMNS)):
            WHERE["what"] = f"reduce_transposed bounds={'default' if bounds is None else bounds}"
            c0, c1 = P.bounds[rank] if bounds is None else bounds[rank]
            ops = dmod.HipShardOps(ctx, ctx.csr_shard(lo, hi, P.n, P.rp, P.cc, P.cv))
            x_own = torch.from_numpy(ex.poison(P.x[lo:hi], np.flatnonzero(np.diff(srp) > 0))).to(dev)
            partial = torch.full((P.n,), float("nan"), dtype=torch.float64, device=dev)
            y_own = torch.from_numpy(P.y0[c0:c1].copy()).to(dev)
            torch.cuda.synchronize()
            ops.product_transpose(x_own, partial)
            ops.sync()  # the exchange runs on torch's stream
            check(np.array_equal(partial.cpu().numpy(), P.want_transpose(rank)), "partial_full differs from the exact A_p^T x_p")
            dmod.reduce_transposed(partial, y_own, P.n, bounds=bounds)
            got = y_own.cpu().numpy()
            check(np.array_equal(got, want[c0:c1]), lambda: f"y_own differs from the exact slice [{c0}, {c1}) of y0 + A^T x in "
                  f"{int(np.sum(got != want[c0:c1]))} entries")
            agreed(True, WHERE["what"])
        dist.barrier()
    except Exception as err:
        import traceback

        traceback.print_exc()
        print(f"SHARDED_RANKS_FAIL rank={rank} at {WHERE['what']}: {type(err).__name__}: {err}", flush=True)
        sys.exit(1)
    if rank == 0:
        for line in report:
            print("SHARDED_RANKS", line)
        print(f"SHARDED_RANKS_OK world={world}", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
