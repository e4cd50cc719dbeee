"""Child process of tests/test_gpu_sharded.py (GPU box only): every rank's LOCAL operations of the sharded solver step.

    python child_sharded_ops.py WORLD N

No process group: the child loops over the ranks of a world of WORLD, builds rank r's shard of an N x N matrix (twice: from host
arrays with csr_shard, and with extract_rows from the whole device handle), puts a dist.HipShardOps on it and calls every method
with torch tensors - against the integer references of tests/sharded_ref.py, bit for bit, on inputs whose unread entries are
NaN / +-inf and outputs that are NaN beforehand.  The Gauss-Seidel sweep of the rank's diagonal block is held to the oracle's
sweep in the sequence the engine reports, within the gate of the single-device sweep tests.  Stops at the first failed check
with a line naming world, rank and operation, and a nonzero exit."""
import collections
import importlib
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

KERNEL_NAMES = {1: "vector", 2: "ldswin", 3: "scalar", 4: "panel", 5: "twophase", 6: "segscan", 7: "split", 8: "ell"}
WHERE = {"world": None, "how": "", "rank": None, "op": ""}
SEEN = collections.defaultdict(collections.Counter)  # operation -> kernel that ran -> calls (handles with entries only)


class Failed(Exception):
    pass


def at(rank, op):
    WHERE["rank"], WHERE["op"] = rank, op


def check(cond, msg=""):
    if not cond:
        raise Failed(msg() if callable(msg) else msg)


def differ(got, want):
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want)))) if got.shape == want.shape else np.zeros(0, int)
    if got.shape != want.shape:
        return f"shape {got.shape}, want {want.shape}"
    i = int(bad[0]) if bad.size else -1
    return f"{bad.size} of {got.size} entries differ; first {i}: got {got[i]!r}, want {want[i]!r}" if bad.size else "equal"


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    check(got.shape == want.shape and np.array_equal(got, want), lambda: f"{what}: {differ(got, want)}")


def main():
    world, n = int(sys.argv[1]), int(sys.argv[2])
    WHERE["world"] = world
    torch.cuda.init()  # torch's HIP runtime first, then the engine (same order as bench.py)
    dev = torch.device("cuda", 0)
    from __graft_entry__ import load_package

    import exact as ex
    import oracle_lib as ol
    import sharded_ref as sr
    from test_gpu_solver import _spd_random, _symgs_close

    pkg = load_package()
    capi = pkg.capi
    dmod = importlib.import_module("arm_spmv_amd.dist")
    orc = ol.load_oracle()
    ctx = capi.Context(0)

    def T(a):  # a host array as a device tensor of torch's
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
        torch.cuda.synchronize()
        return t

    def nans(m):
        t = torch.full((m,), float("nan"), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        return t

    def host(t):
        ctx.sync()
        return t.cpu().numpy()

    def build(how, whole, rp, cc, cv, lo, hi):
        if how == "csr_shard":
            return ctx.csr_shard(lo, hi, n, rp, cc, cv)
        return ctx.extract_rows(whole, lo, hi)

    def record(op, A):
        if A.info.nnz > 0:
            SEEN[op][KERNEL_NAMES.get(A.info.kernel, str(A.info.kernel))] += 1

    try:
        P = sr.OpsProblem(n, world)
        check(P.bounds == [tuple(dmod.shard_rows(n, world, r)) for r in range(world)], "row bounds")
        _, srp_, scc_, scv_ = _spd_random(n, 6, 9)  # symmetric, strictly diagonally dominant: the sweep's matrix
        outside_entries = 0
        for how in ("csr_shard", "extract_rows"):
            WHERE["how"] = how
            at(None, "upload of the whole matrix")
            whole = ctx.csr(n, n, P.rp.astype(np.int32), P.cc, P.cv)
            whole_s = ctx.csr(n, n, srp_, scc_, scv_)
            partial_sum = np.zeros(n)
            for r, (lo, hi) in enumerate(P.bounds):
                own = hi - lo
                srp, scol, sval = P.shard(r)
                at(r, "shard")
                A = build(how, whole, P.rp, P.cc, P.cv, lo, hi)
                A.validate()
                i = A.info
                check((i.nrow, i.ncol, i.nnz, i.row_begin) == (own, n, len(scol), lo), lambda: f"info {(i.nrow, i.ncol, i.nnz, i.row_begin)}")
                rp_d, cc_d, cv_d = A.download()
                same(rp_d, srp, "row_ptr"), same(cc_d, scol, "col"), same(cv_d, sval, "val")
                ops = dmod.HipShardOps(ctx, A)
                want_q, want_dot = P.want_product(r)
                w_own = T(P.w[lo:hi])

                # ---- product_dot under the handle's own choice and three forced kernels
                p_full = T(ex.poison(P.p, scol))
                for kernel in (capi.CSR_AUTO, capi.CSR_SCALAR, capi.CSR_VECTOR, capi.CSR_PANEL):
                    at(r, f"product_dot kernel={KERNEL_NAMES.get(kernel, 'auto')}")
                    if kernel != capi.CSR_AUTO:
                        A.set_kernel(kernel)
                        check(A.info.kernel == kernel, "the forced kernel did not take")
                    q_own = nans(own)
                    d = ops.product_dot(p_full, w_own, q_own)
                    same(host(q_own), want_q, "q_own")
                    check(d == want_dot, lambda: f"dot {d!r}, exact {want_dot!r}")
                    record("product_dot", A)

                # ---- enable_overlap with the rank's own rows, and splits by other ranges
                at(r, "enable_overlap")
                ops.enable_overlap(lo, hi)
                t_in, t_out = sr.split_columns(srp, scol, sval, lo, hi)
                outside_entries += len(t_out[1])
                for part, twin, name in ((ops.A_in, t_in, "inside"), (ops.A_out, t_out, "outside")):
                    part.validate()
                    got = part.download()
                    for g, t, arr in zip(got, twin, ("row_ptr", "col", "val")):
                        same(g, t, f"{name} {arr}")
                ii, io = ops.A_in.info, ops.A_out.info
                check((ii.nrow, ii.ncol, ii.row_begin) == (own, own, 0), lambda: f"inside info {(ii.nrow, ii.ncol, ii.row_begin)}")
                check((io.nrow, io.ncol, io.row_begin) == (own, n, lo), lambda: f"outside info {(io.nrow, io.ncol, io.row_begin)}")
                check(ii.nnz + io.nnz == len(scol) and ii.nnz == len(t_in[1]), lambda: f"nnz {ii.nnz} + {io.nnz} of {len(scol)}")
                for c0, c1 in ((min(lo + 1, hi), hi), (lo, lo), (0, n)):
                    at(r, f"csr_split_columns [{c0}, {c1})")
                    B_in, B_out = ctx.csr_split_columns(A, c0, c1)
                    u_in, u_out = sr.split_columns(srp, scol, sval, c0, c1)
                    for part, twin, name in ((B_in, u_in, "inside"), (B_out, u_out, "outside")):
                        part.validate()
                        for g, t, arr in zip(part.download(), twin, ("row_ptr", "col", "val")):
                            same(g, t, f"{name} {arr}")
                    bi, bo = B_in.info, B_out.info
                    check((bi.nrow, bi.ncol, bi.row_begin) == (own, c1 - c0, lo - c0), lambda: f"inside info {(bi.nrow, bi.ncol, bi.row_begin)}")
                    check((bo.nrow, bo.ncol, bo.row_begin) == (own, n, lo), lambda: f"outside info {(bo.nrow, bo.ncol, bo.row_begin)}")
                    check(bi.nnz + bo.nnz == len(scol), "nnz")

                # ---- begin_local + finish_remote_dot: the same bits as product_dot
                p_own = T(ex.poison(P.p[lo:hi], t_in[1]))
                p_rest = T(ex.poison(P.p, t_out[1]))  # every column of the rank's own range is poison here
                for forced in (False, True):
                    at(r, "begin_local + finish_remote_dot" + (" kernel=panel on both parts" if forced else ""))
                    if forced:
                        for part in (ops.A_in, ops.A_out):
                            part.set_kernel(capi.CSR_PANEL)
                            check(part.info.kernel == capi.CSR_PANEL, "the forced kernel did not take")
                    q_own = nans(own)
                    ops.begin_local(p_own, q_own)
                    d = ops.finish_remote_dot(p_rest, w_own, q_own)
                    same(host(q_own), want_q, "q_own")
                    check(d == want_dot, lambda: f"dot {d!r}, exact {want_dot!r}")
                    record("begin_local", ops.A_in)
                    record("finish_remote_dot", ops.A_out)

                # ---- product_transpose: this rank's contribution to every column
                at(r, "product_transpose")
                x_own = T(ex.poison(P.x[lo:hi], np.flatnonzero(np.diff(srp) > 0)))
                partial = nans(n)
                ops.product_transpose(x_own, partial)
                got = host(partial)
                same(got, P.want_transpose(r), "partial_full")
                partial_sum += got

                # ---- axpby and dot on the rank's slices
                at(r, "axpby")
                u_own, v_own, out = T(P.u[lo:hi]), T(P.v[lo:hi]), nans(own)
                ops.axpby(P.ALPHA, u_own, P.BETA, v_own, out)
                same(host(out), P.want_axpby(lo, hi), "w")
                at(r, "dot")
                d = ops.dot(u_own, v_own)
                check(d == P.want_dot(lo, hi), lambda: f"dot {d!r}, exact {P.want_dot(lo, hi)!r}")
                ops.sync()

                # ---- enable_symgs + precondition on the diagonal block of the dominant matrix, in both sweep orders
                at(r, "enable_symgs")
                S = build(how, whole_s, srp_.astype(np.int64), scc_, scv_, lo, hi)
                gs = dmod.HipShardOps(ctx, S)
                gs.enable_symgs(lo, hi)
                b_in, _ = sr.split_columns(*sr.shard_arrays(srp_, scc_, scv_, lo, hi), lo, hi)
                check(gs.A_in.info.row_begin == 0 and gs.A_in.info.nrow == gs.A_in.info.ncol == own, "the block is not square from row 0")
                r_host = np.random.default_rng(500 + r).uniform(-1, 1, own)
                r_own = T(r_host)
                for order in (1, 0):
                    at(r, f"precondition symgs_order={order}")
                    if order == 0:
                        gs.A_in.set_param("symgs_order", 0)
                    seq = ctx.symgs_order(gs.A_in)
                    want_seq = ol.greedy_colour_order(orc, b_in[0], b_in[1])[2] if order == 1 else np.arange(own, dtype=np.int32)
                    same(seq, want_seq, "sweep sequence")
                    z_own = nans(own)
                    gs.precondition(r_own, z_own)
                    got = host(z_own)
                    want = np.zeros(own)
                    check(ol.symgs(orc, *b_in, r_host, want, 1, order=seq) == 0, "the oracle found no diagonal")
                    check(got.shape == want.shape and not np.any(np.isnan(got)), "NaN left in z_own")
                    if own:
                        _symgs_close(got, want, f"world {world} rank {r} order {order}")
            at(None, "rank-order sum of the transposed partials")
            same(partial_sum, P.want_transpose_whole(), "sum over the ranks of A_p^T x_p")
        at(None, "every kernel ran")
        for op in ("product_dot", "finish_remote_dot") if outside_entries else ("product_dot",):  # (one rank with rows: no outside part)
            check(SEEN[op]["panel"] > 0, lambda: f"the panel kernel never ran for {op}: {dict(SEEN[op])}")
        check({"scalar", "vector", "panel"} <= set(SEEN["product_dot"]), lambda: f"product_dot ran {dict(SEEN['product_dot'])}")
    except Exception as err:
        import traceback

        traceback.print_exc()
        print(f"SHARDED_OPS_FAIL world={WHERE['world']} n={n} shard={WHERE['how']} rank={WHERE['rank']} op={WHERE['op']}: "
              f"{type(err).__name__}: {err}", flush=True)
        sys.exit(1)
    kernels = " ".join(f"{op}={{{','.join(f'{k}:{c}' for k, c in sorted(SEEN[op].items()))}}}" for op in sorted(SEEN))
    print(f"SHARDED_OPS_OK world={world} n={n} ranks={world} kernels: {kernels}")


if __name__ == "__main__":
    main()
