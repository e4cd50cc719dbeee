"""spmv_lobpcg on the GPU (csrc/solver_lobpcg.hip): every problem of tests/lobpcg_ref.py, held to the outcome checks (a)-(d) of
lobpcg_ref.outcome_failures for its first nev columns and to the iteration count of the NumPy twin on the same problem and start:

    iters <= ceil(1.25 * twin) + 2

(the twin differs in rounding and in its small eigensolver, which act like a perturbation of the start block; such perturbations moved
the prototype's counts by at most 7 %).  The start block is spmv_gen_vec_uniform with seed 1 over n * k entries, whose NumPy twin is
synth.vec_uniform.  For the Chebyshev and AMG cases the twin's M^-1 is the engine's spmv_chebyshev_solve / spmv_amg_solve, column by
column: entry points older than the solver.  Exact eigenvalues: closed forms for the Laplacians, a dense solver for the 12 x 12 matrix,
Sturm bisection for the tridiagonal one.  With SPMV_LOBPCG_COUNTS=<file> the closing test writes both counts of every case there.
"""
import collections
import gc
import math
import os
import time

import numpy as np
import pytest

import lobpcg_ref as lr
import oracle_lib as ol

pytestmark = pytest.mark.gpu
AUTO, SCALAR = 0, 3
INVALID, UNSUPPORTED = -1, -5
RUNS = collections.Counter()
COUNTS = {}  # case -> (GPU iterations, twin iterations)
FORMATS = ("coo", "csc", "ell", "dia")
PRECOND_PROBLEMS = ("lap64_chebyshev", "lap64_amg", "lap64_amg_sa")
CSR_CASES = [(name, "auto") for name in lr.PROBLEMS if name not in PRECOND_PROBLEMS] + [(name, "scalar") for name in lr.LAPLACIANS]


def _handle(ctx, orc, E, fmt="csr"):
    n = E.n
    rp, cc, cv = E.csr()
    if fmt == "csr":
        return ctx.csr(n, n, rp, cc, cv)
    if fmt == "coo":
        o = np.random.default_rng(5).permutation(len(E.row))
        return ctx.coo(n, n, ol.i32(E.row[o]), ol.i32(E.col[o]), ol.f64(E.val[o]))
    if fmt == "csc":
        cp, cri, ccv = ol.coo_to_csc(orc, n, ol.i32(E.row), ol.i32(E.col), ol.f64(E.val))
        return ctx.csc(n, n, cp, cri, ccv)
    if fmt == "ell":
        k, ec, ev = ol.coo_to_ell(orc, n, ol.i32(E.row), ol.i32(E.col), ol.f64(E.val))
        return ctx.ell(n, n, k, len(E.val), ec, ev)
    offsets, dval = ol.csr_to_dia(orc, n, n, rp, cc, cv)
    return ctx.dia(n, n, offsets, dval)


def _start(ctx, pkg, name):
    """the start block on the device: generated there (and equal to its twin), or uploaded where the problem brings its own"""
    E, _, k = lr.problem(name)[:3]
    host = lr.start_block(name, pkg.synth.vec_uniform)
    if name == "diagonal_unit_start":
        return ctx.vector_from(np.ascontiguousarray(host.T).ravel())
    X = ctx.gen_vector(E.n * k, seed=1)
    assert np.array_equal(X.download(), np.ascontiguousarray(host.T).ravel()), "the device's start block is not its NumPy twin's"
    return X


def _solve_and_check(ctx, pkg, A, name, what, precond_code=None, twin_precond=None):
    capi = pkg.capi
    E, lam, k, nev, largest, tol, max_iter, pre = lr.problem(name)
    code = precond_code if precond_code is not None else (capi.PRECOND_JACOBI if pre == "jacobi" else capi.PRECOND_NONE)
    X = _start(ctx, pkg, name)
    theta, resid, iters = ctx.lobpcg(A, X, k, nev=nev, largest=largest, max_iter=max_iter, tol=tol, precond=code)
    Xh = X.download().reshape(k, E.n).T
    t_it = lr.twin(name, pkg.synth.vec_uniform, precond=twin_precond)[2]
    COUNTS[f"{name} {what}"] = (iters, t_it)
    print(f"{name} {what}: {iters} iterations (twin {t_it}), resid max {resid[:nev].max():.2e}, theta {theta[:nev]}")
    fails = lr.outcome_failures(E.matvec_ld, E.norm_inf(), Xh, theta, resid, nev, tol, lam, largest)
    assert fails == [], (name, what, fails, iters, resid, theta, lam[:k])
    assert iters <= math.ceil(1.25 * t_it) + 2, f"{name} {what}: {iters} iterations, the twin took {t_it}"
    if name == "diagonal_unit_start":
        assert iters == 0
    return theta, resid, iters, Xh


@pytest.mark.parametrize("name,kernel", CSR_CASES)
def test_problem_as_a_csr_handle(ctx, orc, pkg, name, kernel):
    A = _handle(ctx, orc, lr.problem(name)[0])
    if kernel == "scalar":
        A.set_kernel(SCALAR)
    _solve_and_check(ctx, pkg, A, name, f"csr {kernel}")
    RUNS["csr"] += 1


@pytest.mark.parametrize("fmt,name", list(zip(FORMATS, ("lap16_k4", "lap32_k8_nev6", "lap16_k1", "lap33_k5_multiple"))))
def test_laplacians_in_the_other_formats(ctx, orc, pkg, fmt, name):
    _solve_and_check(ctx, pkg, _handle(ctx, orc, lr.problem(name)[0], fmt), name, fmt)
    RUNS["formats"] += 1


@pytest.mark.parametrize("name", PRECOND_PROBLEMS)
def test_engine_preconditioners(ctx, orc, pkg, name):
    capi = pkg.capi
    E = lr.problem(name)[0]
    A = _handle(ctx, orc, E)
    if name == "lap64_chebyshev":
        ctx.chebyshev_setup(A, 4, True)  # what the solver's own set-up on first use would take
        code, apply = capi.PRECOND_CHEBYSHEV, ctx.chebyshev_solve
    else:
        (ctx.amg_setup_smoothed if name == "lap64_amg_sa" else ctx.amg_setup)(A)
        code, apply = capi.PRECOND_AMG, ctx.amg_solve
    r, z = ctx.vector(E.n), ctx.vector(E.n)

    def minv(v):
        r.upload(v)
        apply(A, r, z)
        ctx.sync()
        return z.download()

    _solve_and_check(ctx, pkg, A, name, "csr", precond_code=code, twin_precond=minv)
    RUNS["preconditioners"] += 1


def test_two_identical_solves_agree_bit_for_bit(ctx, orc, pkg):
    name = "lap16_k4"
    E, _, k, nev, largest, tol, max_iter, _ = lr.problem(name)
    A = _handle(ctx, orc, E)
    A.set_kernel(SCALAR)  # a product that adds in a fixed order: what is tested is the solver's own sums
    out = []
    for _ in range(2):
        X = _start(ctx, pkg, name)
        theta, resid, iters = ctx.lobpcg(A, X, k, max_iter=max_iter, tol=tol)
        out.append((X.download().tobytes(), theta.tobytes(), resid.tobytes(), iters))
    assert out[0] == out[1], "two calls on the same data differ"
    RUNS["bits"] += 1


def test_iteration_limits(ctx, orc, pkg):
    name = "lap16_k4"
    E, lam, k, nev, _, tol, _, _ = lr.problem(name)
    A = _handle(ctx, orc, E)
    # max_iter = 0: the Rayleigh-Ritz of the start block
    X = _start(ctx, pkg, name)
    X0 = lr.start_block(name, pkg.synth.vec_uniform)
    theta, resid, iters = ctx.lobpcg(A, X, k, max_iter=0, tol=tol)
    Xh = X.download().reshape(k, E.n).T
    assert iters == 0
    assert np.max(np.abs(Xh.T @ Xh - np.eye(k))) <= 1e-12
    Q, _ = np.linalg.qr(X0)
    assert np.max(np.abs(Xh - Q @ (Q.T @ Xh))) <= 1e-12, "the vectors left the span of the start block"
    AX = np.column_stack([E.matvec(np.ascontiguousarray(Xh[:, j])) for j in range(k)])
    ritz = np.linalg.eigvalsh(Q.T @ np.column_stack([E.matvec(np.ascontiguousarray(Q[:, j])) for j in range(k)]))
    assert np.max(np.abs(theta - ritz)) <= 1e-12 * E.norm_inf() and np.all(np.diff(theta) >= 0)
    assert np.max(np.abs(np.linalg.norm(AX - Xh * theta[None, :], axis=0) - resid)) <= 1e-12 * E.norm_inf()
    # max_iter = 3: three iterations, no error, residuals above the tolerance
    X = _start(ctx, pkg, name)
    theta3, resid3, iters = ctx.lobpcg(A, X, k, max_iter=3, tol=tol)
    assert iters == 3 and np.all(resid3 > tol) and np.all(theta3 <= theta + 1e-12), (iters, resid3, theta3, theta)
    Xh = X.download().reshape(k, E.n).T
    assert "b" not in lr.outcome_failures(E.matvec_ld, E.norm_inf(), Xh, theta3, resid3, k, tol, lam)
    RUNS["limits"] += 1


def test_a_rank_deficient_start_block_is_refused(ctx, orc, pkg):
    name = "lap16_k4"
    E, _, k = lr.problem(name)[:3]
    A = _handle(ctx, orc, E)
    X0 = lr.start_block(name, pkg.synth.vec_uniform).copy()
    X0[:, 2] = X0[:, 0]
    X = ctx.vector_from(np.ascontiguousarray(X0.T).ravel())
    with pytest.raises(pkg.capi.SpmvError) as e:
        ctx.lobpcg(A, X, k)
    assert e.value.code == INVALID and "start block" in str(e.value), str(e.value)
    RUNS["rank"] += 1


def test_dependent_residual_columns_are_left_out(ctx, orc, pkg):
    """diag(1 .. 40) from x_0 = e_0 + 1e-3 e_5 and x_1 = e_1 + 1e-3 e_5: projected against X, both residuals point along e_5, the
    residual block has rank one, and the solve goes on with one column of W instead of refusing (tests/test_lobpcg_ref.py: the twin)"""
    E, lam = lr.diagonal(40)
    order = np.argsort(E.diagonal())
    X0 = np.zeros((40, 2))
    X0[order[0], 0] = X0[order[1], 1] = 1.0
    X0[order[5], :] = 1e-3
    X = ctx.vector_from(np.ascontiguousarray(X0.T).ravel())
    theta, resid, iters = ctx.lobpcg(_handle(ctx, orc, E), X, 2, max_iter=50, tol=1e-10)
    t_it = lr.lobpcg(E.matvec, X0, tol=1e-10, max_iter=50)[2]
    fails = lr.outcome_failures(E.matvec_ld, E.norm_inf(), X.download().reshape(2, 40).T, theta, resid, 2, 1e-10, lam)
    assert fails == [] and 1 <= iters <= math.ceil(1.25 * t_it) + 2, (fails, iters, t_it, theta, resid)
    RUNS["dependent"] += 1


@pytest.mark.parametrize("fmt", ("csr",) + FORMATS)
def test_a_solve_leaves_the_handle_and_the_device_memory_alone(ctx, orc, pkg, fmt):
    name = "lap16_k4"
    E, _, k, nev, _, tol, max_iter, _ = lr.problem(name)
    A = _handle(ctx, orc, E, fmt)
    X = _start(ctx, pkg, name)
    ctx.lobpcg(A, X, k, max_iter=2, tol=tol)  # (whatever a context allocates once on first use is there now)
    plan, kernel, info_bytes, param_bytes = A.get_plan(), A.info.kernel, A.info.device_bytes, A.get_param("device_bytes")
    gc.collect()
    ctx.sync()
    free0, _ = ctx.mem_info()
    theta, resid, iters = ctx.lobpcg(A, X, k, max_iter=max_iter, tol=tol)
    ctx.sync()
    free1, _ = ctx.mem_info()
    assert np.all(resid <= tol) and 0 <= iters < max_iter
    assert free1 == free0, f"{fmt}: {free0 - free1} bytes of device memory not returned"
    assert A.get_param("transpose_ready") == 0, f"{fmt}: the solve built the transposed state"
    assert A.get_plan() == plan, f"{fmt}: the solve changed the plan"
    assert (A.info.kernel, A.info.device_bytes, A.get_param("device_bytes")) == (kernel, info_bytes, param_bytes), fmt
    RUNS["state"] += 1


def test_refusals_on_a_live_handle(ctx, orc, pkg):
    capi = pkg.capi
    E = lr.problem("lap16_k4")[0]
    n = E.n
    A = _handle(ctx, orc, E)
    L = _handle(ctx, orc, E, "ell")
    rp, cc, cv = E.csr()
    keep = cc < n - 1
    R = ctx.csr(n, n - 1, np.r_[0, np.cumsum(np.bincount(E.row[keep], minlength=n))].astype(np.int32), cc[keep], cv[keep])
    X = ctx.gen_vector(n * 4, seed=1)
    before = X.download()

    def refused(code, needle, M=A, x=X, k=4, **kw):
        with pytest.raises(capi.SpmvError) as e:
            ctx.lobpcg(M, x, k, **kw)
        assert e.value.code == code and "spmv_lobpcg" in str(e.value) and needle in str(e.value), str(e.value)

    refused(INVALID, "square", M=R)
    refused(INVALID, "k = 0", k=0, nev=0)
    refused(INVALID, "k = 17", k=17, nev=1)
    refused(INVALID, "nev", nev=0)
    refused(INVALID, "nev", nev=5)
    refused(INVALID, "3 k", M=_handle(ctx, orc, lr.problem("dense12_smallest")[0]), x=ctx.gen_vector(12 * 5), k=5)
    refused(INVALID, "entries", x=ctx.gen_vector(n * 4 - 1))
    refused(INVALID, "max_iter", max_iter=-1)
    refused(INVALID, "tol", tol=-1.0)
    refused(INVALID, "unknown preconditioner", precond=9)
    refused(UNSUPPORTED, "Gauss-Seidel", precond=capi.PRECOND_SYMGS)
    refused(UNSUPPORTED, "Jacobi", M=L, precond=capi.PRECOND_JACOBI)
    refused(UNSUPPORTED, "ILU", M=L, precond=capi.PRECOND_ILU0)
    refused(UNSUPPORTED, "AMG", M=L, precond=capi.PRECOND_AMG)
    assert np.array_equal(X.download(), before), "a refused call wrote X"
    RUNS["refusals"] += 1


# ---- the pairs family: k = 16 past 256 workgroups and past one and two trips of the grid -----------------------------------------------
# lobpcg_ref.pairs at n1 = 256 B + 1 (257 workgroups: the last-ticket sum of lobpcg_resid_kernel takes a second step), n2 = 257 B + 1,
# n3 = G B + 1 (a full grid and one row on the second trip) and n4 = 2 G B + 2051 (a third trip, ld = padded(n) != n).  The twin takes up
# to a minute there: its iteration counts and early theta come from tests/golden/lobpcg_pairs_twin.json, which tests/test_lobpcg_ref.py
# holds to the twin.
_PAIRS = {}  # n -> the host start block; (n, largest, kernel) -> the handle


def _pairs_sizes():
    """the four sizes, each held to the grid it is there for"""
    B, G = lr.grid_constants()
    z = lr.pairs_sizes()
    grid = lambda n: max(1, min(G, -(-n // B)))  # noqa: E731  (stream_grid of csrc/common.hpp)
    assert G > 258 and grid(z["n1"]) == 257 and grid(z["n2"]) == 258
    assert grid(z["n3"]) == G and z["n3"] - G * B == 1
    assert grid(z["n4"]) == G and z["n4"] > 2 * G * B and z["n4"] % 2 == 1 and z["n4"] % 32 != 0
    return z


def _pairs_handle(ctx, name, kernel=AUTO):
    E, _, _, _, largest = lr.pairs_problem(name)[:5]
    key = (E.n, largest, kernel)
    if key not in _PAIRS:
        rp, cc, cv = E.csr()
        _PAIRS[key] = ctx.csr(E.n, E.n, rp, cc, cv)
        if kernel != AUTO:
            _PAIRS[key].set_kernel(kernel)
    return _PAIRS[key]


def _pairs_start(ctx, pkg, n):
    """(the start block on the device - generated there and equal to its twin -, the twin's block)"""
    if n not in _PAIRS:
        _PAIRS[n] = lr.pairs_start(n, pkg.synth.vec_uniform)
    X = ctx.gen_vector(n * lr.PAIRS_K, seed=1)
    assert np.array_equal(X.download().reshape(lr.PAIRS_K, n).T, _PAIRS[n]), "the device's start block is not its NumPy twin's"
    return X, _PAIRS[n]


def _pairs_solve(ctx, pkg, name, max_iter=None, kernel=AUTO):
    E, lam, k, nev, largest, tol, limit, pre = lr.pairs_problem(name)
    assert k == 16 and E.n == _pairs_sizes()[lr.PAIRS_CASES[name][0]]
    A = _pairs_handle(ctx, name, kernel)
    X, X0 = _pairs_start(ctx, pkg, E.n)
    code = pkg.capi.PRECOND_JACOBI if pre == "jacobi" else pkg.capi.PRECOND_NONE
    theta, resid, iters = ctx.lobpcg(A, X, k, nev=nev, largest=largest, max_iter=limit if max_iter is None else max_iter, tol=tol, precond=code)
    return theta, resid, iters, X.download().reshape(k, E.n).T, X0


@pytest.mark.parametrize("name", list(lr.PAIRS_CASES))
def test_pairs_converged_solves(ctx, pkg, name):
    """Checks (a)-(d) for the first nev columns, (e) max |X^T A X - diag(theta)| <= 1e-12 ||A||_inf over all 16 in long double, and
    iters <= ceil(1.25 * twin) + 2 against the recorded twin count.

    pairs_n2_nev12_largest is the case that loses rank among its residuals: from this start block at iteration 17 (smallest pivot
    9.8e-07 against kLobpcgRankPivot = 1e-6) and in most iterations after, where the solver leaves the dependent columns out; the twin,
    by the same rule, takes 49 iterations."""
    E, lam, k, nev, largest, tol, _, _ = lr.pairs_problem(name)
    rec = lr.load_records()[name]
    assert rec["n"] == E.n and rec["k"] == k and rec["nev"] == nev
    theta, resid, iters, Xh, _ = _pairs_solve(ctx, pkg, name)
    print(f"{name}: {iters} iterations (twin {rec['iterations']}), resid max {resid[:nev].max():.2e}, theta {theta[:nev]}")
    fails = lr.outcome_failures(E.matvec_ld, E.norm_inf(), Xh, theta, resid, nev, tol, lam, largest)
    assert fails == [], (name, fails, iters, resid, theta, lam[:k])
    assert lr.ritz_failure(E, Xh, theta) is None, lr.ritz_failure(E, Xh, theta)
    COUNTS[f"{name} csr auto"] = (iters, rec["iterations"])
    assert iters <= math.ceil(1.25 * rec["iterations"]) + 2, f"{name}: {iters} iterations, the twin took {rec['iterations']}"
    RUNS["pairs_solves"] += 1


@pytest.mark.parametrize("max_iter", lr.EARLY)
@pytest.mark.parametrize("name", lr.PAIRS_EARLY)
def test_pairs_early_iterates(ctx, pkg, name, max_iter):
    """After max_iter = 0 .. 3 iterations: checks (b), (c) and (e), and theta of all 16 columns within 1e-12 ||A||_inf of the twin's.
    Ritz values of a subspace both sides share: moving every entry of the start block by one ulp moves the twin's theta by at most
    3.7e-14, 2.7e-14, 2.8e-14 and 6.2e-15 at t = 0, 1, 2, 3 over the four sizes (`python tests/lobpcg_ref.py --one-ulp`; ||A||_inf = 21,
    so the gate of 2.1e-11 is some 560 times that, and the measured value is below 1e-13 ||A||_inf).  n1 is here because the last of
    its 257 workgroups holds nothing but the row that stands alone: at convergence that row's residual is zero, on the way it is not."""
    E, lam, k, nev, largest, tol, _, _ = lr.pairs_problem(name)
    rec = lr.load_records()[name]
    assert rec["n"] == E.n and rec["iterations"] > lr.EARLY[-1]
    theta, resid, iters, Xh, X0 = _pairs_solve(ctx, pkg, name, max_iter=max_iter)
    assert iters == max_iter
    moved = float(np.max(np.abs(theta - lr.recorded_theta(rec)[max_iter])))
    print(f"{name} max_iter {max_iter}: max |theta - twin's| = {moved:.2e}, resid {resid.min():.2e} .. {resid.max():.2e}")
    fails = lr.outcome_failures(E.matvec_ld, E.norm_inf(), Xh, theta, resid, k, tol, lam, largest)
    assert "b" not in fails and "c" not in fails, (name, max_iter, fails)
    assert lr.ritz_failure(E, Xh, theta) is None, lr.ritz_failure(E, Xh, theta)
    assert moved <= 1e-12 * E.norm_inf(), (name, max_iter, moved, theta, lr.recorded_theta(rec)[max_iter])
    if max_iter == 0:
        Q, _ = np.linalg.qr(X0)
        assert np.max(np.abs(Xh - Q @ (Q.T @ Xh))) <= 1e-12, "the vectors left the span of the start block"
    RUNS["pairs_early"] += 1


def _free_settled(ctx, expect, seconds=1.0):
    """the free device memory, read again until it is `expect` or `seconds` have passed: hipMemGetInfo can still count a slab for a
    fraction of a millisecond after the hipFree that returned it (seen after a solve at 257 B + 1 rows: 69,206,016 bytes still counted
    0.01 ms after the call, gone at 0.15 ms; the small problems' slabs never showed it)"""
    end = time.perf_counter() + seconds
    while True:
        ctx.sync()
        free = ctx.mem_info()[0]
        if free == expect or time.perf_counter() >= end:
            return free


@pytest.mark.parametrize("name", ("pairs_n2_nev12_jacobi", "pairs_n4_nev12_jacobi"))
def test_pairs_two_identical_solves_agree_bit_for_bit(ctx, pkg, name):
    """under SCALAR and max_iter = 3: equal bits, the free device memory as before, and the result held to (b), (c) and (e)"""
    E, lam, k, nev, largest, tol, _, _ = lr.pairs_problem(name)
    A = _pairs_handle(ctx, name, SCALAR)  # a product that adds in a fixed order: what is tested is the solver's own sums
    X, X0 = _pairs_start(ctx, pkg, E.n)
    out, free = [], []
    for _ in range(2):  # (the second solve allocates nothing but its workspace: the same X, written again)
        X.upload(np.ascontiguousarray(X0.T).ravel())
        gc.collect()
        ctx.sync()
        free.append(ctx.mem_info()[0])
        theta, resid, iters = ctx.lobpcg(A, X, k, nev=nev, max_iter=3, tol=tol, precond=pkg.capi.PRECOND_JACOBI)
        free.append(_free_settled(ctx, free[-1]))
        out.append((X.download().tobytes(), theta.tobytes(), resid.tobytes(), iters))
    assert out[0][3] == 3 and out[0] == out[1], "two calls on the same data differ"
    assert free[3] == free[2], f"{free[2] - free[3]} bytes of device memory not returned by the second solve"
    Xh = np.frombuffer(out[1][0]).reshape(k, E.n).T
    fails = lr.outcome_failures(E.matvec_ld, E.norm_inf(), Xh, theta, resid, k, tol, lam, largest)
    assert "b" not in fails and "c" not in fails, (name, fails)
    assert lr.ritz_failure(E, Xh, theta) is None, lr.ritz_failure(E, Xh, theta)
    RUNS["pairs_bits"] += 1


def test_every_case_ran():
    expect = {"csr": len(CSR_CASES), "formats": len(FORMATS), "preconditioners": len(PRECOND_PROBLEMS), "bits": 1, "limits": 1, "rank": 1, "dependent": 1,
              "state": 1 + len(FORMATS), "refusals": 1, "pairs_solves": len(lr.PAIRS_CASES), "pairs_early": len(lr.PAIRS_EARLY) * len(lr.EARLY),
              "pairs_bits": 2}
    if any(RUNS[f] != c for f, c in expect.items()):
        pytest.skip(f"the coverage check needs every test of this module (ran {dict(RUNS)}, expected {expect})")
    assert len(COUNTS) == len(CSR_CASES) + len(FORMATS) + len(PRECOND_PROBLEMS) + len(lr.PAIRS_CASES)
    out = os.environ.get("SPMV_LOBPCG_COUNTS")
    if out:
        lines = ["# spmv_lobpcg against its NumPy twin (tests/test_gpu_lobpcg.py): iterations to the problem's tolerance on the same problem and start block;",
                 "# the condition is GPU <= ceil(1.25 * twin) + 2.", "# case | GPU | twin"]
        lines += [f"{case:40s} {g:5d} {t:5d}" for case, (g, t) in COUNTS.items()]
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
