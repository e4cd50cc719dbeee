"""spmv_minres - symmetric indefinite solves with a shift over one forward product per iteration - iterate by iterate against the
extended-precision recurrence (`pytest -m gpu`).

spmv_minres(max_iter = k, rel_tol = 0) runs exactly k iterations from the x passed in.  For the k of (1, 2, 3, 4, 5, 8, 9, 13) that
the drop rule of tests/minres_ref.py leaves (an iterate behind a residual at the noise floor is not asked for) and with the host
looking every iteration and every fourth, x_k and the returned phibar_k / beta_b are held to Paige and Saunders' MINRES in
np.longdouble.  The gate at step k is F = 8 times the largest deviation from that reference of any float64 twin of the recurrence
(three dot orders x two orders of a row's products), measured on the reference's own arithmetic and floored at 2^-50; neither gate
is ever measured on the engine.  What the gate catches - the r1 term dropped, a stale w1, dbar's sign, the shift ignored, beta from
r2.r2 under a preconditioner, an element of x left out - is checked on the CPU in tests/test_minres_ref.py.

Problems (all symmetric, none definite): 1 x 1 negative, the 2 x 2 swap, 3 x 3 dense; 33 x 33 and 4097 x 4097 random with a dominant
diagonal of alternating sign; a 4099 x 4099 band of seven diagonals around 0; a saddle point [[K, B^T], [B, 0]] whose preconditioner
is built from the separate handle blockdiag(K, I); the 65 x 63 Laplacian with a shift inside its spectrum, preconditioned by the
Laplacian itself; and the band at a size that is odd and beyond two sweeps of the vector kernels' largest grid (csrc/common.hpp:
2 * kMaxGrid * kBlock).  CSR under AUTO, plain and with Jacobi where the preconditioner's diagonal is positive, and forced VECTOR,
SCALAR and PANEL; COO (entries shuffled), CSC, ELL and DIA handles of the band; x and b 256-byte aligned (the 16-byte kernels) and
8 bytes past a 16-byte boundary (the 8-byte kernels); a random start and x0 = 0.

FSAI and Chebyshev (given bounds) of a separate positive definite handle P are stepped through in the same way (tests/precond_ops.py:
SYM_CASES): the factor is read back from P, and the reference and its six twins apply that factor as a fixed linear operator in their
own arithmetic, so a deviation belongs to the solver - b.M^-1 b and r1.y of the set-up, launch 3 without y, the application, r2.y
with the rotation, the pointers rotating around a y of its own.  1 x 1 .. 3 x 3 with the 1-D Laplacian as P, the shifted Laplacian,
the saddle point, and the large odd size; both alignments, both starts.  ILU(0) is refused by this solver.

AMG has no fixed factor to read back and no twin here, so it - and, kept beside it, Chebyshev on the saddle point's P and FSAI on the
Laplacian run to a tolerance with the default set-ups - is held to CONVERGENCE ONLY: the solve ends within the tolerance it reports,
and the true 2-norm residual computed on the host in np.longdouble is within F sqrt(cond(P)) of it (the M^-1 norm the solver stops on
and the 2-norm differ by at most the root of M's condition number, and M^-1 stands between a multiple of I and P^-1).

Then convergence to 1e-10 against the true residual (with spmv_cg answering SPMV_ERR_INVALID on the same systems), the stopping rules
and special cases, refusals, a preconditioner that is not positive definite, reproducibility bit for bit, the handles' state and the
device memory before and after, and the torch operator.  test_every_case_ran asserts at the end that all of it ran; with
SPMV_MINRES_RATIOS=<file> it also writes the largest GPU deviation over twin envelope per problem
(profiles/minres_steps_gpu_vs_twin_envelope.txt).
"""
import collections
import os
import re
from pathlib import Path

import numpy as np
import pytest

import minres_ref as mr
import oracle_lib as ol
import precond_ops as po
from cgls_ref import rect

pytestmark = pytest.mark.gpu
AUTO, VECTOR, SCALAR, PANEL = 0, 1, 3, 4
NONE, JACOBI, SYMGS, ILU0, CHEBYSHEV, AMG, FSAI = 0, 1, 2, 3, 4, 5, 6
INVALID, UNSUPPORTED = -1, -5
CHECK_EVERY = (1, 4)
PRECOND_NAME = {NONE: None, JACOBI: "jacobi"}
LAUNCHED_ID = {"chebyshev": CHEBYSHEV, "fsai": FSAI}
RUNS = collections.Counter()
RATIO = {}  # problem -> {"x" | "residual": (largest deviation / twin envelope, where)}
_MAT = {}
_ENV = {}
_OP = {}  # (problem, spec) -> (the engine's factor, the operator of tests/precond_ops.py over it)


def _grid_constants():
    """kBlock and kMaxGrid as csrc/common.hpp defines them"""
    text = (Path(__file__).resolve().parent.parent / "arm-spmv_amd" / "csrc" / "common.hpp").read_text()
    vals = {}
    for name, expr in re.findall(r"constexpr int (k\w+)\s*=\s*([^;]+);", text):
        try:
            vals[name] = int(eval(expr, {"__builtins__": {}}, dict(vals)))
        except Exception:
            pass
    return vals["kBlock"], vals["kMaxGrid"]


def _big_n():
    block, max_grid = _grid_constants()
    return 2 * max_grid * block + 2051  # odd, and beyond two sweeps of the one- and of the two-element grids


def _problem(name):
    if name not in _MAT:
        _MAT[name] = mr.problem(name, _big_n() if name == "big" else None)
    return _MAT[name]


def _envelope(name, precond, zero_start=False):
    """the reference iterates and twin envelopes of one problem (computed once and shared)"""
    key = (name, precond, zero_start)
    if key not in _ENV:
        p = _problem(name)
        why = mr.available(p.n)
        if why:
            pytest.skip(why)
        _ENV[key] = mr.Envelope(p.entries, p.n, p.b, np.zeros_like(p.x0) if zero_start else p.x0, p.ks, p.shift, PRECOND_NAME[precond], p.p_entries)
    return _ENV[key]


def _device_vector(ctx, host, aligned):
    """host on the device, 256-byte aligned (spmv_vec_create) or 8 bytes past a 16-byte boundary (a wrapped pointer into a vector
    of n + 1: an ordinary, legal double*)"""
    n = len(host)
    if aligned:
        v = ctx.vector_from(host)
        assert v.device_ptr % 16 == 0
        return v, None
    base = ctx.vector(n + 1)
    base.fill(0.0)
    ptr = base.device_ptr + 8
    assert ptr % 16 == 8
    v = ctx.wrap_vector(ptr, n)
    v.upload(host)
    return v, base


def _note(name, kind, ratio, where):
    old = RATIO.setdefault(name, {})
    if kind not in old or ratio > old[kind][0]:  # (a ratio of 0 - an exact iterate - is a record too)
        old[kind] = (ratio, where)


def _sorted_csr(n, entries):
    row, col, val = entries
    o = np.argsort(row, kind="stable")
    return mr.csr_arrays(n, row[o], col[o], val[o])


def _csr(ctx, name):
    p = _problem(name)
    return ctx.csr(p.n, p.n, *_sorted_csr(p.n, p.entries))


def _precond_handle(ctx, name, A):
    """the handle the preconditioner is built from: a separate one where the problem names its matrix (shifted: the Laplacian is the
    system's own matrix, and is still passed as P), else None"""
    p = _problem(name)
    if p.p_entries is None:
        return None
    return A if p.p_entries is p.entries else ctx.csr(p.n, p.n, *_sorted_csr(p.n, p.p_entries))


# ---- the preconditioners applied by launches: the engine's own factor, and the references over it ---------------------------------
def _engine_factor(ctx, M, spec):
    """sets the handle M up as `spec` says and reads back what defines M^-1: G, the ILU(0) values in row order, or the Chebyshev state"""
    if spec.kind == "fsai":
        ctx.fsai_setup(M, spec.level)
        return ctx.fsai_factor(M)
    if spec.kind == "ilu0":
        M.set_param("ilu0_order", 0)
        ctx.ilu0_setup(M)
        assert np.array_equal(ctx.ilu0_order(M), np.arange(M.info.nrow))
        return ctx.ilu0_factors(M)
    ctx.chebyshev_setup(M, degree=spec.degree, scaled=spec.scaled, lmin=spec.lmin, lmax=spec.lmax)
    return ctx.chebyshev_info(M)


def _same_factor(a, c):
    return all(np.array_equal(u, v) for u, v in zip(a, c)) if isinstance(a, tuple) else np.array_equal(a, c)


def _launched_problem(name):
    if ("launched", name) not in _MAT:
        _MAT["launched", name] = po.sym_problem(name, _big_n() if name == "big" else None)
    return _MAT["launched", name]


def _launched_handles(ctx, name, spec):
    """(A, P): the system and, ALWAYS a handle of its own, the positive definite matrix the preconditioner is built from, set up as
    `spec` says; the operator over the engine's factor is built once per (problem, spec), and every later P must hold the same
    factor bit for bit"""
    p = _launched_problem(name)
    A = ctx.csr(p.n, p.n, *_sorted_csr(p.n, p.entries))
    P = ctx.csr(p.n, p.n, *_sorted_csr(p.n, p.p_entries))
    factor = _engine_factor(ctx, P, spec)
    if (name, spec) not in _OP:
        _OP[name, spec] = (factor, po.build(spec, p.n, p.p_entries, factor))
    assert _same_factor(factor, _OP[name, spec][0]), f"{po.label(name, spec)}: two set-ups of the same matrix differ"
    return A, P


def _launched_envelope(name, spec, zero_start):
    key = ("launched", name, spec, zero_start)
    if key not in _ENV:
        p = _launched_problem(name)
        why = mr.available(p.n)
        if why:
            pytest.skip(why)
        _ENV[key] = mr.Envelope(p.entries, p.n, p.b, np.zeros_like(p.x0) if zero_start else p.x0, p.ks, p.shift, _OP[name, spec][1])
    return _ENV[key]


def _steps(ctx, A, P, name, precond, aligned, what, zero_start=False, spec=None):
    """every k the problem keeps with check_every 1 and 4: iters, x_k and the residual against the reference.  spec: the problem is
    precond_ops', the preconditioner the launched one that P was set up with (_launched_handles), the reference runs over its factor"""
    if spec is None:
        p = _problem(name)
        env = _envelope(name, precond, zero_start)
    else:
        p = _launched_problem(name)
        env = _launched_envelope(name, spec, zero_start)
        precond, name = LAUNCHED_ID[spec.kind], po.label(name, spec)
    start = np.zeros_like(p.x0) if zero_start else p.x0
    db, keep_b = _device_vector(ctx, p.b, aligned)
    misses = []
    for k in env.ks:
        for check_every in CHECK_EVERY:
            x, keep_x = _device_vector(ctx, start, aligned)
            iters, res = ctx.minres(A, db, x, shift=p.shift, P=P if precond != NONE else None, max_iter=k, rel_tol=0.0, check_every=check_every,
                                    precond=precond)
            got = x.download()
            del x, keep_x
            tag = f"{name} {what} precond={precond} {'aligned' if aligned else 'offset'}{' x0=0' if zero_start else ''} k={k} check_every={check_every}"
            assert iters == k, (tag, iters)
            dev, rdev = env.x_dev(k, got), env.resid_dev(k, res)
            print(f"{tag}: x deviation {dev:.2e} (twins {env.envelope(k):.2e}, gate {env.gate(k):.2e}); residual {res:.6e} deviation {rdev:.2e} "
                  f"(gate {env.gate_resid(k):.2e})")
            _note(name, "x", dev / env.envelope(k), tag)
            _note(name, "residual", rdev / env.envelope(k, 1), tag)
            if not dev <= env.gate(k):
                misses.append(f"{tag}: max|x_k - ref_k| / max|ref_k| = {dev:.3e} > gate {env.gate(k):.3e}")
            if not rdev <= env.gate_resid(k):
                misses.append(f"{tag}: rel_resid {res!r} against {env.ref_resid[k]!r}: {rdev:.3e} > gate {env.gate_resid(k):.3e}")
    del db, keep_b
    return misses


# ---- 1. every problem as a CSR handle under AUTO: both alignments, plain and Jacobi where P's diagonal is positive ----------------
JACOBI_OK = ("band4099", "saddle", "shifted")
CSR_CASES = [(name, NONE) for name in mr.PROBLEMS[:-1]] + [(name, JACOBI) for name in JACOBI_OK] + [("big", JACOBI)]


@pytest.mark.parametrize("name,precond", CSR_CASES, ids=lambda v: str(v))
def test_minres_iterates_match_the_extended_precision_recurrence(ctx, pkg, name, precond):
    A = _csr(ctx, name)
    P = _precond_handle(ctx, name, A)
    misses = []
    for aligned in (True, False) if name != "big" else (False,):
        misses += _steps(ctx, A, P, name, precond, aligned, "csr auto")
    assert not misses, "\n".join(misses)
    RUNS["csr"] += 1


@pytest.mark.parametrize("name", ("r33", "saddle"))
def test_minres_iterates_from_a_zero_start(ctx, pkg, name):
    A = _csr(ctx, name)
    P = _precond_handle(ctx, name, A)
    misses = _steps(ctx, A, P, name, NONE, True, "csr auto", zero_start=True)
    if name in JACOBI_OK:
        misses += _steps(ctx, A, P, name, JACOBI, False, "csr auto", zero_start=True)
    assert not misses, "\n".join(misses)
    RUNS["zero start"] += 1


# ---- 1b. FSAI and Chebyshev of a separate handle P: y is a buffer of its own, written by apply_preconditioner ----------------------
LAUNCHED_CASES = po.SYM_CASES
LAUNCHED_NAMES = tuple(po.label(name, spec) for name, spec in LAUNCHED_CASES)


@pytest.mark.parametrize("name,spec", LAUNCHED_CASES, ids=lambda v: v if isinstance(v, str) else v.kind)
def test_minres_iterates_under_the_preconditioners_applied_by_launches(ctx, pkg, name, spec):
    """the reference and its twins apply the factor read back from P, so a deviation is the solver's: the set-up's b.M^-1 b and r1.y,
    launch 3 without y, the application, r2.y with the rotation, the pointers rotating around y; 16-byte and 8-byte x and b, both starts"""
    A, P = _launched_handles(ctx, name, spec)
    misses = []
    for aligned, zero_start in ((True, False), (False, False), (True, True), (False, True)) if name != "big" else ((False, False),):
        misses += _steps(ctx, A, P, name, None, aligned, "csr auto", zero_start, spec)
    assert not misses, "\n".join(misses)
    RUNS["launched steps"] += 1


# ---- 2. forced product kernels ---------------------------------------------------------------------------------------------------------
KERNEL_CASES = [("r4097", "vector", VECTOR), ("r4097", "scalar", SCALAR), ("r4097", "panel", PANEL)]


@pytest.mark.parametrize("name,label,kid", KERNEL_CASES, ids=lambda v: str(v))
def test_minres_iterates_under_forced_csr_kernels(ctx, pkg, name, label, kid):
    A = _csr(ctx, name)
    A.set_kernel(kid)
    assert A.info.kernel == kid
    misses = []
    for aligned in (False, True):
        misses += _steps(ctx, A, None, name, NONE, aligned, f"csr {label}")
    assert not misses, "\n".join(misses)
    assert A.info.kernel == kid
    RUNS["kernels"] += 1


# ---- 3. the other formats, on the band -------------------------------------------------------------------------------------------------
def _band_handle(ctx, orc, fmt):
    p = _problem("band4099")
    n, (row, col, val) = p.n, p.entries
    rp, cc, cv = _sorted_csr(n, p.entries)
    if fmt == "csr":
        return ctx.csr(n, n, rp, cc, cv)
    if fmt == "coo":
        o = np.random.default_rng(5).permutation(len(row))
        return ctx.coo(n, n, ol.i32(row[o]), ol.i32(col[o]), ol.f64(val[o]))
    if fmt == "csc":
        cp, cri, ccv = ol.coo_to_csc(orc, n, ol.i32(row), ol.i32(col), ol.f64(val))
        return ctx.csc(n, n, cp, cri, ccv)
    if fmt == "ell":
        k, ec, ev = ol.coo_to_ell(orc, n, ol.i32(row), ol.i32(col), ol.f64(val))
        return ctx.ell(n, n, k, len(val), ec, ev)
    offsets, dval = ol.csr_to_dia(orc, n, n, rp, cc, cv)
    assert len(offsets) == len(mr.SYM_OFFSETS)
    return ctx.dia(n, n, offsets, dval)


FORMATS = ("coo", "csc", "ell", "dia")


@pytest.mark.parametrize("fmt", FORMATS)
def test_minres_iterates_on_every_format(ctx, orc, pkg, fmt):
    A = _band_handle(ctx, orc, fmt)
    misses = []
    for aligned in (True, False):
        misses += _steps(ctx, A, None, "band4099", NONE, aligned, fmt)
    assert not misses, "\n".join(misses)
    RUNS["formats"] += 1


# ---- 4. convergence ----------------------------------------------------------------------------------------------------------------------
def _shifted_explicitly(ctx, name):
    """A - shift I as a handle of its own, built on the host: what a solver without a shift has to be given"""
    p = _problem(name)
    row, col, val = p.entries
    val = np.where(row == col, val - p.shift, val)
    return ctx.csr(p.n, p.n, *_sorted_csr(p.n, (row, col, val)))


@pytest.mark.parametrize("name", ("saddle", "shifted", "n2"))
def test_minres_converges_to_the_tolerance_it_reports(ctx, pkg, name):
    """to 1e-10 without a preconditioner, against the true residual in np.longdouble with tests/test_gpu_bicgstab.py's margin (F times
    the float64 twin's own true residual, or the tolerance).  The swap ends within two iterations.  On the swap and on the shifted
    Laplacian spmv_cg, given the same system (for the latter as a handle of A - shift I built on the host: it takes no shift), answers
    SPMV_ERR_INVALID: the gap this solver closes"""
    capi = pkg.capi
    rel_tol, max_iter = 1e-10, 5000
    p = _problem(name)
    why = mr.available(p.n)
    if why:
        pytest.skip(why)
    A = _csr(ctx, name)
    db, x = ctx.vector_from(p.b), ctx.vector_from(p.x0)
    iters, res = ctx.minres(A, db, x, shift=p.shift, max_iter=max_iter, rel_tol=rel_tol)
    true = mr.true_residual(p.entries, p.n, p.b, x.download(), p.shift)
    twin_x, twin_iters = mr.run_to_tolerance(p.entries, p.n, p.b, p.x0, p.shift, rel_tol, max_iter)
    twin_true = mr.true_residual(p.entries, p.n, p.b, twin_x, p.shift)
    print(f"{name}: {iters} iterations (twin {twin_iters}), reported residual {res:.3e}, true {true:.3e} (twin's {twin_true:.3e})")
    assert 0 < iters < max_iter and res <= rel_tol, (iters, res)
    assert true <= mr.F * max(rel_tol, twin_true), (true, twin_true)
    if name == "n2":
        assert iters <= 2, iters
    if name in ("n2", "shifted"):
        S = _shifted_explicitly(ctx, name)
        with pytest.raises(capi.SpmvError) as e:
            ctx.cg(S, db, ctx.vector_from(p.x0), max_iter=max_iter, rel_tol=rel_tol)
        assert e.value.code == INVALID and "spmv_cg" in str(e.value), e.value
    RUNS["convergence"] += 1


def _cond_sqrt(name):
    """sqrt(cond_2(P)) of the preconditioner's matrix, from its eigenvalues in closed form"""
    if name == "shifted":
        lam = mr.laplacian_eigenvalues(mr.SHIFTED_GRID)
        return float(np.sqrt(lam[-1] / lam[0]))
    assert name == "saddle"  # blockdiag(K, I): K's eigenvalues 4 sin^2(j pi / (2 (n + 1))), and 1
    lam = 4 * np.sin(np.arange(1, mr.SADDLE_K + 1) * np.pi / (2 * (mr.SADDLE_K + 1))) ** 2
    return float(np.sqrt(max(lam[-1], 1.0) / min(lam[0], 1.0)))


BY_LAUNCHES_CASES = [("saddle", CHEBYSHEV), ("shifted", FSAI), ("shifted", AMG)]


@pytest.mark.parametrize("name,precond", BY_LAUNCHES_CASES, ids=lambda v: str(v))
def test_minres_converges_under_the_preconditioners_applied_by_launches(ctx, pkg, name, precond):
    """convergence only (AMG has no twin; the other two are stepped through above and run to a tolerance here): the separate handle
    P, set up on first use with the defaults; the solve ends within the tolerance it reports, in fewer iterations than max_iter, from both alignments with the same count, and the true
    2-norm residual is within F sqrt(cond(P)) of the tolerance"""
    rel_tol, max_iter = 1e-10, 20000
    p = _problem(name)
    why = mr.available(p.n)
    if why:
        pytest.skip(why)
    A = _csr(ctx, name)
    P = ctx.csr(p.n, p.n, *_sorted_csr(p.n, p.p_entries))  # (a handle of its own even where it holds A's matrix)
    bound = mr.F * _cond_sqrt(name) * rel_tol
    counts = []
    for aligned in (True, False):
        db, kb = _device_vector(ctx, p.b, aligned)
        x, kx = _device_vector(ctx, p.x0, aligned)
        iters, res = ctx.minres(A, db, x, shift=p.shift, P=P, max_iter=max_iter, rel_tol=rel_tol, check_every=5, precond=precond)
        true = mr.true_residual(p.entries, p.n, p.b, x.download(), p.shift)
        print(f"{name} precond {precond} {'aligned' if aligned else 'offset'}: {iters} iterations, reported {res:.3e} (M^-1 norm), true 2-norm residual "
              f"{true:.3e} (bound {bound:.3e})")
        assert 0 < iters < max_iter and res <= rel_tol, (iters, res)
        assert true <= bound, (true, bound)
        counts.append(iters)
        del db, kb, x, kx
    assert counts[0] == counts[1], counts
    RUNS["by launches"] += 1


# ---- 5. stopping rules and special cases -------------------------------------------------------------------------------------------------
def test_stopping_rules_and_special_cases(ctx, pkg):
    capi = pkg.capi
    name = "band4099"
    p = _problem(name)
    n, b, x0 = p.n, p.b, p.x0
    A = _csr(ctx, name)
    for aligned in (True, False):
        # b = 0: nothing to do, x stays
        db, kb = _device_vector(ctx, np.zeros(n), aligned)
        x, kx = _device_vector(ctx, x0, aligned)
        assert ctx.minres(A, db, x, max_iter=50, precond=JACOBI) == (0, 0.0)
        assert x.download().tobytes() == x0.tobytes(), "b = 0: x was written"
        # max_iter = 0: x stays, the residual is that of x0
        db, kb = _device_vector(ctx, b, aligned)
        for precond in (NONE, JACOBI):
            env0 = mr.Envelope(p.entries, n, b, x0, (0,), 0.0, PRECOND_NAME[precond])
            iters, res = ctx.minres(A, db, x, max_iter=0, rel_tol=0.0, precond=precond)
            assert iters == 0 and x.download().tobytes() == x0.tobytes()
            assert env0.resid_dev(0, res) <= env0.gate_resid(0), (res, env0.ref_resid)
        # a start that is already within the tolerance: no iteration either
        iters, res = ctx.minres(A, db, x, max_iter=50, rel_tol=1e3)
        assert iters == 0 and x.download().tobytes() == x0.tobytes() and 0.0 < res <= 1e3
        del db, kb, x, kx
    swap = _csr(ctx, "n2")
    for check_every in (1, 4):
        # beta = 0 exactly: the swap from x0 = 0 with b = (2, 0) has v_1 = e_1, v_2 = e_2 and a Krylov space of dimension 2 (and
        # beta / oldb = 1/2, exact under fma as well); the second iteration lands on x = (0, 2) with phibar = 0, and the solve ends there
        x = ctx.vector_from(np.zeros(2))
        assert ctx.minres(swap, ctx.vector_from(np.array([2.0, 0.0])), x, max_iter=50, rel_tol=0.0, check_every=check_every) == (2, 0.0)
        assert x.download().tobytes() == np.array([0.0, 2.0]).tobytes()
        # the floor: diag(2, 2, -1, -1) has two eigenvalues, so the second iteration leaves of phibar what rounding leaves; that is
        # below 1e-14 ||b||, every later iteration passes quietly, and the count stays at 2
        D = ctx.csr(4, 4, np.arange(5, dtype=np.int32), np.arange(4, dtype=np.int32), np.array([2.0, 2.0, -1.0, -1.0]))
        bd = np.array([0.5, -1.25, 2.0, 0.75])
        x = ctx.vector_from(np.zeros(4))
        iters, res = ctx.minres(D, ctx.vector_from(bd), x, max_iter=50, rel_tol=0.0, check_every=check_every)
        assert iters == 2 and res <= 1e-14, (iters, res)
        assert np.max(np.abs(x.download() - bd / np.array([2.0, 2.0, -1.0, -1.0]))) <= 2e-15
    # a NaN in b: read by the host in b.b, an error and no fault
    bn = b.copy()
    bn[7] = np.nan
    with pytest.raises(capi.SpmvError) as e:
        ctx.minres(A, ctx.vector_from(bn), ctx.vector_from(x0), max_iter=5)
    assert e.value.code == INVALID and "spmv_minres" in str(e.value) and "b.b" in str(e.value), e.value
    # a NaN in x0 alone: beta1
    xn = x0.copy()
    xn[7] = np.nan
    with pytest.raises(capi.SpmvError) as e:
        ctx.minres(A, ctx.vector_from(b), ctx.vector_from(xn), max_iter=5)
    assert e.value.code == INVALID and "beta1" in str(e.value), e.value
    # an empty matrix: nothing is launched
    E = ctx.csr(0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    assert ctx.minres(E, ctx.vector(0), ctx.vector(0), max_iter=5) == (0, 0.0)
    RUNS["stopping"] += 1


def test_refusals_are_made_on_the_host(ctx, orc, pkg):
    capi = pkg.capi
    p = _problem("band4099")
    n, b, x0 = p.n, p.b, p.x0
    A = _csr(ctx, "band4099")
    db, dx = ctx.vector_from(b), ctx.vector_from(x0)

    def expect(fn, word="spmv_minres", code=INVALID):
        with pytest.raises(capi.SpmvError) as e:
            fn()
        assert e.value.code == code and "spmv_minres" in str(e.value) and word in str(e.value), e.value

    expect(lambda: ctx.minres(A, ctx.vector(n + 1), dx), "entries")
    expect(lambda: ctx.minres(A, db, ctx.vector(n - 1)), "entries")
    big = ctx.vector(3 * n)
    expect(lambda: ctx.minres(A, ctx.wrap_vector(big.device_ptr, n), ctx.wrap_vector(big.device_ptr + 8 * 5, n)), "overlap")
    expect(lambda: ctx.minres(A, db, dx, max_iter=-1), "max_iter")
    expect(lambda: ctx.minres(A, db, dx, rel_tol=-1e-8), "rel_tol")
    expect(lambda: ctx.minres(A, db, dx, shift=float("nan")), "shift")
    expect(lambda: ctx.minres(A, db, dx, shift=float("inf")), "shift")
    expect(lambda: ctx.minres(A, db, dx, precond=7), "unknown preconditioner")
    expect(lambda: ctx.minres(A, db, dx, precond=SYMGS), "Gauss-Seidel", UNSUPPORTED)
    expect(lambda: ctx.minres(A, db, dx, precond=ILU0), "ILU(0)", UNSUPPORTED)
    rp, cc, cv = mr.csr_arrays(33, *rect(33, 17, 6, 7))
    R = ctx.csr(33, 17, rp, cc, cv)
    expect(lambda: ctx.minres(R, ctx.vector(33), ctx.vector(17)), "square")
    # the preconditioner's handle: another size, a rectangle with A's rows, another context, and P with no preconditioner named
    small = _csr(ctx, "r33")
    expect(lambda: ctx.minres(A, db, dx, P=small, precond=JACOBI), "P is 33 x 33")
    R2 = ctx.csr(n, 17, np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    expect(lambda: ctx.minres(A, db, dx, P=R2, precond=JACOBI), "square")
    other = capi.Context(0)
    try:
        rp, cc, cv = _sorted_csr(n, p.entries)
        foreign = other.csr(n, n, rp, cc, cv)
        expect(lambda: ctx.minres(A, db, dx, P=foreign, precond=JACOBI), "another context")
        del foreign
    finally:
        other.close()
    expect(lambda: ctx.minres(A, db, dx, P=A), "SPMV_PRECOND_NONE")
    # Jacobi reads the diagonal of a CSR handle: the preconditioner's, where one is given
    L = _band_handle(ctx, orc, "ell")
    expect(lambda: ctx.minres(L, db, dx, precond=JACOBI), "Jacobi", UNSUPPORTED)
    expect(lambda: ctx.minres(A, db, dx, P=L, precond=JACOBI), "Jacobi", UNSUPPORTED)
    iters, res = ctx.minres(L, db, ctx.vector_from(x0), P=A, max_iter=3, rel_tol=0.0, precond=JACOBI)  # (an ELL system with a CSR P is fine)
    assert iters == 3 and np.isfinite(res)
    assert dx.download().tobytes() == x0.tobytes()
    RUNS["refusals"] += 1


def test_a_preconditioner_that_is_not_positive_definite_is_named(ctx, pkg):
    capi = pkg.capi
    # Jacobi on a diagonal of alternating sign: refused at the set-up, x untouched
    p = _problem("r33")
    A = _csr(ctx, "r33")
    x = ctx.vector_from(p.x0)
    with pytest.raises(capi.SpmvError) as e:
        ctx.minres(A, ctx.vector_from(p.b), x, precond=JACOBI)
    assert e.value.code == INVALID and "spmv_minres" in str(e.value) and "the Jacobi preconditioner is not positive definite" in str(e.value), e.value
    assert x.download().tobytes() == p.x0.tobytes()
    # a zero diagonal entry is refused as in the siblings (the saddle point's own diagonal)
    S = _csr(ctx, "saddle")
    ps = _problem("saddle")
    with pytest.raises(capi.SpmvError) as e:
        ctx.minres(S, ctx.vector_from(ps.b), ctx.vector_from(ps.x0), precond=JACOBI)
    assert e.value.code == INVALID and "zero or missing diagonal" in str(e.value), e.value
    # Chebyshev of an indefinite P.  After three products the residual polynomial is T_4, even: M^-1 = p_3(P) is positive below the
    # interval of the bounds - at the eigenvalue -1 as well - and negative above it (tests/chebyshev_ref.py: closed_form), so the
    # indefinite P = diag(3/2, ..., 3/2, -1, 8) with the bounds [1, 2] makes an M^-1 with the eigenvalue -49 at the entry 8;
    # b = (1, ..., 1) meets it in the set-up's b.M^-1 b, b = e_1 + e_n / 16 only in the r.M^-1 r of the first iteration
    import chebyshev_ref as cr

    assert cr.closed_form(8.0, 3, 1.0, 2.0) < -40 and cr.closed_form(-1.0, 3, 1.0, 2.0) > 0 and cr.closed_form(1.5, 3, 1.0, 2.0) > 0
    n = 33
    d = np.full(n, 1.5)
    d[-2], d[-1] = -1.0, 8.0
    P = ctx.csr(n, n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), d)
    ctx.chebyshev_setup(P, degree=3, scaled=False, lmin=1.0, lmax=2.0)
    b2 = np.zeros(n)
    b2[0], b2[-1] = 1.0, 2.0**-4
    for bvec, it in ((np.ones(n), 0), (b2, 1)):
        x = ctx.vector_from(np.zeros(n))
        with pytest.raises(capi.SpmvError) as e:
            ctx.minres(A, ctx.vector_from(bvec), x, P=P, precond=CHEBYSHEV, max_iter=20)
        msg = str(e.value)
        assert e.value.code == INVALID and "spmv_minres" in msg and "preconditioner is not positive definite" in msg and "M^-1" in msg, msg
        assert f"at or before iteration {it}" in msg, msg
        assert not x.download().any(), "x was written behind a preconditioner that is not positive definite"
    RUNS["not definite"] += 1


# ---- 6. reproducibility, the handles' state, device memory -----------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ("dia", "csr vector"))
def test_two_solves_give_the_same_bits(ctx, orc, pkg, fmt):
    """the DIA kernel and the row-parallel CSR kernel add in fixed orders, so what this tests is the dot reduction"""
    p = _problem("band4099")
    A = _band_handle(ctx, orc, fmt.split()[0])
    if fmt == "csr vector":
        A.set_kernel(VECTOR)
    db = ctx.vector_from(p.b)
    for precond in (NONE,) if fmt == "dia" else (NONE, JACOBI):
        out = []
        for _ in range(2):
            x = ctx.vector_from(p.x0)
            stats = ctx.minres(A, db, x, shift=0.125, max_iter=13, rel_tol=0.0, check_every=4, precond=precond)
            out.append((x.download().tobytes(), stats))
        assert out[0][1][0] == 13 and out[0] == out[1], "two calls on the same data differ"
    RUNS["bits"] += 1


def _state(M):
    return M.get_plan(), M.info.kernel, M.info.device_bytes, M.get_param("device_bytes"), M.get_param("transpose_ready")


@pytest.mark.parametrize("fmt", ("csr",) + FORMATS)
def test_a_solve_leaves_the_handles_alone(ctx, orc, pkg, fmt):
    p = _problem("band4099")
    A = _band_handle(ctx, orc, fmt)
    P = _band_handle(ctx, orc, "csr")
    before_a, before_p = _state(A), _state(P)
    assert before_a[4] == 0
    iters, res = ctx.minres(A, ctx.vector_from(p.b), ctx.vector_from(p.x0), shift=0.125, P=P, max_iter=40, rel_tol=0.0, check_every=7, precond=JACOBI)
    assert iters == 40 and 0 < res < 1
    assert _state(A) == before_a, f"{fmt}: the solve changed A's plan, kernel, device bytes or transposed state"
    assert _state(P) == before_p, f"{fmt}: the solve changed P's plan, kernel, device bytes or transposed state"
    RUNS["state"] += 1


def test_work_vectors_go_back_on_every_path(ctx, pkg):
    """67 MB of work vectors per Jacobi solve on the large problem: ten solves that end well and ten that end in an error would
    leave far more than the suite's leak tolerance (tests/test_gpu_parity.py: 256 MiB) behind if a path kept them"""
    import gc

    capi = pkg.capi
    p = _problem("big")
    n = p.n
    A = _csr(ctx, "big")
    db, x = ctx.vector_from(p.b), ctx.vector_from(p.x0)
    bn = p.b.copy()
    bn[n // 2] = np.nan
    dbn = ctx.vector_from(bn)
    gc.collect()
    ctx.sync()
    free0, _ = ctx.mem_info()
    for _ in range(10):
        assert ctx.minres(A, db, x, max_iter=2, rel_tol=0.0, precond=JACOBI)[0] == 2
        with pytest.raises(capi.SpmvError):
            ctx.minres(A, dbn, x, max_iter=2, precond=JACOBI)
    ctx.sync()
    free1, _ = ctx.mem_info()
    assert 6 * 8 * n * 10 > 256 << 20
    assert abs(free0 - free1) < 256 << 20, f"{(free0 - free1) >> 20} MiB of device memory not returned"
    RUNS["memory"] += 1


# ---- 7. torch ------------------------------------------------------------------------------------------------------------------------------
def test_torch_solve_symmetric_is_the_engine_solve_bit_for_bit():
    """tests/child_minres_torch.py in a fresh process: torch initialises its HIP runtime before the engine's library is loaded"""
    import subprocess
    import sys

    child = Path(__file__).with_name("child_minres_torch.py")
    r = subprocess.run([sys.executable, str(child)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "MINRES_TORCH_OK" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    RUNS["torch"] += 1


# ---- 8. coverage ---------------------------------------------------------------------------------------------------------------------------
def test_every_case_ran():
    """every problem, kernel and format of the cases above ran, and no ratio lies above the gate"""
    expect = {"csr": len(CSR_CASES), "zero start": 2, "kernels": len(KERNEL_CASES), "formats": len(FORMATS), "convergence": 3,
              "by launches": len(BY_LAUNCHES_CASES), "launched steps": len(LAUNCHED_CASES), "stopping": 1, "refusals": 1, "not definite": 1, "bits": 2, "state": 1 + len(FORMATS), "memory": 1,
              "torch": 1}
    if any(RUNS[f] != c for f, c in expect.items()):
        pytest.skip(f"the coverage check needs every test of this module (ran {dict(RUNS)}, expected {expect})")
    names = mr.PROBLEMS + LAUNCHED_NAMES
    assert set(RATIO) == set(names), sorted(set(names) ^ set(RATIO))
    lines = ["# spmv_minres iterate by iterate (tests/test_gpu_minres.py): the largest deviation of the GPU's x_k and of its phibar_k / beta_b",
             "# from the np.longdouble recurrence, in units of the float64 twins' own largest deviation at that k (the gate is 8).",
             "# problem | x ratio | residual ratio | where the x ratio was largest"]
    for name in names:
        r = RATIO[name]
        lines.append(f"{name:18s}  x {r['x'][0]:6.3f}  residual {r['residual'][0]:6.3f}  ({r['x'][1]})")
    print("\n".join(lines))
    out = os.environ.get("SPMV_MINRES_RATIOS")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    for name in names:
        assert all(RATIO[name][kind][0] <= mr.F for kind in RATIO[name]), (name, RATIO[name])
