"""spmv_bicgstab - nonsymmetric square solves over two forward products - iterate by iterate against the extended-precision
recurrence (`pytest -m gpu`).

spmv_bicgstab(max_iter = k, rel_tol = 0) runs exactly k iterations from the x passed in.  For the k of (1, 2, 3, 4, 5, 8, 9, 13) that
the drop rule of tests/bicgstab_ref.py leaves (an iterate behind a residual at the noise floor is not asked for) and with the host
looking every iteration and every fourth, x_k and the returned ||r_k|| / ||b|| are held to right-preconditioned BiCGSTAB in
np.longdouble.  The gate at step k is F = 8 times the largest deviation from that reference of any float64 twin of the recurrence
(three dot orders x two orders of a row's products), measured on the reference's own arithmetic and floored at 2^-50.  What the
gate catches - beta without alpha / omega, omega over s.s, a stale p, an element of x left out, the preconditioner on the other
side - is checked on the CPU in tests/test_bicgstab_ref.py.

Problems: 1 x 1, 2 x 2, 3 x 3 dense; 33 x 33 and 4097 x 4097 random with a dominant diagonal; a 4099 x 4099 band of seven diagonals;
and one whose size is odd and beyond two sweeps of the vector kernels' largest grid (csrc/common.hpp: 2 * kMaxGrid * kBlock).  CSR
under AUTO, plain and with Jacobi, and forced VECTOR, SCALAR and PANEL; COO (entries shuffled), CSC, ELL and DIA handles of the
band; x and b 256-byte aligned (the 16-byte kernels) and 8 bytes past a 16-byte boundary (the 8-byte kernels); a random start and
x0 = 0.

The preconditioners applied by launches - FSAI, ILU(0) in row order, Chebyshev with given bounds - are stepped through in the same
way (tests/precond_ops.py: BICGSTAB_CASES): the factor is read back from the handle, and the reference and its six twins apply that
factor as a fixed linear operator in their own arithmetic, so a deviation belongs to the solver - phat and shat as buffers of their own,
the two applications per iteration, the half, update and direction kernels reading them.  1 x 1 .. 3 x 3, the 33 x 33 Laplacian
(n = 1089), upwind convection-diffusion on 45 x 45 (n = 2025) and the large odd size; both alignments, both starts.  AMG alone stays
at convergence only (tests/test_gpu_amg.py): its cycle has no fixed factor to read back.

Then convergence to 1e-10 against the true residual, the stopping rules and special cases, refusals, reproducibility bit
for bit, the handle's state and the device memory before and after, and the torch operator.  test_every_case_ran asserts at the
end that all of it ran; with SPMV_BICGSTAB_RATIOS=<file> it also writes the largest GPU deviation over twin envelope per problem
(profiles/bicgstab_steps_gpu_vs_twin_envelope.txt).
"""
import collections
import os
import re
from pathlib import Path

import numpy as np
import pytest

import bicgstab_ref as br
import oracle_lib as ol
import precond_ops as po

pytestmark = pytest.mark.gpu
AUTO, VECTOR, SCALAR, PANEL = 0, 1, 3, 4
NONE, JACOBI, SYMGS, ILU0, CHEBYSHEV, AMG, FSAI = 0, 1, 2, 3, 4, 5, 6
LAUNCHED_ID = {"ilu0": ILU0, "chebyshev": CHEBYSHEV, "fsai": FSAI}
INVALID, UNSUPPORTED = -1, -5
CHECK_EVERY = (1, 4)
PRECOND_NAME = {NONE: None, JACOBI: "jacobi"}
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
        n, ent, b, x0, ks = br.problem(name, _big_n() if name == "big" else None)
        _MAT[name] = (n, ent, b, x0, ks, br.csr_arrays(n, *ent))
    return _MAT[name]


def _envelope(name, precond, zero_start=False):
    """the reference iterates and twin envelopes of one problem (computed once and shared)"""
    key = (name, precond, zero_start)
    if key not in _ENV:
        n, ent, b, x0, ks, _ = _problem(name)
        why = br.available(n)
        if why:
            pytest.skip(why)
        _ENV[key] = br.Envelope(ent, n, b, np.zeros_like(x0) if zero_start else x0, ks, PRECOND_NAME[precond])
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
        n, ent, b, x0, ks = po.nonsym_problem(name, _big_n() if name == "big" else None)
        _MAT["launched", name] = (n, ent, b, x0, ks, br.csr_arrays(n, *ent))
    return _MAT["launched", name]


def _launched_handle(ctx, name, spec):
    """a CSR handle of the problem set up as `spec` says; the operator over the engine's factor is built once per (problem, spec), and
    every later handle must hold the same factor bit for bit"""
    n, ent, _, _, _, (rp, cc, cv) = _launched_problem(name)
    A = ctx.csr(n, n, rp, cc, cv)
    factor = _engine_factor(ctx, A, spec)
    if (name, spec) not in _OP:
        _OP[name, spec] = (factor, po.build(spec, n, ent, factor))
    assert _same_factor(factor, _OP[name, spec][0]), f"{po.label(name, spec)}: two set-ups of the same matrix differ"
    return A


def _launched_envelope(name, spec, zero_start):
    key = ("launched", name, spec, zero_start)
    if key not in _ENV:
        n, ent, b, x0, ks, _ = _launched_problem(name)
        why = br.available(n)
        if why:
            pytest.skip(why)
        _ENV[key] = br.Envelope(ent, n, b, np.zeros_like(x0) if zero_start else x0, ks, _OP[name, spec][1])
    return _ENV[key]


def _steps(ctx, A, name, precond, aligned, what, zero_start=False, spec=None):
    """every k the problem keeps with check_every 1 and 4: iters, x_k and the residual against the reference.  spec: the problem is
    precond_ops', the preconditioner the launched one that A was set up with (_launched_handle), the reference runs over its factor"""
    if spec is None:
        n, ent, b, x0, _, _ = _problem(name)
        env = _envelope(name, precond, zero_start)
    else:
        n, ent, b, x0, _, _ = _launched_problem(name)
        env = _launched_envelope(name, spec, zero_start)
        precond, name = LAUNCHED_ID[spec.kind], po.label(name, spec)
    start = np.zeros_like(x0) if zero_start else x0
    db, keep_b = _device_vector(ctx, b, aligned)
    misses = []
    for k in env.ks:
        for check_every in CHECK_EVERY:
            x, keep_x = _device_vector(ctx, start, aligned)
            iters, res = ctx.bicgstab(A, db, x, max_iter=k, rel_tol=0.0, check_every=check_every, precond=precond)
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


def _csr(ctx, name):
    n, _, _, _, _, (rp, cc, cv) = _problem(name)
    return ctx.csr(n, n, rp, cc, cv)


# ---- 1. every problem as a CSR handle under AUTO: both alignments, plain and Jacobi ------------------------------------------------
CSR_CASES = [(name, precond) for name in br.PROBLEMS[:-1] for precond in (NONE, JACOBI)] + [("big", JACOBI)]


@pytest.mark.parametrize("name,precond", CSR_CASES, ids=lambda v: str(v))
def test_bicgstab_iterates_match_the_extended_precision_recurrence(ctx, pkg, name, precond):
    A = _csr(ctx, name)
    misses = []
    for aligned in (True, False) if name != "big" else (False,):
        misses += _steps(ctx, A, name, precond, aligned, "csr auto")
    assert not misses, "\n".join(misses)
    RUNS["csr"] += 1


@pytest.mark.parametrize("name", ("r33", "r4097"))
def test_bicgstab_iterates_from_a_zero_start(ctx, pkg, name):
    A = _csr(ctx, name)
    misses = []
    for precond, aligned in ((NONE, True), (JACOBI, False)):
        misses += _steps(ctx, A, name, precond, aligned, "csr auto", zero_start=True)
    assert not misses, "\n".join(misses)
    RUNS["zero start"] += 1


# ---- 1b. FSAI, ILU(0), Chebyshev: phat and shat are buffers of their own, written by apply_preconditioner -------------------------
LAUNCHED_CASES = po.BICGSTAB_CASES
LAUNCHED_NAMES = tuple(po.label(name, spec) for name, spec in LAUNCHED_CASES)


@pytest.mark.parametrize("name,spec", LAUNCHED_CASES, ids=lambda v: v if isinstance(v, str) else v.kind)
def test_bicgstab_iterates_under_the_preconditioners_applied_by_launches(ctx, pkg, name, spec):
    """the reference and its twins apply the factor read back from the handle, so a deviation is the solver's: the two applications
    per iteration into phat and shat, the half, update and direction kernels reading them, 16-byte and 8-byte x and b, both starts"""
    A = _launched_handle(ctx, name, spec)
    misses = []
    for aligned, zero_start in ((True, False), (False, False), (True, True), (False, True)) if name != "big" else ((False, False),):
        misses += _steps(ctx, A, name, None, aligned, "csr auto", zero_start, spec)
    assert not misses, "\n".join(misses)
    RUNS["launched"] += 1


# ---- 2. forced product kernels ---------------------------------------------------------------------------------------------------------
KERNEL_CASES = [(name, label, kid) for name in ("r33", "r4097") for label, kid in (("vector", VECTOR), ("scalar", SCALAR))]
KERNEL_CASES += [("r4097", "panel", PANEL)]


@pytest.mark.parametrize("name,label,kid", KERNEL_CASES, ids=lambda v: str(v))
def test_bicgstab_iterates_under_forced_csr_kernels(ctx, pkg, name, label, kid):
    A = _csr(ctx, name)
    A.set_kernel(kid)
    assert A.info.kernel == kid
    misses = []
    for precond, aligned in ((NONE, False), (JACOBI, True)):
        misses += _steps(ctx, A, name, precond, aligned, f"csr {label}")
    assert not misses, "\n".join(misses)
    assert A.info.kernel == kid
    RUNS["kernels"] += 1


# ---- 3. the other formats, on the band -------------------------------------------------------------------------------------------------
def _band_handle(ctx, orc, fmt):
    n, (row, col, val), _, _, _, (rp, cc, cv) = _problem("band4099")
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
    assert len(offsets) == len(br.BAND_OFFSETS)
    return ctx.dia(n, n, offsets, dval)


FORMATS = ("coo", "csc", "ell", "dia")


@pytest.mark.parametrize("fmt", FORMATS)
def test_bicgstab_iterates_on_every_format(ctx, orc, pkg, fmt):
    A = _band_handle(ctx, orc, fmt)
    misses = []
    for aligned in (True, False):
        misses += _steps(ctx, A, "band4099", NONE, aligned, fmt)
    assert not misses, "\n".join(misses)
    RUNS["formats"] += 1


# ---- 4. convergence ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", (NONE, JACOBI))
def test_bicgstab_converges_to_the_tolerance_it_reports(ctx, pkg, precond):
    name, rel_tol = "r4097", 1e-10
    n, ent, b, x0, ks, _ = _problem(name)
    why = br.available(n)
    if why:
        pytest.skip(why)
    A = _csr(ctx, name)
    db, x = ctx.vector_from(b), ctx.vector_from(x0)
    iters, res = ctx.bicgstab(A, db, x, max_iter=500, rel_tol=rel_tol, precond=precond)
    true = br.true_residual(ent, n, b, x.download())
    twin_x, twin_iters = br.run_to_tolerance(ent, n, b, x0, PRECOND_NAME[precond], rel_tol, 500)
    twin_true = br.true_residual(ent, n, b, twin_x)
    print(f"{name} precond {precond}: {iters} iterations (twin {twin_iters}), reported residual {res:.3e}, true {true:.3e} (twin's {twin_true:.3e})")
    assert 0 < iters < 500 and res <= rel_tol, (iters, res)
    assert true <= br.F * max(rel_tol, twin_true), (true, twin_true)
    RUNS["convergence"] += 1


# ---- 5. stopping rules and special cases -------------------------------------------------------------------------------------------------
def test_stopping_rules_and_special_cases(ctx, pkg):
    capi = pkg.capi
    name = "r33"
    n, ent, b, x0, ks, _ = _problem(name)
    A = _csr(ctx, name)
    for aligned in (True, False):
        # b = 0: nothing to do, x stays
        db, kb = _device_vector(ctx, np.zeros(n), aligned)
        x, kx = _device_vector(ctx, x0, aligned)
        assert ctx.bicgstab(A, db, x, max_iter=50, precond=JACOBI) == (0, 0.0)
        assert x.download().tobytes() == x0.tobytes(), "b = 0: x was written"
        # max_iter = 0: x stays, the residual is that of x0
        db, kb = _device_vector(ctx, b, aligned)
        for precond in (NONE, JACOBI):
            env0 = br.Envelope(ent, n, b, x0, (0,), PRECOND_NAME[precond])
            iters, res = ctx.bicgstab(A, db, x, max_iter=0, rel_tol=0.0, precond=precond)
            assert iters == 0 and x.download().tobytes() == x0.tobytes()
            assert env0.resid_dev(0, res) <= env0.gate_resid(0), (res, env0.ref_resid)
        # a start that is already within the tolerance: no iteration either
        iters, res = ctx.bicgstab(A, db, x, max_iter=50, rel_tol=1e3)
        assert iters == 0 and x.download().tobytes() == x0.tobytes() and 0.0 < res <= 1e3
        del db, kb, x, kx
    # t.t = 0: the 5 x 5 identity from x0 = 0 lands on b with the half step: one iteration, x = b and r = 0 exactly
    eye = ctx.csr(5, 5, np.arange(6, dtype=np.int32), np.arange(5, dtype=np.int32), np.ones(5))
    bd = np.array([0.5, -1.25, 2.0, 0.75, -3.0])
    x = ctx.vector_from(np.zeros(5))
    assert ctx.bicgstab(eye, ctx.vector_from(bd), x) == (1, 0.0)
    assert x.download().tobytes() == bd.tobytes()
    # an exact breakdown: the rotation by a quarter turn makes v = A r orthogonal to rhat = r
    rot = ctx.csr(2, 2, np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32), np.array([1.0, -1.0]))
    x = ctx.vector_from(np.zeros(2))
    with pytest.raises(capi.SpmvError) as e:
        ctx.bicgstab(rot, ctx.vector_from(np.array([1.0, 2.0])), x)
    assert e.value.code == INVALID and "spmv_bicgstab" in str(e.value) and "rhat.v" in str(e.value) and "iteration 1" in str(e.value), e.value
    assert x.download().tobytes() == np.zeros(2).tobytes(), "the kernel that saw the breakdown wrote x"
    # a NaN in b: read by the host in b.b, an error and no fault
    bn = b.copy()
    bn[7] = np.nan
    with pytest.raises(capi.SpmvError) as e:
        ctx.bicgstab(A, ctx.vector_from(bn), ctx.vector_from(x0), max_iter=5)
    assert e.value.code == INVALID and "spmv_bicgstab" in str(e.value) and "b.b" in str(e.value), e.value
    # an empty matrix: nothing is launched
    E = ctx.csr(0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    assert ctx.bicgstab(E, ctx.vector(0), ctx.vector(0), max_iter=5) == (0, 0.0)
    RUNS["stopping"] += 1


def test_refusals_are_made_on_the_host(ctx, orc, pkg):
    capi = pkg.capi
    n, ent, b, x0, ks, _ = _problem("r33")
    A = _csr(ctx, "r33")
    db, dx = ctx.vector_from(b), ctx.vector_from(x0)

    def expect(fn, word="spmv_bicgstab", code=INVALID):
        with pytest.raises(capi.SpmvError) as e:
            fn()
        assert e.value.code == code and "spmv_bicgstab" in str(e.value) and word in str(e.value), e.value

    expect(lambda: ctx.bicgstab(A, ctx.vector(n + 1), dx))
    expect(lambda: ctx.bicgstab(A, db, ctx.vector(n - 1)))
    big = ctx.vector(3 * n)
    expect(lambda: ctx.bicgstab(A, ctx.wrap_vector(big.device_ptr, n), ctx.wrap_vector(big.device_ptr + 8 * 5, n)), "overlap")
    expect(lambda: ctx.bicgstab(A, db, dx, max_iter=-1))
    expect(lambda: ctx.bicgstab(A, db, dx, rel_tol=-1e-8))
    expect(lambda: ctx.bicgstab(A, db, dx, precond=7), "preconditioner")
    expect(lambda: ctx.bicgstab(A, db, dx, precond=SYMGS), "Gauss-Seidel", UNSUPPORTED)
    rp, cc, cv = br.csr_arrays(33, *br.rect(33, 17, 6, 7))
    R = ctx.csr(33, 17, rp, cc, cv)
    expect(lambda: ctx.bicgstab(R, db, ctx.vector(17)), "square")
    expect(lambda: ctx.bicgstab(R, db, dx), "square")
    nb = _problem("band4099")[0]
    L = _band_handle(ctx, orc, "ell")
    expect(lambda: ctx.bicgstab(L, ctx.vector(nb), ctx.vector(nb), precond=JACOBI), "Jacobi", UNSUPPORTED)
    assert dx.download().tobytes() == x0.tobytes()
    # a PANEL handle that released its CSR arrays (panel_keep_csr = 0): no diagonal to read, but the forward product is all a plain
    # solve needs
    nb = 1_000_000
    P = ctx.gen_csr_uniform(0, nb, nb, 16, seed=31)
    P.set_kernel(capi.CSR_PANEL)
    P.set_param("panel_keep_csr", 0)
    assert P.get_param("panel_keep_csr") == 0
    pb, px = ctx.gen_vector(nb, seed=5), ctx.vector(nb)
    px.fill(0.0)
    expect(lambda: ctx.bicgstab(P, pb, px, precond=JACOBI), "gave up")
    assert not px.download().any()
    iters, res = ctx.bicgstab(P, pb, px, max_iter=2, rel_tol=0.0)
    assert iters == 2 and np.isfinite(res) and px.download().any()
    RUNS["refusals"] += 1


# ---- 6. reproducibility, the handle's state, device memory -----------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ("dia", "csr vector"))
def test_two_solves_give_the_same_bits(ctx, orc, pkg, fmt):
    """the DIA kernel and the row-parallel CSR kernel add in fixed orders, so what this tests is the dot reduction"""
    n, _, b, x0, _, _ = _problem("band4099")
    A = _band_handle(ctx, orc, fmt.split()[0])
    if fmt == "csr vector":
        A.set_kernel(VECTOR)
    db = ctx.vector_from(b)
    for precond in (NONE,) if fmt == "dia" else (NONE, JACOBI):
        out = []
        for _ in range(2):
            x = ctx.vector_from(x0)
            stats = ctx.bicgstab(A, db, x, max_iter=13, rel_tol=0.0, check_every=4, precond=precond)
            out.append((x.download().tobytes(), stats))
        assert out[0][1][0] == 13 and out[0] == out[1], "two calls on the same data differ"
    RUNS["bits"] += 1


@pytest.mark.parametrize("fmt", ("csr",) + FORMATS)
def test_a_solve_leaves_the_handle_alone(ctx, orc, pkg, fmt):
    n, _, b, x0, _, _ = _problem("band4099")
    A = _band_handle(ctx, orc, fmt)
    plan, kernel, info_bytes, param_bytes = A.get_plan(), A.info.kernel, A.info.device_bytes, A.get_param("device_bytes")
    assert A.get_param("transpose_ready") == 0
    iters, res = ctx.bicgstab(A, ctx.vector_from(b), ctx.vector_from(x0), max_iter=300, rel_tol=1e-9, precond=JACOBI if fmt == "csr" else NONE)
    assert 0 < iters < 300 and res <= 1e-9
    assert A.get_param("transpose_ready") == 0, f"{fmt}: the solve built the transposed state"
    assert A.get_plan() == plan, f"{fmt}: the solve changed the plan"
    assert (A.info.kernel, A.info.device_bytes, A.get_param("device_bytes")) == (kernel, info_bytes, param_bytes), fmt
    RUNS["state"] += 1


def test_work_vectors_go_back_on_every_path(ctx, pkg):
    """75 MB of work vectors per Jacobi solve on the large problem: ten solves that end well and ten that end in an error would
    leave far more than the suite's leak tolerance (tests/test_gpu_parity.py: 256 MiB) behind if a path kept them"""
    import gc

    capi = pkg.capi
    n, _, b, x0, _, _ = _problem("big")
    A = _csr(ctx, "big")
    db, x = ctx.vector_from(b), ctx.vector_from(x0)
    bn = b.copy()
    bn[n // 2] = np.nan
    dbn = ctx.vector_from(bn)
    gc.collect()
    ctx.sync()
    free0, _ = ctx.mem_info()
    for _ in range(10):
        assert ctx.bicgstab(A, db, x, max_iter=2, rel_tol=0.0, precond=JACOBI)[0] == 2
        with pytest.raises(capi.SpmvError):
            ctx.bicgstab(A, dbn, x, max_iter=2, precond=JACOBI)
    ctx.sync()
    free1, _ = ctx.mem_info()
    assert 6 * 8 * n * 10 > 256 << 20
    assert abs(free0 - free1) < 256 << 20, f"{(free0 - free1) >> 20} MiB of device memory not returned"
    RUNS["memory"] += 1


# ---- 7. torch ------------------------------------------------------------------------------------------------------------------------------
def test_torch_solve_is_the_engine_solve_bit_for_bit():
    """tests/child_bicgstab_torch.py in a fresh process: torch initialises its HIP runtime before the engine's library is loaded"""
    import subprocess
    import sys

    child = Path(__file__).with_name("child_bicgstab_torch.py")
    r = subprocess.run([sys.executable, str(child)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "BICGSTAB_TORCH_OK" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    RUNS["torch"] += 1


# ---- 8. coverage ---------------------------------------------------------------------------------------------------------------------------
def test_every_case_ran():
    """every problem, kernel and format of the cases above ran, and no ratio lies above the gate"""
    expect = {"csr": len(CSR_CASES), "zero start": 2, "kernels": len(KERNEL_CASES), "formats": len(FORMATS), "convergence": 2, "stopping": 1,
              "launched": len(LAUNCHED_CASES), "refusals": 1, "bits": 2, "state": 1 + len(FORMATS), "memory": 1, "torch": 1}
    if any(RUNS[f] != c for f, c in expect.items()):
        pytest.skip(f"the coverage check needs every test of this module (ran {dict(RUNS)}, expected {expect})")
    names = br.PROBLEMS + LAUNCHED_NAMES
    assert set(RATIO) == set(names), sorted(set(names) ^ set(RATIO))
    lines = ["# spmv_bicgstab iterate by iterate (tests/test_gpu_bicgstab.py): the largest deviation of the GPU's x_k and of its ||r_k|| / ||b||",
             "# from the np.longdouble recurrence, in units of the float64 twins' own largest deviation at that k (the gate is 8).",
             "# problem | x ratio | residual ratio | where the x ratio was largest"]
    for name in names:
        r = RATIO[name]
        lines.append(f"{name:18s}  x {r['x'][0]:6.3f}  residual {r['residual'][0]:6.3f}  ({r['x'][1]})")
    print("\n".join(lines))
    out = os.environ.get("SPMV_BICGSTAB_RATIOS")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    for name in names:
        assert all(RATIO[name][kind][0] <= br.F for kind in RATIO[name]), (name, RATIO[name])
