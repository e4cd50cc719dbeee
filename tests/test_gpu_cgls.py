"""spmv_cgls - least squares over A and A^T - iterate by iterate against the extended-precision recurrence (`pytest -m gpu`).

spmv_cgls(max_iter = k, rel_tol = 0) runs exactly k iterations from the x passed in.  For k in (1, 2, 3, 4, 5, 8, 9, 13) and with
the host looking every iteration and every fourth, x_k and both returned residuals - sqrt(gamma_k) / ||A^T b|| and ||r_k|| / ||b|| -
are held to CGLS in np.longdouble (tests/cgls_ref.py).  The gate at step k is F = 8 times the largest deviation from that reference
of any float64 twin of the recurrence (three dot orders x two orders of a row's products), measured on the reference's own
arithmetic and floored at 2^-50.  What the gate catches - a wrong beta, delta without its damping term, an s that was not reset
before the transposed product, an element of x left out - is checked on the CPU in tests/test_cgls_ref.py.

Problems: 1 x 1, 2 x 1, 3 x 2; 33 x 17; 4097 x 4097 (square, not symmetric); 6001 x 4097; 4097 x 6001 (columns that carry random
entries only, some none at all); a 4099 x 4093 band of seven diagonals; and one whose nrow and ncol are both odd and beyond two
sweeps of the vector kernels' largest grid (csrc/common.hpp: 2 * kMaxGrid * kBlock).  CSR under AUTO and forced VECTOR, SCALAR and
PANEL; COO (entries shuffled), CSC, ELL and DIA handles of the band; the transposed side's kernel at AUTO and forced; x and b 256-byte
aligned (the 16-byte kernels) and 8 bytes past a 16-byte boundary (the 8-byte kernels); a random start and x0 = 0; damp 0 and 0.5.
Then convergence to 1e-10 against the true normal residual, the stopping rules, refusals, reproducibility bit for bit on the DIA
handle, the handle's forward state and the device memory before and after, and the torch operator.  test_every_case_ran asserts
at the end that all of it ran; with SPMV_CGLS_RATIOS=<file> it also writes the largest GPU deviation over twin envelope per
problem (profiles/cgls_steps_gpu_vs_twin_envelope.txt).
"""
import collections
import os
import re
from pathlib import Path

import numpy as np
import pytest

import cgls_ref as cr
import oracle_lib as ol

pytestmark = pytest.mark.gpu
AUTO, VECTOR, SCALAR, PANEL = 0, 1, 3, 4
INVALID = -1
CHECK_EVERY = (1, 4)
RUNS = collections.Counter()
RATIO = {}  # problem -> {"x" | "normal residual" | "residual": (largest deviation / twin envelope, where)}
_MAT = {}
_ENV = {}


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


def _big_shape():
    block, max_grid = _grid_constants()
    sweep2 = 2 * max_grid * block
    return sweep2 + 2051, sweep2 + 3  # both odd, both beyond one sweep of the one- and of the two-element grids


def _problem(name):
    if name not in _MAT:
        shape, ent, b, x0, ks = cr.problem(name, _big_shape() if name == "big" else None)
        _MAT[name] = (shape, ent, b, x0, ks, cr.csr_arrays(shape[0], *ent))
    return _MAT[name]


def _envelope(name, damp, zero_start=False):
    """the reference iterates and twin envelopes of one problem (computed once and shared)"""
    key = (name, damp, zero_start)
    if key not in _ENV:
        shape, ent, b, x0, ks, _ = _problem(name)
        why = cr.available(max(shape))
        if why:
            pytest.skip(why)
        _ENV[key] = cr.Envelope(ent, shape, b, np.zeros_like(x0) if zero_start else x0, ks, damp)
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
    if ratio > old.get(kind, (0.0, ""))[0]:
        old[kind] = (ratio, where)


def _steps(ctx, A, name, damp, aligned, what, zero_start=False):
    """every k of the problem's list with check_every 1 and 4: iters, x_k and both residuals against the reference"""
    shape, ent, b, x0, ks, _ = _problem(name)
    env = _envelope(name, damp, zero_start)
    start = np.zeros_like(x0) if zero_start else x0
    db, keep_b = _device_vector(ctx, b, aligned)
    misses = []
    for k in ks:
        for check_every in CHECK_EVERY:
            x, keep_x = _device_vector(ctx, start, aligned)
            iters, nres, res = ctx.cgls(A, db, x, max_iter=k, rel_tol=0.0, check_every=check_every, damp=damp)
            got = x.download()
            del x, keep_x
            tag = f"{name} {what} damp={damp} {'aligned' if aligned else 'offset'}{' x0=0' if zero_start else ''} k={k} check_every={check_every}"
            assert iters == k, (tag, iters)
            dev, ndev, rdev = env.x_dev(k, got), env.nres_dev(k, nres), env.resid_dev(k, res)
            print(f"{tag}: x deviation {dev:.2e} (twins {env.envelope(k):.2e}, gate {env.gate(k):.2e}); normal residual {nres:.6e} deviation "
                  f"{ndev:.2e} (gate {env.gate_nres(k):.2e}); residual {res:.6e} deviation {rdev:.2e} (gate {env.gate_resid(k):.2e})")
            _note(name, "x", dev / env.envelope(k), tag)
            _note(name, "normal residual", ndev / env.envelope(k, 1), tag)
            _note(name, "residual", rdev / env.envelope(k, 2), tag)
            if not dev <= env.gate(k):
                misses.append(f"{tag}: max|x_k - ref_k| / max|ref_k| = {dev:.3e} > gate {env.gate(k):.3e}")
            if not ndev <= env.gate_nres(k):
                misses.append(f"{tag}: rel_normal_resid {nres!r} against {env.ref_nres[k]!r}: {ndev:.3e} > gate {env.gate_nres(k):.3e}")
            if not rdev <= env.gate_resid(k):
                misses.append(f"{tag}: rel_resid {res!r} against {env.ref_resid[k]!r}: {rdev:.3e} > gate {env.gate_resid(k):.3e}")
    del db, keep_b
    return misses


def _csr(ctx, name):
    (m, n), _, _, _, _, (rp, cc, cv) = _problem(name)
    return ctx.csr(m, n, rp, cc, cv)


# ---- 1. every problem as a CSR handle under AUTO: both alignments, both damps --------------------------------------------------------
CSR_CASES = [(name, damp) for name in cr.PROBLEMS[:-1] for damp in (0.0, 0.5)] + [("big", 0.5)]


@pytest.mark.parametrize("name,damp", CSR_CASES, ids=lambda v: str(v))
def test_cgls_iterates_match_the_extended_precision_recurrence(ctx, pkg, name, damp):
    A = _csr(ctx, name)
    misses = []
    for aligned in (True, False):
        misses += _steps(ctx, A, name, damp, aligned, "csr auto")
    assert not misses, "\n".join(misses)
    RUNS["csr"] += 1


@pytest.mark.parametrize("name", ("r33x17", "r6001x4097"))
def test_cgls_iterates_from_a_zero_start(ctx, pkg, name):
    A = _csr(ctx, name)
    misses = []
    for damp, aligned in ((0.0, True), (0.5, False)):
        misses += _steps(ctx, A, name, damp, aligned, "csr auto", zero_start=True)
    assert not misses, "\n".join(misses)
    RUNS["zero start"] += 1


# ---- 2. forced product kernels, on both sides ----------------------------------------------------------------------------------------
KERNEL_CASES = [(name, label, kid) for name in ("r33x17", "r4097x6001") for label, kid in (("vector", VECTOR), ("scalar", SCALAR))]
KERNEL_CASES += [(name, "panel", PANEL) for name in ("r4097x4097", "r6001x4097", "r4097x6001")]


@pytest.mark.parametrize("name,label,kid", KERNEL_CASES, ids=lambda v: str(v))
def test_cgls_iterates_under_forced_csr_kernels(ctx, pkg, name, label, kid):
    A = _csr(ctx, name)
    A.set_kernel(kid)
    assert A.info.kernel == kid
    misses = []
    for damp, aligned in ((0.0, False), (0.5, True)):
        misses += _steps(ctx, A, name, damp, aligned, f"csr {label}")
    assert not misses, "\n".join(misses)
    assert A.info.kernel == kid
    RUNS["kernels"] += 1


def test_cgls_iterates_with_the_transposed_kernel_forced(ctx, pkg):
    name = "r6001x4097"
    A = _csr(ctx, name)
    A.set_param("transpose_kernel", VECTOR)  # the CSC companion's own kernel instead of AUTO's pick
    misses = _steps(ctx, A, name, 0.5, True, "csr auto, transposed vector") + _steps(ctx, A, name, 0.0, False, "csr auto, transposed vector")
    assert not misses, "\n".join(misses)
    assert A.get_param("transpose_kernel") == VECTOR and A.get_param("transpose_ready") == 1
    RUNS["transpose kernel"] += 1


# ---- 3. the other formats, on the band ---------------------------------------------------------------------------------------------------
def _band_handle(ctx, orc, fmt):
    (m, n), (row, col, val), _, _, _, (rp, cc, cv) = _problem("band4099")
    if fmt == "csr":
        return ctx.csr(m, n, rp, cc, cv)
    if fmt == "coo":
        o = np.random.default_rng(5).permutation(len(row))
        return ctx.coo(m, n, ol.i32(row[o]), ol.i32(col[o]), ol.f64(val[o]))
    if fmt == "csc":
        cp, cri, ccv = ol.coo_to_csc(orc, n, ol.i32(row), ol.i32(col), ol.f64(val))
        return ctx.csc(m, n, cp, cri, ccv)
    if fmt == "ell":
        k, ec, ev = ol.coo_to_ell(orc, m, ol.i32(row), ol.i32(col), ol.f64(val))
        return ctx.ell(m, n, k, len(val), ec, ev)
    offsets, dval = ol.csr_to_dia(orc, m, n, rp, cc, cv)
    assert len(offsets) == len(cr.BAND_OFFSETS)
    return ctx.dia(m, n, offsets, dval)


FORMATS = ("coo", "csc", "ell", "dia")


@pytest.mark.parametrize("fmt", FORMATS)
def test_cgls_iterates_on_every_format(ctx, orc, pkg, fmt):
    A = _band_handle(ctx, orc, fmt)
    misses = []
    for damp, aligned in ((0.0, True), (0.5, False)):
        misses += _steps(ctx, A, "band4099", damp, aligned, fmt)
    assert not misses, "\n".join(misses)
    RUNS["formats"] += 1


# ---- 4. convergence ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("damp", (0.0, 0.5))
def test_cgls_converges_to_the_tolerance_it_reports(ctx, pkg, damp):
    name, rel_tol = "r6001x4097", 1e-10
    shape, ent, b, x0, ks, _ = _problem(name)
    why = cr.available(max(shape))
    if why:
        pytest.skip(why)
    A = _csr(ctx, name)
    db, x = ctx.vector_from(b), ctx.vector_from(x0)
    iters, nres, res = ctx.cgls(A, db, x, max_iter=500, rel_tol=rel_tol, damp=damp)
    true = cr.true_normal_residual(ent, shape, b, x.download(), damp)
    twin_x, twin_iters = cr.run_to_tolerance(ent, shape, b, x0, damp, rel_tol, 500)
    twin_true = cr.true_normal_residual(ent, shape, b, twin_x, damp)
    print(f"{name} damp {damp}: {iters} iterations (twin {twin_iters}), reported normal residual {nres:.3e}, true {true:.3e} (twin's {twin_true:.3e}), "
          f"residual {res:.3e}")
    assert 0 < iters < 500 and nres <= rel_tol, (iters, nres)
    assert true <= cr.F * max(rel_tol, twin_true), (true, twin_true)
    RUNS["convergence"] += 1


# ---- 5. stopping rules --------------------------------------------------------------------------------------------------------------------
def test_stopping_rules(ctx, pkg):
    capi = pkg.capi
    name = "r33x17"
    (m, n), ent, b, x0, ks, (rp, cc, cv) = _problem(name)
    A = _csr(ctx, name)
    for aligned in (True, False):
        # b = 0: nothing to do, x stays
        db, kb = _device_vector(ctx, np.zeros(m), aligned)
        x, kx = _device_vector(ctx, x0, aligned)
        assert ctx.cgls(A, db, x, max_iter=50, damp=0.5) == (0, 0.0, 0.0)
        assert x.download().tobytes() == x0.tobytes(), "b = 0: x was written"
        # max_iter = 0: x stays, the residuals are those of x0
        for damp in (0.0, 0.5):
            env0 = cr.Envelope(ent, (m, n), b, x0, (0,), damp)
            db, kb = _device_vector(ctx, b, aligned)
            iters, nres, res = ctx.cgls(A, db, x, max_iter=0, rel_tol=0.0, damp=damp)
            assert iters == 0 and x.download().tobytes() == x0.tobytes()
            assert env0.nres_dev(0, nres) <= env0.gate_nres(0) and env0.resid_dev(0, res) <= env0.gate_resid(0), (nres, res, env0.ref_nres, env0.ref_resid)
        del db, kb, x, kx
    # b orthogonal to the range of A: row 5 of A is empty and b = e_5, so A^T b = 0 although b is not
    keep = ent[0] != 5
    rp0, cc0, cv0 = cr.csr_arrays(m, ent[0][keep], ent[1][keep], ent[2][keep])
    Z = ctx.csr(m, n, rp0, cc0, cv0)
    e5 = np.zeros(m)
    e5[5] = 1.0
    x = ctx.vector_from(x0)
    assert ctx.cgls(Z, ctx.vector_from(e5), x, max_iter=50) == (0, 0.0, 0.0)
    assert x.download().tobytes() == x0.tobytes(), "A^T b = 0: x was written"
    # a NaN in b: read by the host in b.b, an error and no fault
    bn = b.copy()
    bn[7] = np.nan
    with pytest.raises(capi.SpmvError) as e:
        ctx.cgls(A, ctx.vector_from(bn), ctx.vector_from(x0), max_iter=5)
    assert e.value.code == INVALID and "spmv_cgls" in str(e.value) and "b.b" in str(e.value), e.value
    # an empty matrix: nothing is launched
    for mm, nn in ((0, 4), (4, 0)):
        E = ctx.csr(mm, nn, np.zeros(mm + 1, np.int32), np.zeros(0, np.int32), np.zeros(0))
        assert ctx.cgls(E, ctx.vector(mm), ctx.vector(nn), max_iter=5) == (0, 0.0, 0.0)
    RUNS["stopping"] += 1


def test_refusals_are_made_on_the_host(ctx, pkg):
    capi = pkg.capi
    (m, n), ent, b, x0, ks, _ = _problem("r33x17")
    A = _csr(ctx, "r33x17")
    db, dx = ctx.vector_from(b), ctx.vector_from(x0)

    def expect(fn, word="spmv_cgls"):
        with pytest.raises(capi.SpmvError) as e:
            fn()
        assert e.value.code == INVALID and "spmv_cgls" in str(e.value) and word in str(e.value), e.value

    expect(lambda: ctx.cgls(A, ctx.vector(m + 1), dx))
    expect(lambda: ctx.cgls(A, db, ctx.vector(n - 1)))
    expect(lambda: ctx.cgls(A, dx, db))  # the lengths the other way round
    big = ctx.vector(3 * m)
    expect(lambda: ctx.cgls(A, ctx.wrap_vector(big.device_ptr, m), ctx.wrap_vector(big.device_ptr + 8 * 5, n)), "overlap")
    expect(lambda: ctx.cgls(A, db, dx, max_iter=-1))
    expect(lambda: ctx.cgls(A, db, dx, rel_tol=-1e-8))
    expect(lambda: ctx.cgls(A, db, dx, damp=-0.5), "damp")
    expect(lambda: ctx.cgls(A, db, dx, damp=float("nan")), "damp")
    expect(lambda: ctx.cgls(A, db, dx, damp=float("inf")), "damp")
    assert dx.download().tobytes() == x0.tobytes()
    # a PANEL handle that released its CSR arrays (panel_keep_csr = 0): nothing left to read the other way round
    nb = 1_000_000
    P = ctx.gen_csr_uniform(0, nb, nb, 16, seed=31)
    P.set_kernel(capi.CSR_PANEL)
    P.set_param("panel_keep_csr", 0)
    assert P.get_param("panel_keep_csr") == 0
    expect(lambda: ctx.cgls(P, ctx.vector(nb), ctx.vector(nb)), "gave up")
    RUNS["refusals"] += 1


# ---- 6. reproducibility, the handle's state, device memory -----------------------------------------------------------------------------
def test_two_solves_on_the_dia_handle_give_the_same_bits(ctx, orc, pkg):
    """the DIA forward and transposed kernels add in fixed orders, so what this tests is the dot reduction"""
    (m, n), _, b, x0, _, _ = _problem("band4099")
    A = _band_handle(ctx, orc, "dia")
    db = ctx.vector_from(b)
    for damp in (0.0, 0.5):
        out = []
        for _ in range(2):
            x = ctx.vector_from(x0)
            stats = ctx.cgls(A, db, x, max_iter=13, rel_tol=0.0, check_every=4, damp=damp)
            out.append((x.download().tobytes(), stats))
        assert out[0][1][0] == 13 and out[0] == out[1], "two calls on the same data differ"
    RUNS["bits"] += 1


@pytest.mark.parametrize("fmt", ("csr",) + FORMATS)
def test_a_solve_leaves_the_forward_state_alone(ctx, orc, pkg, fmt):
    (m, n), _, b, x0, _, _ = _problem("band4099")
    A = _band_handle(ctx, orc, fmt)
    plan, kernel, info_bytes, param_bytes = A.get_plan(), A.info.kernel, A.info.device_bytes, A.get_param("device_bytes")
    assert A.get_param("transpose_ready") == 0
    iters, nres, _ = ctx.cgls(A, ctx.vector_from(b), ctx.vector_from(x0), max_iter=300, rel_tol=1e-9, damp=0.5)
    assert 0 < iters < 300 and nres <= 1e-9
    assert A.get_param("transpose_ready") == 1 and A.get_param("transpose_bytes") >= 0
    assert A.get_plan() == plan, f"{fmt}: the solve changed the plan"
    assert (A.info.kernel, A.info.device_bytes, A.get_param("device_bytes")) == (kernel, info_bytes, param_bytes), fmt
    RUNS["state"] += 1


def test_work_vectors_go_back_on_every_path(ctx, pkg):
    """33 MB of work vectors per solve on the large problem: ten solves that end well and ten that end in an error would leave
    far more than the suite's leak tolerance (tests/test_gpu_parity.py: 256 MiB) behind if a path kept them"""
    import gc

    capi = pkg.capi
    (m, n), _, b, x0, _, _ = _problem("big")
    A = _csr(ctx, "big")
    A.transpose_setup()  # (the transposed state stays with the handle: built before the first measurement)
    db, x = ctx.vector_from(b), ctx.vector_from(x0)
    bn = b.copy()
    bn[m // 2] = np.nan
    dbn = ctx.vector_from(bn)
    gc.collect()
    ctx.sync()
    free0, _ = ctx.mem_info()
    for _ in range(10):
        assert ctx.cgls(A, db, x, max_iter=2, rel_tol=0.0, damp=0.5)[0] == 2
        with pytest.raises(capi.SpmvError):
            ctx.cgls(A, dbn, x, max_iter=2)
    ctx.sync()
    free1, _ = ctx.mem_info()
    assert 4 * 8 * min(m, n) * 10 > 256 << 20
    assert abs(free0 - free1) < 256 << 20, f"{(free0 - free1) >> 20} MiB of device memory not returned"
    RUNS["memory"] += 1


# ---- 7. torch ------------------------------------------------------------------------------------------------------------------------------
def test_torch_lstsq_is_the_engine_solve_bit_for_bit():
    """tests/child_cgls_torch.py in a fresh process: torch initialises its HIP runtime before the engine's library is loaded"""
    import subprocess
    import sys

    child = Path(__file__).with_name("child_cgls_torch.py")
    r = subprocess.run([sys.executable, str(child)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "CGLS_TORCH_OK" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    RUNS["torch"] += 1


# ---- 8. coverage ---------------------------------------------------------------------------------------------------------------------------
def test_every_case_ran():
    """every problem, kernel and format of the cases above ran, and no ratio lies above the gate"""
    expect = {"csr": len(CSR_CASES), "zero start": 2, "kernels": len(KERNEL_CASES), "transpose kernel": 1, "formats": len(FORMATS), "convergence": 2,
              "stopping": 1, "refusals": 1, "bits": 1, "state": 1 + len(FORMATS), "memory": 1, "torch": 1}
    if any(RUNS[f] != c for f, c in expect.items()):
        pytest.skip(f"the coverage check needs every test of this module (ran {dict(RUNS)}, expected {expect})")
    assert set(RATIO) == set(cr.PROBLEMS), sorted(set(cr.PROBLEMS) - set(RATIO))
    lines = ["# spmv_cgls iterate by iterate (tests/test_gpu_cgls.py): the largest deviation of the GPU's x_k, of its sqrt(gamma_k) / ||A^T b||",
             "# and of its ||r_k|| / ||b|| from the np.longdouble recurrence, in units of the float64 twins' own largest deviation at that k",
             "# (the gate is 8).  problem | x ratio | normal residual ratio | residual ratio | where the x ratio was largest"]
    for name in cr.PROBLEMS:
        r = RATIO[name]
        lines.append(f"{name:12s}  x {r['x'][0]:6.3f}  normal residual {r['normal residual'][0]:6.3f}  residual {r['residual'][0]:6.3f}  ({r['x'][1]})")
        assert all(r[kind][0] <= cr.F for kind in r)
    print("\n".join(lines))
    out = os.environ.get("SPMV_CGLS_RATIOS")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
