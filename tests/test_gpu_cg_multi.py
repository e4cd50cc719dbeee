"""spmv_cg_multi - k conjugate-gradient solves in one loop - column by column against the extended-precision recurrence
(`pytest -m gpu`).

spmv_cg_multi(max_iter = j, rel_tol = 0) runs exactly j iterations of every column from the X passed in.  For j in the problem's list
(tests/solver_ref.py: KS) every column's x_j and rel_resid[c] are held to that column's own np.longdouble recurrence with the gate of
tests/test_gpu_solver_steps.py, unchanged: F = 8 times the float64 twins' largest deviation at that j (solver_ref.Envelope).  Column
0 is solver_ref.problem's b and x0, column 1 comes from a second seed, column c >= 2 is 2^(c // 2) times column c % 2, whose reference
is the scaled reference (tests/solver_multi_ref.py) - two Envelopes per problem.  What the gate catches - a column that takes its
neighbour's alpha or gamma_old, a frozen column still updated, a row of X left out - is checked on the CPU in
tests/test_solver_multi_ref.py.

Shapes: n = 1, 2, 3 at k = 1, 3; the 33 x 33 Laplacian at k = 1, 3, 8, 17, 64 (lanes masked, two columns per lane, 4 rows per
workgroup); the 4097-row system (odd n, diagonal stored twice, unsorted columns) at k = 3, 17, plain and Jacobi; the Laplacian of
n = 525,625 at k = 3 (eight sweeps of the grid-stride loop); the two mid-size systems as ELL handles.  Each with X 256-byte aligned
(k even: the 16-byte kernels) and with X 8 bytes past a 16-byte boundary (the 8-byte kernels), and with the host looking at the
residual after every iteration and only at the end.  Then, bit for bit: two calls give the same X and a column does not depend on
its neighbours; a column with b = 0 and a column that x0 already solves stay untouched and report 0 iterations next to ordinary
columns that converge; a frozen column is the column of a solve that stopped there.  Refusals; spmv_cg before and after;
test_every_combination_ran asserts at the end that all of it ran, and with SPMV_SOLVER_MULTI_RATIOS=<file> writes the largest
deviation over twin envelope per combination (profiles/r09_cg_multi_ratios.txt).
"""
import collections
import os

import numpy as np
import pytest

import oracle_lib as ol
import solver_multi_ref as mr
import solver_ref as sr

pytestmark = pytest.mark.gpu
SCALAR = 3
UNSUPPORTED, INVALID = -5, -1
SEEN = set()  # (k, "aligned" | "offset", "plain" | "jacobi", "csr" | "ell")
RUNS = collections.Counter()
RATIO = {}
_MAT = {}
_CG_BEFORE = {}


def _problem(name, k):
    if (name, k) not in _MAT:
        n, ent, B, X0, ks = mr.columns(name, k)
        _MAT[name, k] = (n, ent, B, X0, ks, sr.csr_arrays(n, *ent))
    return _MAT[name, k]


def _envelopes(name, precond):
    n = sr.problem(name)[0]
    why = sr.available(n)
    if why:
        pytest.skip(why)
    return mr.envelopes(name, precond)


def _start_block(ctx, X0, aligned):
    """X0 (n, k) row-major on the device, 256-byte aligned (spmv_vec_create) or 8 bytes past a 16-byte boundary (a wrapped pointer
    into a vector of n * k + 1: an ordinary, legal double*)"""
    flat = np.ascontiguousarray(X0).ravel()
    if aligned:
        v = ctx.vector_from(flat)
        assert v.device_ptr % 16 == 0
        return v, None
    base = ctx.vector(flat.size + 1)
    base.fill(0.0)
    ptr = base.device_ptr + 8
    assert ptr % 16 == 8
    v = ctx.wrap_vector(ptr, flat.size)
    v.upload(flat)
    return v, base


def _note(key, kind, ratio, where):
    old = RATIO.setdefault(key, {})
    if ratio > old.get(kind, (0.0, ""))[0]:
        old[kind] = (ratio, where)


def _steps(ctx, A, name, k, envs, jacobi, aligned, fmt):
    """every j of the problem's list with check_every in {1, j}: iters, and every column's x_j and rel_resid against its reference"""
    n, ent, B, X0, ks, _ = _problem(name, k)
    dB = ctx.vector_from(B.ravel())
    key = (k, "aligned" if aligned else "offset", "jacobi" if jacobi else "plain", fmt)
    misses = []
    for j in ks:
        for check_every in ((j,) if j == 1 else (1, j)):
            X, keep = _start_block(ctx, X0, aligned)
            iters, relres = ctx.cg_multi(A, dB, X, k, max_iter=j, rel_tol=0.0, check_every=check_every, jacobi=jacobi)
            got = X.download().reshape(n, k)
            del X, keep
            tag = f"{name} {fmt} k={k} {key[2]} {key[1]} j={j} check_every={check_every}"
            assert iters.dtype == np.int32 and relres.dtype == np.float64 and len(iters) == k == len(relres)
            assert np.all(iters == j), (tag, iters)
            worst = (0.0, 0.0, 0)
            for c in range(k):
                env = envs[c % 2]
                dev, rdev = mr.column_dev(envs, c, j, got[:, c], relres[c])
                worst = max(worst, (dev / env.envelope(j), rdev / env.envelope(j, 1), c))
                _note(key, "x", dev / env.envelope(j), f"{tag} column {c}")
                _note(key, "residual", rdev / env.envelope(j, 1), f"{tag} column {c}")
                if not dev <= env.gate(j):
                    misses.append(f"{tag} column {c}: max|x_j - ref_j| / max|ref_j| = {dev:.3e} > gate {env.gate(j):.3e}")
                if not rdev <= env.gate_resid(j):
                    misses.append(f"{tag} column {c}: rel_resid {relres[c]!r} against {env.ref_resid[j]!r}: {rdev:.3e} > gate {env.gate_resid(j):.3e}")
            print(f"{tag}: largest x deviation / twin envelope {worst[0]:.2f}, residual {worst[1]:.2f} (gate {sr.F:g})")
    SEEN.add(key)
    return misses


# ---- 6a. spmv_cg before any multi-column solve (the first test of the module) -----------------------------------------------------
def _cg_scalar_run(ctx):
    n, ent, b, x0, ks = sr.problem("rand4097")
    rp, cc, cv = sr.csr_arrays(n, *ent)
    A = ctx.csr(n, n, rp, cc, cv)
    A.set_kernel(SCALAR)
    assert A.info.kernel == SCALAR
    env = _envelopes("rand4097", None)[0]
    db = ctx.vector_from(b)
    x = ctx.vector_from(x0)
    iters, res = ctx.cg(A, db, x, max_iter=1000, rel_tol=1e-10)
    out = {"iters": iters, "res": res, "dev": {}}
    for j in ks:
        x = ctx.vector_from(x0)
        it, rr = ctx.cg(A, db, x, max_iter=j, rel_tol=0.0, check_every=j)
        assert it == j
        out["dev"][j] = (env.x_dev(j, x.download()), env.resid_dev(j, rr))
        assert out["dev"][j][0] <= env.gate(j) and out["dev"][j][1] <= env.gate_resid(j), (j, out["dev"][j])
    return out


def test_spmv_cg_before_any_multi_column_solve(ctx, pkg):
    assert not RUNS, "this test must run before the first spmv_cg_multi of the module"
    _CG_BEFORE.update(_cg_scalar_run(ctx))
    assert 0 < _CG_BEFORE["iters"] < 1000 and _CG_BEFORE["res"] <= 1e-10


# ---- 1. iterates against the extended-precision recurrence -------------------------------------------------------------------------
CASES = [(name, k, False, "csr") for name in ("n1", "n2", "n3") for k in (1, 3)]
CASES += [("lap33", k, False, "csr") for k in (1, 3, 8, 17, 64)]
CASES += [("lap33", 8, True, "csr")]  # two columns per lane with the diagonal
CASES += [("rand4097", k, jac, "csr") for k in (3, 17) for jac in (False, True)]
CASES += [("lap725", 3, False, "csr")]
CASES += [(name, k, False, "ell") for name in ("lap33", "rand4097") for k in (3, 8)]


@pytest.mark.parametrize("name,k,jacobi,fmt", CASES, ids=lambda v: str(v))
def test_every_column_matches_its_extended_precision_recurrence(ctx, pkg, name, k, jacobi, fmt):
    n, ent, B, X0, ks, (rp, cc, cv) = _problem(name, k)
    A = ctx.csr(n, n, rp, cc, cv)
    if fmt == "ell":
        A = ctx.csr_to_ell(A)
    envs = _envelopes(name, "jacobi" if jacobi else None)
    misses = []
    for aligned in (True, False):
        misses += _steps(ctx, A, name, k, envs, jacobi, aligned, fmt)
    assert not misses, "\n".join(misses)
    RUNS["steps"] += 1


# ---- 2. column independence and determinism, bit for bit ---------------------------------------------------------------------------
def test_a_column_is_independent_of_its_neighbours_and_two_calls_agree(ctx, pkg):
    n, ent, B, X0, ks, (rp, cc, cv) = _problem("rand4097", 3)
    A = ctx.csr(n, n, rp, cc, cv)

    def solve(Bm, Xm, jacobi):
        dB, dX = ctx.vector_from(np.ascontiguousarray(Bm).ravel()), ctx.vector_from(np.ascontiguousarray(Xm).ravel())
        iters, res = ctx.cg_multi(A, dB, dX, 3, max_iter=13, rel_tol=0.0, check_every=4, jacobi=jacobi)
        return dX.download().reshape(n, 3), iters, res

    rng = np.random.default_rng(99)
    for jacobi in (False, True):
        first, it1, res1 = solve(B, X0, jacobi)
        again, it2, res2 = solve(B, X0, jacobi)
        assert first.tobytes() == again.tobytes(), "two calls on the same data differ"
        assert np.array_equal(it1, it2) and res1.tobytes() == res2.tobytes()
        B2, X2 = B.copy(), X0.copy()
        B2[:, 1], X2[:, 1] = rng.uniform(-1e6, 1e6, n), rng.uniform(-1e-3, 1e-3, n)  # junk
        B2[:, 2], X2[:, 2] = 0.0, 0.0
        other, it3, res3 = solve(B2, X2, jacobi)
        assert other[:, 0].tobytes() == first[:, 0].tobytes(), "column 0 depends on what columns 1 and 2 hold"
        assert it3[0] == 13 and res3[0] == res1[0] and it3[2] == 0 and res3[2] == 0.0 and np.all(other[:, 2] == 0.0)
    RUNS["bits"] += 1


# ---- 3. the zero column and the solved column ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("check_every,rel_tol", ((1, 1e-10), (5, 1e-10), (5, mr.MARGIN_REL_TOL)))
def test_a_zero_column_and_a_solved_column_stay_untouched(ctx, orc, pkg, check_every, rel_tol):
    n, ent, B, X0, kinds, _ = mr.special_columns()
    rp, cc, cv = sr.csr_arrays(n, *ent)
    A = ctx.csr(n, n, rp, cc, cv)
    S = sr.System(ent, n, "f64")
    _, t_iters, _, kept = mr.run_multi(S, B, X0, 1000, rel_tol, check_every)
    bb = np.einsum("ic,ic->c", B, B)
    for aligned in (True, False):
        dB = ctx.vector_from(B.ravel())
        dX, keep = _start_block(ctx, X0, aligned)
        iters, res = ctx.cg_multi(A, dB, dX, 4, max_iter=1000, rel_tol=rel_tol, check_every=check_every)
        got = dX.download().reshape(n, 4)
        assert not np.isnan(got).any() and not np.isnan(res).any()
        for c in (1, 2):
            assert iters[c] == 0 and res[c] == 0.0, (kinds[c], iters, res)
            assert got[:, c].tobytes() == X0[:, c].tobytes(), f"the {kinds[c]} column was written"
        for c in (0, 3):
            assert 0 < iters[c] < 1000 and iters[c] != iters[1] and res[c] <= rel_tol, (iters, res)
            assert iters[c] % check_every == 0
            y = np.zeros(n)
            ol.csr_spmv(orc, rp, cc, cv, np.ascontiguousarray(got[:, c]), y, fma=True)
            true = float(np.linalg.norm(B[:, c] - y) / np.linalg.norm(B[:, c]))
            under, over = mr.stopping_margin(kept, bb, c, rel_tol, check_every, int(t_iters[c]))
            print(f"lap33 special columns rel_tol {rel_tol:g} check_every {check_every} column {c}: iters {iters[c]} (twin {t_iters[c]}, "
                  f"its margins {under:.2f} / {over:.2f}), rel_resid {res[c]:.3e}, true residual {true:.3e}")
            assert true <= 4 * rel_tol, (c, true)
            if under >= 2 and over >= 2:
                assert iters[c] == t_iters[c], (c, iters, t_iters)
            if rel_tol == mr.MARGIN_REL_TOL:
                assert under >= 2 and over >= 2, "MARGIN_REL_TOL is chosen so that the twin's look binds (tests/test_solver_multi_ref.py)"
        del dX, keep
    RUNS["special"] += 1


# ---- 4. freeze -------------------------------------------------------------------------------------------------------------------------
def test_a_frozen_column_is_the_column_of_a_solve_that_stopped_there(ctx, pkg):
    n, ent, B, X0 = mr.freeze_columns()
    rp, cc, cv = sr.csr_arrays(n, *ent)
    A = ctx.csr(n, n, rp, cc, cv)
    for aligned in (True, False):
        out = []
        for max_iter in (1000, None):
            dB = ctx.vector_from(B.ravel())
            dX, keep = _start_block(ctx, X0, aligned)
            iters, res = ctx.cg_multi(A, dB, dX, 2, max_iter=max_iter or int(out[0][1][0]), rel_tol=1e-8, check_every=1)
            out.append((dX.download().reshape(n, 2), iters, res))
            del dX, keep
        (full, it_f, res_f), (short, it_s, res_s) = out
        assert it_f[0] == 1 and res_f[0] <= 1e-13 and 20 < it_f[1] < 1000 and res_f[1] <= 1e-8, (it_f, res_f)
        assert it_s[0] == 1 and it_s[1] == 1 and res_s[0] == res_f[0]
        assert full[:, 0].tobytes() == short[:, 0].tobytes(), "the frozen column moved after the look that froze it"
        assert full[:, 1].tobytes() != short[:, 1].tobytes()
    RUNS["freeze"] += 1


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_handle_stays_as_it_was(ctx, orc, pkg):
    capi = pkg.capi
    n, ent, B, X0, ks, (rp, cc, cv) = _problem("lap33", 3)
    k = 3
    A = ctx.csr(n, n, rp, cc, cv)
    dB, dX = ctx.vector_from(B.ravel()), ctx.vector_from(X0.ravel())
    plan, dev_bytes = A.get_plan(), A.info.device_bytes
    iters, res = ctx.cg_multi(A, dB, dX, k, max_iter=200, rel_tol=1e-9)
    assert np.all(iters > 0) and np.all(res <= 1e-9)
    assert A.get_plan() == plan and A.info.device_bytes == dev_bytes, "a solve changed the handle's plan or its device memory"

    def expect(code, fn, word="spmv_cg_multi"):
        with pytest.raises(capi.SpmvError) as e:
            fn()
        assert e.value.code == code and word in str(e.value), e.value

    expect(UNSUPPORTED, lambda: ctx.cg_multi(A, dB, dX, k, precond=capi.PRECOND_SYMGS))
    E = ctx.csr_to_ell(A)
    expect(UNSUPPORTED, lambda: ctx.cg_multi(E, dB, dX, k, jacobi=True))
    row, col, val = ent
    coo = ctx.coo(n, n, ol.i32(row), ol.i32(col), ol.f64(val))
    expect(UNSUPPORTED, lambda: ctx.cg_multi(coo, dB, dX, k))
    for bad_k in (0, 65):
        expect(INVALID, lambda: ctx.cg_multi(A, ctx.vector(n * bad_k), ctx.vector(n * bad_k), bad_k))
    expect(INVALID, lambda: ctx.cg_multi(A, ctx.vector(n * k - 1), dX, k))
    expect(INVALID, lambda: ctx.cg_multi(A, dB, ctx.vector(n * k + 1), k))
    expect(INVALID, lambda: ctx.cg_multi(A, dX, dX, k))
    big = ctx.vector(3 * n * k)
    expect(INVALID, lambda: ctx.cg_multi(A, ctx.wrap_vector(big.device_ptr, n * k), ctx.wrap_vector(big.device_ptr + 8 * 5, n * k), k))
    expect(INVALID, lambda: ctx.cg_multi(A, dB, dX, k, max_iter=-1))
    expect(INVALID, lambda: ctx.cg_multi(A, dB, dX, k, rel_tol=-1e-8))
    expect(INVALID, lambda: ctx.cg_multi(A, dB, dX, k, precond=7))
    wide = ctx.csr(n, n + 1, rp, cc, cv)
    expect(INVALID, lambda: ctx.cg_multi(wide, dB, dX, k))
    # a PANEL handle that released its CSR arrays (panel_keep_csr = 0): nothing left for the product to read, refused on the host
    nb = 1_000_000
    P = ctx.gen_csr_uniform(0, nb, nb, 16, seed=31)
    P.set_kernel(capi.CSR_PANEL)
    P.set_param("panel_keep_csr", 0)
    assert P.get_param("panel_keep_csr") == 0
    expect(INVALID, lambda: ctx.cg_multi(P, ctx.vector(nb * 2), ctx.vector(nb * 2), 2), "gave up")
    # -I with Jacobi: r . D^-1 r < 0 in the live column; the column with b = 0 is no breakdown
    m = 7
    negI = ctx.csr(m, m, np.arange(m + 1), np.arange(m), -np.ones(m))
    Bn = np.zeros((m, 2))
    Bn[:, 1] = 1.0
    expect(INVALID, lambda: ctx.cg_multi(negI, ctx.vector_from(Bn.ravel()), ctx.vector_from(np.zeros(2 * m)), 2, jacobi=True), "column 1")
    expect(INVALID, lambda: ctx.cg_multi(negI, ctx.vector_from(Bn.ravel()), ctx.vector_from(np.zeros(2 * m)), 2), "column 1")  # p.Ap < 0
    # a NaN in one column of B
    Bnan = B.copy()
    Bnan[5, 2] = np.nan
    expect(INVALID, lambda: ctx.cg_multi(A, ctx.vector_from(Bnan.ravel()), ctx.vector_from(X0.ravel()), k), "column 2")
    # and the handle still solves
    dX2 = ctx.vector_from(X0.ravel())
    iters2, res2 = ctx.cg_multi(A, dB, dX2, k, max_iter=200, rel_tol=1e-9)
    assert np.array_equal(iters2, iters) and dX2.download().tobytes() == dX.download().tobytes()
    assert A.get_plan() == plan and A.info.device_bytes == dev_bytes
    RUNS["refusals"] += 1


# ---- 6b. spmv_cg after the multi-column solves -----------------------------------------------------------------------------------------
def test_spmv_cg_is_untouched_by_the_multi_column_solves(ctx, pkg):
    """bits are not asserted: spmv_cg adds its dot products up in arrival order"""
    if not _CG_BEFORE or not RUNS["steps"]:
        pytest.skip("needs test_spmv_cg_before_any_multi_column_solve and the multi-column solves of this module before it")
    after = _cg_scalar_run(ctx)
    assert after["iters"] == _CG_BEFORE["iters"], (after["iters"], _CG_BEFORE["iters"])
    assert after["res"] <= 1e-10
    RUNS["cg"] += 1


# ---- 7. coverage -----------------------------------------------------------------------------------------------------------------------
def test_every_combination_ran():
    """every (k, alignment, preconditioner, format) of the cases above ran, and no ratio lies above the gate"""
    expect = {"steps": len(CASES), "bits": 1, "special": 3, "freeze": 1, "refusals": 1, "cg": 1}
    if any(RUNS[f] != c for f, c in expect.items()):
        pytest.skip(f"the coverage check needs every test of this module (ran {dict(RUNS)}, expected {expect})")
    need = {(k, a, "jacobi" if jac else "plain", fmt) for _, k, jac, fmt in CASES for a in ("aligned", "offset")}
    assert need <= SEEN, f"never ran: {sorted(need - SEEN)}"
    lines = ["# spmv_cg_multi column by column (tests/test_gpu_cg_multi.py): the largest deviation of a column's x_j, and of its",
             "# rel_resid, from that column's np.longdouble recurrence, in units of the float64 twins' own largest deviation at that j",
             "# (the gate is 8).  k | X alignment | preconditioner | format | x ratio | residual ratio | where the x ratio was largest"]
    for (k, a, p, fmt), r in sorted(RATIO.items()):
        lines.append(f"k={k:<3d} {a:8s} {p:7s} {fmt:4s}  x {r['x'][0]:6.3f}  residual {r['residual'][0]:6.3f}  ({r['x'][1]})")
        assert r["x"][0] <= sr.F and r["residual"][0] <= sr.F
    print("\n".join(lines))
    out = os.environ.get("SPMV_SOLVER_MULTI_RATIOS")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
