"""The NumPy reference of ILU(0) (tests/ilu0_ref.py) held to facts that need no engine - no GPU.

What pins a reference that the engine is then compared with number by number: the defining property of ILU(0), (L U)_ij = a_ij on
the pattern, in both sweep orders; exactness where no fill arises; two mutations that must break the first property; and the
iteration counts of the float64 solver twins that tests/test_gpu_ilu0.py compares the engine's with."""
import numpy as np
import pytest

import ilu0_ref as ir

EPS = float(np.finfo(np.float64).eps)
# (L U)_ij - a_ij on the pattern is what rounding leaves: a_ij takes at most d - 1 fused subtractions (d entries in the row), each
# rounded once on the scale of the running value, which stays below max |A| for these diagonally dominant matrices, and the check
# re-forms the sum with d roundings of its own: (2 d) * eps / 2 * max |A| at worst, d <= 9 here.  MEASURED (printed below): 1.3
# eps * max |A| on the Laplacian in both orders (values up to 6), 0.1 on the random matrix (values up to 6.7).
PATTERN_GATE = 9.0
# Without fill L U = A up to the roundings above and the two substitutions are backward stable, so A z - r is a few roundings of
# terms no larger than |r| scaled by the row sums of |L| |U| |A^-1| - below 4 for these dominant rows with d <= 7 entries:
# (d + 2) * 4 * eps / 2 at worst.  MEASURED: 3.3e-16 = 1.5 eps on the tridiagonal matrix, 1.0 eps on the triangular one.
EXACT_GATE = 18.0


def _matrices():
    yield "laplacian_3d_6", ir.laplacian_3d(6)
    yield "dominant_random_200", ir.dominant_random(200, 5, 11)


def _orders(n, rp, cc):
    return {"row_order": np.arange(n), "multicolour": ir.greedy_colour_order(n, rp, cc)[2]}


@pytest.mark.parametrize("order", ["row_order", "multicolour"])
def test_the_factors_multiply_back_to_the_matrix_on_its_pattern(order):
    for name, (n, rp, cc, cv) in _matrices():
        a = ir.merged_entries(n, rp, cc, cv)
        f = ir.Ilu0(n, rp, cc, cv, _orders(n, rp, cc)[order])
        err = np.max(np.abs(f.product_on_pattern() - a)) / (EPS * np.max(np.abs(a)))
        print(f"{name} {order}: max |(LU - A) on P| = {err:.2f} eps max|A|")
        assert err <= PATTERN_GATE, (name, order, err)
        # of a set of duplicates the first stored one carries the value, the others hold 0.0
        rows = np.repeat(np.arange(n), np.diff(rp))
        code = rows.astype(np.int64) * n + cc
        firsts = np.zeros(len(cc), bool)
        firsts[np.unique(code, return_index=True)[1]] = True
        assert np.all(f.values[~firsts] == 0.0) and np.all(f.values[firsts & (rows == cc)] != 0.0)


def test_mutations_break_the_pattern_property():
    """a reference without the pattern restriction, and one that ignores pos under the multicolour order (the elimination of the
    row order passed off as the multicolour one), are both far outside the gate"""
    for name, (n, rp, cc, cv) in _matrices():
        a = ir.merged_entries(n, rp, cc, cv)
        scale = EPS * np.max(np.abs(a))
        mc = _orders(n, rp, cc)["multicolour"]
        for order in _orders(n, rp, cc).values():
            g = ir.Ilu0(n, rp, cc, cv, order, restrict=False)
            assert np.max(np.abs(g.product_on_pattern() - a)) / scale > 1e6 * PATTERN_GATE, name
        g = ir.Ilu0(n, rp, cc, cv, np.arange(n))
        g.pos = ir.Ilu0(n, rp, cc, cv, mc).pos
        assert np.max(np.abs(g.product_on_pattern() - a)) / scale > 1e6 * PATTERN_GATE, name


@pytest.mark.parametrize("problem", ["tridiagonal_nonsym_33", "lower_triangular_200"])
def test_without_fill_the_application_is_the_exact_solve(problem):
    n, rp, cc, cv = ir.tridiagonal_nonsym(33) if problem.startswith("tri") else ir.lower_triangular_cut(200, 5, 6)
    f = ir.Ilu0(n, rp, cc, cv, np.arange(n))
    r = np.random.default_rng(17).uniform(-1, 1, n)
    z = f.apply(r)
    resid = np.max(np.abs(ir.csr_mv(n, rp, cc, cv, z) - r)) / np.max(np.abs(r))
    print(f"{problem}: |A z - r|_inf / |r|_inf = {resid:.3e} = {resid / EPS:.2f} eps")
    assert resid <= EXACT_GATE * EPS, (problem, resid)
    mv = lambda x: ir.csr_mv(n, rp, cc, cv, x)
    for order in ir.DOT_ORDERS:
        for run in (ir.run_cg, ir.run_bicgstab):
            x, iters = run(mv, f.apply, r, 1e-9, 50, dot_order=order)
            assert iters == 1, (problem, run.__name__, order, iters)
            assert np.max(np.abs(mv(x) - r)) <= 1e-9 * np.max(np.abs(r))


@pytest.mark.parametrize("system", ir.SOLVER_SYSTEMS)
def test_iteration_counts_of_the_twins(system):
    """the table of the feature's motivation, measured: none / Jacobi / ILU(0) in both orders, every dot order"""
    solver, n, rp, cc, cv, b = ir.solver_system(system)
    for precond in ("none", "jacobi"):
        counts = ir.twin_iterations(system, None, precond)
        print(f"{system} {precond}: {counts}")
        assert set(counts.values()) == {ir.UNPRECONDITIONED_ITERATIONS[system]}, (precond, counts)
    for mode, order in enumerate(_orders(n, rp, cc).values()):
        counts = ir.twin_iterations(system, order)
        print(f"{system} ilu0 order {mode}: {counts}")
        assert (min(counts.values()), max(counts.values())) == ir.TWIN_ITERATIONS[system, mode], (mode, counts)
        assert max(counts.values()) * 1.5 < ir.UNPRECONDITIONED_ITERATIONS[system]
