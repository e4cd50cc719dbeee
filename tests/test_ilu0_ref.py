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


# ---- the exact family: A = (I + L) U from dyadic numbers on a pattern without fill (ilu0_ref.clique_blocks, band_lu) ----------------
# What tests/test_gpu_ilu0_exact.py asks of the engine, asked of the reference first - and the structure every case is there for.
# STRUCTURE[name, order] = (colours, levels of L, levels of U, lanes of (L, U), launches of one application)
STRUCTURE = {
    ("cliques_130", 0): (130, 130, 130, (16, 16), 2), ("cliques_130", 1): (130, 130, 130, (16, 16), 2),
    ("cliques_mixed", 0): (130, 130, 130, (4, 4), 6), ("cliques_mixed", 1): (130, 130, 130, (4, 4), 6),
    ("cliques_12", 0): (12, 12, 12, (4, 4), 2), ("cliques_12", 1): (12, 12, 12, (4, 4), 2),
    ("cliques_tiny", 0): (3, 3, 3, (1, 1), 4), ("cliques_tiny", 1): (3, 3, 3, (1, 1), 4),
    ("band_1_20", 0): (None, 5000, 5000, (1, 16), 2), ("band_20_1", 0): (None, 5000, 5000, (16, 1), 2),
    ("band_3_3", 0): (None, 3000, 3000, (4, 4), 2),
}
_EXACT = {}


def _exact(name):
    if name not in _EXACT:
        _EXACT[name] = ir.exact_case(name)
    return _EXACT[name]


def _sequence(name, order, n, rp, cc):
    return ir.greedy_colour_order(n, rp, cc)[2] if order else np.arange(n)


def test_the_exact_cases_are_those_of_the_gpu_test():
    assert set(STRUCTURE) == set(ir.EXACT_CASES)


@pytest.mark.parametrize("name,order", ir.EXACT_CASES, ids=[f"{n}-{'multicolour' if o else 'row_order'}" for n, o in ir.EXACT_CASES])
def test_the_reference_returns_the_factors_and_z_of_an_exact_case(name, order):
    n, rp, cc, cv, expected, z = _exact(name)
    seq = _sequence(name, order, n, rp, cc)
    f = ir.Ilu0(n, rp, cc, cv, seq)
    assert np.array_equal(f.values, expected), name  # (by value: -0.0 == 0.0)
    r = ir.csr_mv(n, rp, cc, cv, z)
    assert np.array_equal(f.apply(r), z), name
    bits = ir.assert_exact_budget(n, rp, cc, cv, expected, seq, z)
    print(f"{name} order {order}: the largest sum takes {bits:.1f} bits on the grid 2^-{ir.EXACT_G} (budget 53)")
    # of what the builder promises: duplicates in both triangles and on the diagonal, stored zeros, rows out of order
    rows = np.repeat(np.arange(n), np.diff(rp))
    code = rows.astype(np.int64) * n + cc
    firsts = np.zeros(len(cc), bool)
    firsts[np.unique(code, return_index=True)[1]] = True
    later = ~firsts
    assert 0.1 * len(cc) < later.sum() < 0.25 * len(cc)
    pos = np.empty(n, np.int64)
    pos[seq] = np.arange(n)
    for part in (pos[cc] < pos[rows], pos[cc] == pos[rows], pos[cc] > pos[rows]):
        assert (later & part).any() or not (part & (rows != cc)).any(), "a triangle without duplicates"
    assert (cv == 0.0).any() and np.any(np.diff(cc)[np.diff(rows) == 0] < 0)


@pytest.mark.parametrize("name,order", ir.EXACT_CASES, ids=[f"{n}-{'multicolour' if o else 'row_order'}" for n, o in ir.EXACT_CASES])
def test_colours_levels_and_launches_of_an_exact_case(name, order):
    n, rp, cc, cv, expected, z = _exact(name)
    colours, lf, lb, lanes, launches = STRUCTURE[name, order]
    if name in ir.EXACT_CLIQUES:
        sizes, seed = ir.EXACT_CLIQUES[name]
        owner, rank = ir.clique_rank(sizes, seed)
        assert n == sum(sizes) and np.array_equal(np.bincount(owner), sizes)
        ncol, colour, seq = ir.greedy_colour_order(n, rp, cc)
        assert ncol == colours == max(sizes) and np.array_equal(colour, rank) and np.array_equal(seq, np.argsort(rank, kind="stable"))
    seq = _sequence(name, order, n, rp, cc)
    lv = ir.level_sizes(n, rp, cc, seq)
    print(f"{name} order {order}: n = {n}, lanes {lv['lanes']}, schedule {lv['schedule']}, largest levels {lv['lower'].max()} / {lv['upper'].max()}")
    assert (len(lv["lower"]), len(lv["upper"]), lv["lanes"], lv["launches"]) == (lf, lb, lanes, launches)
    assert lv["lower"].sum() == n and lv["upper"].sum() == n
    if name in ir.EXACT_CLIQUES:  # level t of L: the rows of rank t; of U: the rows t before their block's last
        assert np.array_equal(lv["lower"], np.bincount(rank))
        assert np.array_equal(lv["upper"], np.bincount(np.asarray(sizes)[owner] - 1 - rank))
    else:
        assert set(lv["lower"]) == set(lv["upper"]) == {1}
    if name == "cliques_130":
        assert lv["lower"].max() == 5 and np.count_nonzero(expected) / n > 2 * 12  # three windows of 64 colours; the 16-lane solve
    if name == "cliques_mixed":  # a level of its own launch in front, then a folded run that starts behind it
        for sched, hist in zip(lv["schedule"], (lv["lower"], lv["upper"])):
            assert sched[0] == (0, 1) and hist[0] > 1500 and sched[-1][0] >= 1 and sched[-1][1] > 1
    if name == "cliques_tiny":  # one lane per row and a level above 4096 rows: the 1-lane level kernel, and the factorisation's
        assert lv["lower"][0] > ir.SMALL_LEVEL and lv["upper"][0] > ir.SMALL_LEVEL
    if name == "cliques_12":
        assert lv["schedule"] == [[(0, 12)], [(0, 12)]]


def test_level_sizes_on_the_laplacian_and_the_degenerate_shapes():
    m = 40  # the mixed schedule of tests/test_gpu_ilu0_exact.py: run, levels of their own, run
    n, rp, cc, cv = ir.laplacian_3d(m)
    lv = ir.level_sizes(n, rp, cc, np.arange(n))
    assert len(lv["lower"]) == len(lv["upper"]) == 3 * m - 2 and lv["lanes"] == (4, 4) and lv["lower"].max() == 1200
    big = np.flatnonzero(lv["lower"] * 4 > ir.SMALL_LEVEL)
    assert len(big) and lv["launches"] == 2 * (len(big) + 2) and lv["schedule"][0][0] == (0, int(big[0]))
    n, rp, cc, cv = ir.laplacian_3d(24)
    assert ir.level_sizes(n, rp, cc, np.arange(n))["launches"] == 2  # (one folded run per triangle: what the 24^3 case never leaves)
    assert ir.level_sizes(n, rp, cc, ir.greedy_colour_order(n, rp, cc)[2])["launches"] == 4
    lv = ir.level_sizes(0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int64))
    assert lv["launches"] == 0 and len(lv["lower"]) == 0
    lv = ir.level_sizes(5000, np.arange(5001), np.arange(5000), np.arange(5000))
    assert lv["launches"] == 2 and lv["lanes"] == (1, 1) and list(lv["lower"]) == [5000]
    # duplicates: counted once for ILU(0), as stored for the Gauss-Seidel sweep
    n, rp, cc, cv = ir.dominant_random(200, 4, 5)
    rp2, cc2 = 2 * np.asarray(rp), np.repeat(cc.reshape(n, -1), 2, axis=1).ravel()
    assert ir.level_sizes(n, rp2, cc2, np.arange(n))["lanes"] == ir.level_sizes(n, rp, cc, np.arange(n))["lanes"] == (1, 1)
    assert ir.level_sizes(n, rp2, cc2, np.arange(n), merged=False)["lanes"] == (4, 4)


def test_the_budget_check_refuses_what_is_not_exact():
    n, rp, cc, cv, expected, z = ir.exact_case("cliques_12")
    seq = np.arange(n)
    ir.assert_exact_budget(n, rp, cc, cv, expected, seq, z)
    off = np.flatnonzero(cv != 0.0)[0]
    for what, change in (("grid", 2.0**-7), ("product", 0.25)):
        v = cv.copy()
        v[off] += change
        with pytest.raises(AssertionError):
            ir.assert_exact_budget(n, rp, cc, v, expected, seq, z)
    with pytest.raises(AssertionError, match="bits"):
        ir.assert_exact_budget(n, rp, cc, cv, expected, seq, z * 2.0**47)
    keep = np.ones(len(cc), bool)  # a position taken out of a block: fill
    rows = np.repeat(np.arange(n), np.diff(rp))
    owner, rank = ir.clique_rank(*ir.EXACT_CLIQUES["cliques_12"])
    i, j = (np.flatnonzero((owner == 0) & (rank == r))[0] for r in (5, 9))
    keep[(rows == i) & (cc == j)] = False
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))])
    with pytest.raises(AssertionError, match="fill"):
        ir.assert_exact_budget(n, rp2, cc[keep], cv[keep], expected[keep], seq, z)
    with pytest.raises(AssertionError):  # the band is exact in row order only
        nb, rpb, ccb, cvb, eb, zb = ir.exact_case("band_3_3")
        ir.assert_exact_budget(nb, rpb, ccb, cvb, eb, ir.greedy_colour_order(nb, rpb, ccb)[2], zb)
