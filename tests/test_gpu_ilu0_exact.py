"""ILU(0) and the level solves held to EQUALITY on matrices they factorise exactly, the mixed launch schedule against the float64
twin, and the degenerate sizes (spmv_ilu0_*; csrc/ilu0.hip, csrc/tri_levels.hpp).

The exact family (tests/ilu0_ref.py: clique_blocks, band_lu; tests/test_ilu0_ref.py checks all of this on the CPU first): A = (I + L) U
from small dyadic numbers on a pattern that takes no fill - dense blocks with their rows interleaved, exact in both sweep orders, and
bands, exact in row order.  ILU(0) must return L and U themselves and map r = A z, z integers, to z: every term of every sum is on one
dyadic grid far inside the 2^53 budget (assert_exact_budget), so no lane tree, summation order or fma moves a bit.  A dropped term, a
row read before it was finished, a wrong merge of duplicates shows as a wrong dyadic number.  Every position of the pattern is stored,
zeros included, a fifth of the entries twice (both triangles and the diagonal), the entries of a row in random order.

  cliques_130    blocks of 1, 2, 27, 65, 130 rows: 130 colours (three windows of the colouring's 64-colour loop), 130 levels of up to
                 5 rows, 48 entries per triangle row: the 16-lane solve
  cliques_mixed  1500 blocks of 1 .. 6 rows and two of 130 and 70: 4 lanes; levels 0 and 1 are above 4096 lanes and launches of their
                 own, the 128 behind them one folded run from first_level = 2 - in the solves and in the factorisation
  cliques_12     60 blocks of 12, 5 of 1: 4 lanes, every level folded
  cliques_tiny   6000 blocks of 1 .. 3 rows: 1 lane, a level of 6000 rows: tri_solve_level_kernel<1> and ilu0_factor_level_kernel
  band_1_20 / band_20_1   5000 rows: 1 lane in one triangle, 16 in the other; 5000 one-row levels in one run
  band_3_3       3000 rows: 4 lanes, a chain

The float64 twin of a case is computed once and shared.  test_every_case_ran asserts at the end that every case ran."""
from collections import defaultdict

import numpy as np
import pytest

import ilu0_ref as ir
import oracle_lib as ol

pytestmark = pytest.mark.gpu

RUNS = defaultdict(int)
_CASE, _LAPLACIAN = {}, {}
_IDS = [f"{name}-{'multicolour' if order else 'row_order'}" for name, order in ir.EXACT_CASES]


def _case(name):
    if name not in _CASE:
        _CASE[name] = ir.exact_case(name)
    return _CASE[name]


def _same(got, want, what):
    """equality by value (-0.0 == 0.0), the differences counted and the first ones shown"""
    bad = np.flatnonzero(~(np.asarray(got) == np.asarray(want)))
    print(f"{what}: {len(bad)} of {len(want)} differ")
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), np.asarray(got)[bad[:5]].tolist(), np.asarray(want)[bad[:5]].tolist())


def _close(got, want, what):
    err = np.max(np.abs(got - want)) / max(np.max(np.abs(want)), 1e-300)
    print(f"{what}: {err:.3e}")
    assert err <= ol.REL_TOL, (what, err)


def _firsts(n, rp, cc):
    rows = np.repeat(np.arange(n), np.diff(rp))
    firsts = np.zeros(len(cc), bool)
    firsts[np.unique(rows.astype(np.int64) * max(n, 1) + cc, return_index=True)[1]] = True
    return firsts


def _apply(ctx, A, r_host):
    n = len(r_host)
    r, z = ctx.vector_from(r_host), ctx.vector(n)
    z.fill(7.0)  # (whatever z holds is ignored)
    ctx.ilu0_solve(A, r, z)
    ctx.sync()
    return z.download()


def _structure(A):
    return A.get_param("ilu0_levels_forward"), A.get_param("ilu0_levels_backward"), A.get_param("ilu0_launches")


# ---- 1. the exact cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,order", ir.EXACT_CASES, ids=_IDS)
def test_exact_factors_application_and_schedule(ctx, orc, pkg, name, order):
    n, rp, cc, cv, expected, z_host = _case(name)
    A = ctx.csr(n, n, rp, cc, cv)
    A.set_param("ilu0_order", order)
    # the order
    seq = ctx.ilu0_order(A)
    if order == 0:
        assert np.array_equal(seq, np.arange(n)) and A.get_param("ilu0_colours") == 0
    else:
        sizes, seed = ir.EXACT_CLIQUES[name]
        ncol, colour, want_seq = ol.greedy_colour_order(orc, rp, cc)
        rank = ir.clique_rank(sizes, seed)[1]
        assert np.array_equal(seq, want_seq) and np.array_equal(seq, np.argsort(rank, kind="stable"))  # colour = rank in the block
        assert A.get_param("ilu0_colours") == ncol == max(sizes)
    # the factors: L and U themselves; later duplicates hold 0.0
    fac = ctx.ilu0_factors(A)
    _same(fac, expected, f"{name} order {order}: factors")
    later = ~_firsts(n, rp, cc)
    assert later.sum() > 0.1 * len(cc) and np.all(fac[later] == 0.0)
    # the application: r = A z gives z back
    r_host = ir.csr_mv(n, rp, cc, cv, z_host)
    got = _apply(ctx, A, r_host)
    _same(got, z_host, f"{name} order {order}: application")
    assert _apply(ctx, A, r_host).tobytes() == got.tobytes(), "two applications differ"
    # levels and launches: what the schedule rule makes of this pattern
    want = ir.level_sizes(n, rp, cc, seq)
    assert _structure(A) == (len(want["lower"]), len(want["upper"]), want["launches"]), (_structure(A), want["schedule"])
    # M^-1 A = I: one iteration (b = A z, so that the first half step lands on z itself: L^-1 and U^-1 of a random product are
    # far too large for a b that is not a product of small numbers)
    b, x = ctx.vector_from(r_host), ctx.vector(n)
    x.fill(0.0)
    iters, res = ctx.bicgstab(A, b, x, max_iter=50, rel_tol=1e-9, precond=pkg.capi.PRECOND_ILU0)
    true = np.linalg.norm(r_host - ir.csr_mv(n, rp, cc, cv, x.download())) / np.linalg.norm(r_host)
    print(f"{name} order {order}: bicgstab {iters} iteration(s), reported {res:.3e}, true {true:.3e}")
    assert iters == 1 and res <= 1e-9 and true <= 1e-9, (iters, res, true)
    RUNS["exact"] += 1


# ---- 2. a schedule that alternates folded runs and levels of their own, against the float64 twin -------------------------------------
def _laplacian40():
    if not _LAPLACIAN:
        n, rp, cc, cv = ir.laplacian_3d(40)
        seq = np.arange(n)
        _LAPLACIAN.update(csr=(n, rp, cc, cv), ref=ir.Ilu0(n, rp, cc, cv, seq), levels=ir.level_sizes(n, rp, cc, seq))
    return _LAPLACIAN["csr"], _LAPLACIAN["ref"], _LAPLACIAN["levels"]


def test_a_mixed_schedule_matches_the_reference(ctx, pkg):
    """the 40^3 Laplacian in row order: 64,000 rows in 118 levels, the middle ones above 4096 lanes (up to 1200 rows of 4 lanes):
    a folded run, launches level by level, a folded run - in both solves and in the factorisation"""
    (n, rp, cc, cv), ref, want = _laplacian40()
    A = ctx.csr(n, n, rp, cc, cv)
    A.set_param("ilu0_order", 0)
    ctx.ilu0_setup(A)
    assert _structure(A) == (118, 118, want["launches"]) and want["launches"] > 2 and want["lanes"] == (4, 4), (_structure(A), want["schedule"])
    for sched in want["schedule"]:
        assert sched[0][1] > 1 and sched[-1][1] > 1 and all(k == 1 for _, k in sched[1:-1]) and len(sched) > 2, sched
    _close(ctx.ilu0_factors(A), ref.values, "laplacian_3d(40) row order: factors")
    r_host = np.random.default_rng(41).uniform(-1, 1, n)
    _close(_apply(ctx, A, r_host), ref.apply(r_host), "laplacian_3d(40) row order: application")
    RUNS["mixed"] += 1


# ---- 3. degenerate sizes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1], ids=["row_order", "multicolour"])
def test_degenerate_sizes(ctx, orc, pkg, order):
    # no rows: set-up, application, factors and order succeed and do nothing
    E = ctx.csr(0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    E.set_param("ilu0_order", order)
    ctx.ilu0_setup(E)
    ctx.ilu0_solve(E, ctx.vector(0), ctx.vector(0))
    ctx.sync()
    assert len(ctx.ilu0_factors(E)) == 0 and len(ctx.ilu0_order(E)) == 0 and E.get_param("ilu0_launches") == 0
    # one row, its diagonal entry stored twice
    O = ctx.csr(1, 1, np.array([0, 2], np.int32), np.zeros(2, np.int32), np.array([0.75, -0.25]))
    O.set_param("ilu0_order", order)
    assert np.array_equal(ctx.ilu0_factors(O), [0.5, 0.0]) and np.array_equal(ctx.ilu0_order(O), [0])
    assert np.array_equal(_apply(ctx, O, np.array([3.0])), [6.0])
    assert _structure(O) == (1, 1, 2) and O.get_param("ilu0_colours") == order
    # a diagonal matrix: both triangles empty; z = r / d bit for bit
    n = 5000
    rng = np.random.default_rng(43)
    d = rng.uniform(0.5, 2.0, n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    D = ctx.csr(n, n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), d)
    D.set_param("ilu0_order", order)
    r_host = rng.uniform(-1, 1, n)
    assert _apply(ctx, D, r_host).tobytes() == (r_host / d).tobytes()
    assert ctx.ilu0_factors(D).tobytes() == d.tobytes() and np.array_equal(ctx.ilu0_order(D), np.arange(n))
    assert _structure(D) == (1, 1, 2) and D.get_param("ilu0_colours") == order  # (one colour in the multicolour order)
    RUNS["degenerate"] += 1


@pytest.mark.parametrize("order", [0, 1], ids=["row_order", "multicolour"])
@pytest.mark.parametrize("cut", ["upper", "lower"])
def test_triangular_cuts_of_an_exact_case(ctx, orc, pkg, cut, order):
    """the entries of cliques_12 on and above (below) the diagonal in ROW order, the diagonal entries replaced by the powers of two of
    U's diagonal (a split one keeps its two parts: u_ii - 1/4 and 1/4).  A triangular matrix is its own factor - U = A and L empty, or
    L = A D^-1 and U = D - and takes no fill; every division is by a power of two and r = A z has the budget of the full case.  The
    multicolour order of the upper cut is the row order (no row names an earlier one: one colour); in that of the lower cut colour =
    rank in the block again, and what is below the diagonal stays before it in the sweep."""
    n, rp, cc, cv, expected, z_host = _case("cliques_12")
    rows = np.repeat(np.arange(n), np.diff(rp))
    keep = cc >= rows if cut == "upper" else cc <= rows
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int32)
    cc2, cv2, rows2 = cc[keep], cv[keep].copy(), rows[keep]
    on_diag, first = cc2 == rows2, _firsts(n, rp2, cc2)
    split = np.bincount(rows2[on_diag], minlength=n) - 1  # later duplicates of a row's diagonal entry: 0 or 1
    assert set(split) == {0, 1}
    cv2[on_diag & first] = expected[keep][on_diag & first] - 0.25 * split[rows2[on_diag & first]]  # (row order: expected = u_ii)
    cv2[on_diag & ~first] = 0.25
    A = ctx.csr(n, n, rp2, cc2, cv2)
    A.set_param("ilu0_order", order)
    seq = ctx.ilu0_order(A)
    if order:
        ncol, colour, want_seq = ol.greedy_colour_order(orc, rp2, cc2)
        assert np.array_equal(seq, want_seq) and A.get_param("ilu0_colours") == ncol == (12 if cut == "lower" else 1)
    else:
        assert np.array_equal(seq, np.arange(n))
    # the expected factors: the sums of the stored duplicates, below the diagonal divided by the pivot of their column
    merged = ir.merged_entries(n, rp2, cc2, cv2)
    diag = np.zeros(n)
    diag[rows2[on_diag]] = merged[on_diag]
    assert np.all(np.abs(np.frexp(diag)[0]) == 0.5)  # +- powers of two
    want = np.where(first, np.where(cc2 < rows2, merged / diag[cc2], merged), 0.0)
    _same(ctx.ilu0_factors(A), want, f"{cut} cut, order {order}: factors")
    r_host = ir.csr_mv(n, rp2, cc2, cv2, z_host)
    _same(_apply(ctx, A, r_host), z_host, f"{cut} cut, order {order}: application")
    lv = ir.level_sizes(n, rp2, cc2, seq)
    assert _structure(A) == (len(lv["lower"]), len(lv["upper"]), lv["launches"])
    assert (len(lv["lower"]), len(lv["upper"])) == ((1, 12) if cut == "upper" else (12, 1))
    RUNS["cuts"] += 1


# ---- 4. coverage -------------------------------------------------------------------------------------------------------------------------
def test_every_case_ran():
    expect = {"exact": len(ir.EXACT_CASES), "mixed": 1, "degenerate": 2, "cuts": 4}
    if any(RUNS[k] != c for k, c in expect.items()):
        pytest.skip(f"the coverage check needs every test of this module (ran {dict(RUNS)}, expected {expect})")
    assert set(_CASE) == set(ir.EXACT_CLIQUES) | set(ir.EXACT_BANDS)
