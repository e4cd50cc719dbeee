"""The NumPy twin of the triangular solves (tests/trsv_ref.py) checked on the CPU: the extraction rules, the float64 twins against
np.longdouble substitution, the exactness budget of every exact case tests/test_gpu_trsv.py runs (and its refusal of an input over
the budget), and the level tables against ilu0_ref.level_sizes."""
import numpy as np
import pytest

import ilu0_ref as ir
import trsv_ref as tr

L, U, UNIT, T = tr.TRSV_LOWER, tr.TRSV_UPPER, tr.TRSV_UNIT, tr.TRSV_TRANSPOSE
EXACT_NAMES = list(ir.EXACT_CLIQUES) + list(ir.EXACT_BANDS)
TRANSPOSED_NAMES = ("band_3_3", "band_1_20", "cliques_12")
_CASE = {}


def _case(name):
    if name not in _CASE:
        _CASE[name] = ir.exact_case(name)
    return _CASE[name]


# ---- extraction ------------------------------------------------------------------------------------------------------------------------
def test_extraction_rules():
    # row 0: diagonal 2 + 3, upper entries (0,2) twice in stored order; row 1: lower (1,0), no diagonal; row 2: lower 1 then 0 (unsorted),
    # a stored zero, diagonal -4; row 3: diagonal 0.5, upper none, lower (3,1)
    rp = np.array([0, 4, 5, 9, 11])
    cc = np.array([2, 0, 2, 0, 0, 1, 2, 0, 1, 3, 1])
    cv = np.array([7.0, 2.0, 9.0, 3.0, 11.0, 5.0, -4.0, 6.0, 0.0, 0.5, 8.0])
    ptr, col, val, diag, has, lower = tr.extract(4, rp, cc, cv, L)
    assert lower and ptr.tolist() == [0, 0, 1, 4, 5] and col.tolist() == [0, 1, 0, 1, 1] and val.tolist() == [11.0, 5.0, 6.0, 0.0, 8.0]
    assert diag.tolist() == [5.0, 0.0, -4.0, 0.5] and has.tolist() == [True, False, True, True]
    assert tr.bad_diagonal_row(diag, has) == 1
    ptr, col, val, diag, has, lower = tr.extract(4, rp, cc, cv, U)  # the lower entries are ignored, the duplicate kept as two terms
    assert not lower and ptr.tolist() == [0, 2, 2, 2, 2] and col.tolist() == [2, 2] and val.tolist() == [7.0, 9.0]
    # transposed lower: entries (2,1)=5, (2,1)=0 and (3,1)=8 become row 1: columns 2, 2, 3 ascending, duplicates in stored order
    ptr, col, val, diag, has, lower = tr.extract(4, rp, cc, cv, L | T)
    assert not lower and ptr.tolist() == [0, 2, 5, 5, 5] and col.tolist() == [1, 2, 2, 2, 3] and val.tolist() == [11.0, 6.0, 5.0, 0.0, 8.0]
    ptr, col, val, diag, has, lower = tr.extract(4, rp, cc, cv, U | T | UNIT)
    assert lower and ptr.tolist() == [0, 0, 0, 2, 2] and col.tolist() == [0, 0] and val.tolist() == [7.0, 9.0]
    # the transposed copy is the transpose: (T^T) x by the copy = the columns' sums by the original
    n, rp, cc, cv = tr.random_system(65, 6, 3)
    x = np.random.default_rng(1).integers(-4, 5, n).astype(np.float64)
    for uplo in (L, U):
        p0, c0, v0, d0, _, _ = tr.extract(n, rp, cc, cv, uplo)
        p1, c1, v1, d1, _, _ = tr.extract(n, rp, cc, cv, uplo | T)
        dense0, dense1 = np.zeros((n, n)), np.zeros((n, n))
        np.add.at(dense0, (np.repeat(np.arange(n), np.diff(p0)), c0), v0)
        np.add.at(dense1, (np.repeat(np.arange(n), np.diff(p1)), c1), v1)
        assert np.array_equal(dense0.T, dense1) and np.array_equal(d0, d1)
        assert all(np.all(np.diff(c1[p1[i]:p1[i + 1]]) >= 0) for i in range(n)), "a transposed row is not in ascending column index"


# ---- the twins against np.longdouble -----------------------------------------------------------------------------------------------
def _systems():
    yield "laplacian_3d(12)", ir.laplacian_3d(12), 3
    for n in (1, 2, 63, 64, 65, 257):
        for per_row in (1, 6, 40):
            yield f"random n={n} per_row={per_row}", tr.random_system(n, per_row, 1000 * n + per_row), per_row
    for name in ("cliques_12", "band_3_3"):
        n, rp, cc, cv, expected, z = _case(name)
        yield name, (n, rp, cc, expected), None


def test_twins_agree_with_longdouble_substitution():
    """Row-wise dominance (|d_i| >= 1 + sum |t_ij|, or a unit diagonal over sums of at most 1/2) bounds cond(T) by a small constant,
    and substitution with m terms per row has the componentwise backward error (m + 1) u: the bound asserted is 8 (m + 2) u.  (The
    Laplacian's triangles under UNIT are I - N with N >= 0, not dominant: x grows to 1e13, but no sum cancels beyond what b brings, and the
    norm-wise error stays at the same level.)  The exact cases' factors are not dominant; there the right-hand side is built from
    integers and the twins must return them exactly."""
    rng = np.random.default_rng(17)
    for what, (n, rp, cc, cv), per_row in _systems():
        for flags in tr.ALL_FLAGS:
            ptr, col, val, diag, has, lower = tr.extract(n, rp, cc, cv, flags)
            unit = bool(flags & UNIT)
            if per_row is None:
                x = ir.integer_vector(n, 5)
                _, b = tr.assert_trsv_budget(n, ptr, col, val, diag, x, unit)
                for lanes in (1, 4, 16):
                    assert np.array_equal(tr.solve_twin(n, ptr, col, val, diag, lower, b, unit, lanes), x), (what, flags, lanes)
                assert np.array_equal(tr.solve_longdouble(n, ptr, col, val, diag, lower, b, unit).astype(np.float64), x)
                continue
            b = rng.uniform(-1, 1, n)
            ref = tr.solve_longdouble(n, ptr, col, val, diag, lower, b, unit)
            m = int(np.max(np.diff(ptr))) if n else 0
            for lanes in (1, 4, 16):
                err = tr.rel_error(tr.solve_twin(n, ptr, col, val, diag, lower, b, unit, lanes), ref)
                assert err <= 8 * (m + 2) * tr.UNIT_ROUNDOFF, (what, tr.flag_name(flags), lanes, err)


def test_the_tree_is_group_sums():
    """lanes 0..L-1 hold the strided partial sums; the tree adds neighbours first: ((p0 + p1) + (p2 + p3)) + ..."""
    big = 2.0**53
    assert tr._tree([big, 1.0, 1.0, -big]) == (big + 1.0) + (1.0 - big)  # 0.0 + ..., not the serial 1.0
    assert tr._tree([1.0]) == 1.0 and tr._tree([0.0] * 16) == 0.0
    # a row of 8 entries on 4 lanes: lane l adds entries l and l + 4
    ptr, col, val = np.array([0, 0, 8]), np.zeros(8, np.int64), np.array([big, 1.0, 1.0, -big, 0.0, 0.0, 0.0, 0.0])
    x4 = tr.solve_twin(2, ptr, col, val, np.ones(2), True, np.array([1.0, 0.0]), True, lanes=4)
    x1 = tr.solve_twin(2, ptr, col, val, np.ones(2), True, np.array([1.0, 0.0]), True, lanes=1)
    assert x4[1] == -((big + 1.0) + (1.0 - big)) and x1[1] == -(((big + 1.0) + 1.0) - big)


# ---- the exactness budget --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EXACT_NAMES)
def test_budget_of_the_exact_cases(name):
    """what tests/test_gpu_trsv.py solves exactly: L y = r with y = U z (multiples of 1/2), U z = y, for one and for 64 columns; and
    the transposed solves of the three cases it transposes"""
    n, rp, cc, cv, expected, z = _case(name)
    seed = (ir.EXACT_CLIQUES.get(name) or ir.EXACT_BANDS[name])[-1]
    Z = np.stack([ir.integer_vector(n, seed + c) for c in range(64)], axis=1)
    assert np.array_equal(Z[:, 0], z)
    lo, up = tr.extract(n, rp, cc, expected, L | UNIT), tr.extract(n, rp, cc, expected, U)
    bits_u, Y = tr.assert_trsv_budget(n, *up[:4], Z, unit=False)
    bits_l, R = tr.assert_trsv_budget(n, *lo[:4], Y, unit=True, gx=1)
    # r = A z from the original values is that right-hand side: the two solves undo the product
    assert np.array_equal(R[:, 0], ir.csr_mv(n, rp, cc, cv, z))
    print(f"{name}: {bits_l:.1f} and {bits_u:.1f} bits of 53")
    assert max(bits_l, bits_u) < 40
    if name in TRANSPOSED_NAMES:
        for flags in (L | T, L | UNIT | T, U | T, U | UNIT | T):
            ptr, col, val, diag, has, lower = tr.extract(n, rp, cc, expected, flags)
            bits, B = tr.assert_trsv_budget(n, ptr, col, val, diag, Z[:, :17], unit=bool(flags & UNIT))
            assert bits < 40 and np.array_equal(tr.solve_twin(n, ptr, col, val, diag, lower, B[:, 3], bool(flags & UNIT), 4), Z[:, 3])


def test_budget_of_the_large_bidiagonal_case():
    n, rp, cc, cv, x = tr.lower_bidiagonal_gaps(4099)
    ptr, col, val, diag, has, lower = tr.extract(n, rp, cc, cv, L)
    bits, b = tr.assert_trsv_budget(n, ptr, col, val, diag, np.stack([x, -x, 2 * x], axis=1), unit=False)
    hist = tr.level_hist(n, ptr, col, lower)
    assert len(hist) == 8 and hist.sum() == n and hist.min() >= n // 8 and tr.lanes_of(n, len(col)) == 1 and bits < 20
    assert np.array_equal(tr.solve_twin(n, ptr, col, val, diag, lower, b[:, 0], False), x)


def test_the_budget_refuses_what_is_over_it():
    ptr, col = np.array([0, 0, 1]), np.array([0])
    x = np.array([2.0**20, 1.0])
    tr.assert_trsv_budget(2, ptr, col, np.array([2.0**20]), np.ones(2), x, unit=False)  # 2^42 on the grid 2^-2: fine
    with pytest.raises(AssertionError, match="budget 53"):
        tr.assert_trsv_budget(2, ptr, col, np.array([2.0**28 + 0.25]), np.ones(2), np.array([2.0**26 + 1.0, 1.0]), unit=False)
    with pytest.raises(AssertionError, match="grid"):
        tr.assert_trsv_budget(2, ptr, col, np.array([0.125]), np.ones(2), x, unit=False)  # off the grid 2^-2
    with pytest.raises(AssertionError, match="power of two"):
        tr.assert_trsv_budget(2, ptr, col, np.array([1.0]), np.array([3.0, 1.0]), x, unit=False)
    tr.assert_trsv_budget(2, ptr, col, np.array([1.0]), np.array([3.0, 1.0]), x, unit=True)  # (unit: the diagonal is not looked at)
    with pytest.raises(AssertionError, match="grid"):
        tr.assert_trsv_budget(2, ptr, col, np.array([1.0]), np.ones(2), np.array([0.5, 1.0]), unit=False)  # x is not an integer


# ---- levels and launches -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EXACT_NAMES + ["laplacian_3d(12)", "random"])
def test_level_tables_are_level_sizes(name):
    if name == "random":
        n, rp, cc, cv = tr.random_system(257, 6, 9)
    elif name.startswith("laplacian"):
        n, rp, cc, cv = ir.laplacian_3d(12)
    else:
        n, rp, cc, cv = _case(name)[:4]
    want = ir.level_sizes(n, rp, cc, order=np.arange(n), merged=False)
    total = 0
    for i, (which, flags) in enumerate((("lower", L), ("upper", U))):
        ptr, col, val, diag, has, lower = tr.extract(n, rp, cc, cv, flags)
        hist = tr.level_hist(n, ptr, col, lower)
        assert np.array_equal(hist, want[which]), (name, which)
        assert tr.lanes_of(n, len(col)) == want["lanes"][i] and tr.schedule(hist, want["lanes"][i]) == want["schedule"][i]
        total += tr.launches(hist, want["lanes"][i])[0]
        # the transposed copy, handed to level_sizes as a matrix of its own: the same rule
        pt, ct, vt, _, _, lower_t = tr.extract(n, rp, cc, cv, flags | T)
        again = ir.level_sizes(n, pt, ct, order=np.arange(n), merged=False)
        assert np.array_equal(tr.level_hist(n, pt, ct, lower_t), again["lower" if lower_t else "upper"])
    assert total == want["launches"]


def test_k_column_launches_of_the_exact_cases():
    """at 16 lanes per row: cliques_tiny's 6000-row level and cliques_mixed's first two levels are launches of their own,
    cliques_130 and the bands one folded run per triangle"""
    def counts(name, flags, k):
        n, rp, cc, cv, expected, z = _case(name)
        ptr, col, val, diag, has, lower = tr.extract(n, rp, cc, expected, flags)
        hist = tr.level_hist(n, ptr, col, lower)
        return hist, tr.schedule(hist, tr.width_of(k)), tr.launches(hist, tr.width_of(k))

    assert [tr.width_of(k) for k in (1, 2, 3, 5, 8, 9, 16, 17, 33, 64)] == [1, 2, 4, 8, 8, 16, 16, 16, 16, 16]
    hist, sched, (total, own) = counts("cliques_tiny", L | UNIT, 16)
    assert hist[0] == 6000 and sched[0] == (0, 1) and own >= 1
    hist, sched, (total, own) = counts("cliques_mixed", L | UNIT, 64)
    assert sched[:2] == [(0, 1), (1, 1)] and own >= 2 and total > own
    for name in ("cliques_130", "band_1_20", "band_20_1", "band_3_3"):
        for flags in (L | UNIT, U):
            assert counts(name, flags, 16)[2] == (1, 0), name
