"""The NumPy twin of FSAI (tests/fsai_ref.py) held to facts of its own, evaluated in np.longdouble - on the CPU, so that the GPU test
(tests/test_gpu_fsai.py) compares the engine with something that was itself checked.

  - (G A G^T)_ii = 1 and (G A)_ij = 0 for j in S_i, j < i - the second is what defines G - on every problem the GPU test runs,
    relative to |G||A||G^T| and |G||A|: held to 8 eps each, measured 2.9 and 2.5 (fsai_ref.DIAG_BOUND_EPS / OFF_BOUND_EPS);
  - on a block-diagonal matrix of dense SPD blocks at level 1 the pattern holds the whole lower triangle of a block, so G is its
    inverse Cholesky factor: G A G^T = I in full, held to 8 eps of |G||A||G^T| (measured 2.9);
  - on diag(4^k), G = diag(2^-k) bit for bit;
  - two mutations break the defining fact by ten decades and more: the upper triangle as the pattern, and the last duplicate stored
    instead of the sum;
  - the iteration counts of the float64 CG twins that the GPU test compares the engine with."""
import numpy as np
import pytest

import fsai_ref as fr
import solver_ref
import tiled

PROBLEMS = {
    "tridiagonal_8": (fr.tridiagonal_8, (1, 2, 3)),
    "laplacian_2d_33": (lambda: fr.laplacian_2d(33), (1, 2, 3)),
    "stencil27_12": (lambda: fr.stencil27(12), (1, 2)),
    "dense_blocks": (lambda: fr.dense_blocks()[:4], (1,)),
    "random_symmetric": (fr.random_symmetric, (1,)),
    "diagonal": (fr.diagonal_powers_of_four, (1,)),
}
CASES = [(p, lv) for p, (_, levels) in PROBLEMS.items() for lv in levels]
FULL_BOUND_EPS = 8.0
_M = {}


def _matrix(problem):
    if problem not in _M:
        _M[problem] = PROBLEMS[problem][0]()
    return _M[problem]


@pytest.mark.parametrize("problem,level", CASES)
def test_the_two_facts_that_define_g(problem, level):
    n, rp, cc, cv = _matrix(problem)
    F = fr.Fsai(n, rp, cc, cv, level)
    lens = np.diff(F.rp)
    assert np.all(F.cc[F.rp[1:] - 1] == np.arange(n)) and np.all(lens >= 1) and F.max_row <= fr.MAX_ROW
    assert all(np.all(np.diff(F.cc[a:b]) > 0) for a, b in zip(F.rp[:-1], F.rp[1:]))
    diag, off = fr.residuals(n, rp, cc, cv, F.rp, F.cc, F.values)
    print(f"{problem} level {level}: nnz(G) = {F.nnz}, longest row {F.max_row}; (G A G^T)_ii - 1: {diag:.2f} eps, (G A)_ij on S: {off:.2f} eps")
    assert diag <= fr.DIAG_BOUND_EPS and off <= fr.OFF_BOUND_EPS, (diag, off)
    assert np.all(F.values[F.rp[1:] - 1] > 0)  # g_ii = 1 / c_mm


def test_the_patterns_are_the_sizes_the_gpu_test_relies_on():
    """longest rows: 2-D five-point 3 / 7 / 13; the 27-point stencil 14 and 63, one below the cap, and beyond it at level 3; every m
    from 1 to 64 in the dense blocks; the realistic refusal of the random matrix at level 2"""
    n, rp, cc, cv = _matrix("laplacian_2d_33")
    assert [int(np.diff(fr.pattern(n, rp, cc, lv)[0]).max()) for lv in (1, 2, 3)] == [3, 7, 13]
    n, rp, cc, cv = _matrix("stencil27_12")
    assert [int(np.diff(fr.pattern(n, rp, cc, lv)[0]).max()) for lv in (1, 2, 3)] == [14, 63, 172]
    with pytest.raises(fr.RowTooLong) as e:
        fr.Fsai(n, rp, cc, cv, 3)
    assert e.value.row == 183 and e.value.m == 74
    n, rp, cc, cv = _matrix("dense_blocks")
    assert sorted(set(np.diff(fr.pattern(n, rp, cc, 1)[0]).tolist())) == list(range(1, 65))
    with pytest.raises(fr.RowTooLong) as e:
        fr.Fsai(*fr.dense_blocks((64, 65, 3))[:4], 1)
    assert e.value.m == 65
    n, rp, cc, cv = _matrix("random_symmetric")
    lens1, lens2 = (np.diff(fr.pattern(n, rp, cc, lv)[0]) for lv in (1, 2))
    print(f"random_symmetric: level 1 longest row {lens1.max()}, mean {lens1.mean():.2f}; level 2 longest row {lens2.max()}")
    assert 8 < lens1.max() <= 16 and lens2.max() > fr.MAX_ROW
    # classes of 4, 8 and 16 lanes all occur at level 1
    assert (lens1 <= 4).any() and ((lens1 > 4) & (lens1 <= 8)).any() and (lens1 > 8).any()
    # duplicates (the doubled diagonal), stored zeros and unsorted columns are really there
    rows = np.repeat(np.arange(n), np.diff(rp))
    assert ((rows == cc).sum() == 2 * n) and (cv == 0).sum() > 1000 and any(np.any(np.diff(cc[a:b]) < 0) for a, b in zip(rp[:50], rp[1:51]))


def test_dense_blocks_give_the_inverse_cholesky_factor():
    n, rp, cc, cv, owner, rank = fr.dense_blocks()
    F = fr.Fsai(n, rp, cc, cv, 1)
    worst = 0.0
    for b in range(int(owner.max()) + 1):
        A, idx = fr.block_of(n, rp, cc, cv, owner, b)
        G = np.zeros_like(A)
        where = np.full(n, -1)
        where[idx] = np.arange(len(idx))
        for k, i in enumerate(idx):
            G[k, where[F.cc[F.rp[i]:F.rp[i + 1]]]] = F.values[F.rp[i]:F.rp[i + 1]]
        assert np.all(np.triu(G, 1) == 0)
        Al, Gl = A.astype(fr.LD), G.astype(fr.LD)
        err = np.abs(Gl @ Al @ Gl.T - np.eye(len(idx))) / (np.abs(Gl) @ np.abs(Al) @ np.abs(Gl.T))
        worst = max(worst, float(err.max()) / fr.EPS)
        # the inverse of numpy's Cholesky factor, to rounding (condition 2.6)
        assert np.allclose(G, np.linalg.inv(np.linalg.cholesky(A)), rtol=0, atol=1e-13)
        assert np.linalg.cond(A) < 3.0
    print(f"dense_blocks: |G A G^T - I| / |G||A||G^T| = {worst:.2f} eps")
    assert worst <= FULL_BOUND_EPS


def test_a_diagonal_of_powers_of_four_gives_its_square_roots_bit_for_bit():
    n, rp, cc, cv = fr.diagonal_powers_of_four()
    F = fr.Fsai(n, rp, cc, cv, 1)
    assert np.array_equal(F.cc, np.arange(n)) and F.values.tobytes() == (1.0 / np.sqrt(cv)).tobytes()
    r = np.random.default_rng(3).uniform(-1, 1, n)
    assert F.apply(r).tobytes() == (r / cv).tobytes()


@pytest.mark.parametrize("mutate", ["upper", "last_wins"])
def test_mutations_break_the_defining_fact(mutate):
    n, rp, cc, cv = _matrix("laplacian_2d_33")
    if mutate == "last_wins":  # every off-diagonal -1 stored as -1/2 twice (the mutated matrix, diagonal 4 and -1/2, is still SPD)
        rows = np.repeat(np.arange(n), np.diff(rp))
        twice = np.where(rows == cc, 1, 2)
        rows, cc, cv = np.repeat(rows, twice), np.repeat(cc, twice), np.repeat(cv / twice, twice)
        rp = np.searchsorted(rows, np.arange(n + 1))
    s_rp, s_cc = fr.pattern(n, rp, cc, 1)
    good = fr.Fsai(n, rp, cc, cv, 1)
    bad = fr.Fsai(n, rp, cc, cv, 1, mutate=mutate)
    d0, o0 = fr.residuals(n, rp, cc, cv, good.rp, good.cc, good.values, s_rp, s_cc)
    d1, o1 = fr.residuals(n, rp, cc, cv, bad.rp, bad.cc, bad.values, s_rp, s_cc)
    print(f"{mutate}: (G A)_ij on S {o0:.2f} eps -> {o1:.3e} eps; diagonal {d0:.2f} eps -> {d1:.3e} eps")
    assert o0 <= fr.OFF_BOUND_EPS and o1 > 1e10 * fr.OFF_BOUND_EPS, (o0, o1)


def test_a_missing_diagonal_entry_and_a_negative_pivot_name_their_rows():
    with pytest.raises(ValueError, match="row 2 "):
        fr.Fsai(3, [0, 1, 2, 3], [0, 1, 0], [1.0, 1.0, 1.0], 1)
    with pytest.raises(ZeroDivisionError, match="row 1 "):
        fr.Fsai(2, [0, 2, 4], [0, 1, 0, 1], [1.0, 2.0, 2.0, 1.0], 1)


def test_block_diagonal_copies_tile_the_twin():
    """the oracle of the GPU test's later trips over the grid (tests/tiled.py): the twin of k copies is the twin of the base, tiled -
    pattern and bytes - at a level with two sparse products in the pattern, and on dense blocks"""
    for copies, level, (n, rp, cc, cv) in ((4, 3, fr.laplacian_2d(8)), (3, 1, fr.dense_blocks((9, 5, 3))[:4])):
        base = fr.Fsai(n, rp, cc, cv, level)
        F = fr.Fsai(copies * n, *tiled.tile_csr(copies, n, rp, cc, cv), level)
        got = (F.rp.astype(np.int32), F.cc.astype(np.int32), F.values)
        assert tiled.tiled_mismatch(got, (base.rp, base.cc, base.values), copies, n) is None
        assert (F.nnz, F.max_row) == (copies * base.nnz, base.max_row)
    # ... and a value of a later copy one ulp off is named by copy, row, m and trip
    case = fr.grid_loop_case(16)
    ref, k = case["ref"], 3
    want = tiled.tile_csr(k, case["n"], ref.rp, ref.cc, ref.values)
    row = int(np.flatnonzero(case["m"] > 8)[0])
    val = want[2].copy()
    at = 2 * ref.nnz + int(ref.rp[row])
    val[at] = np.nextafter(val[at], -np.inf)
    said = tiled.tiled_mismatch((want[0], want[1], val), (ref.rp, ref.cc, ref.values), k, case["n"], case["where"])
    assert said.startswith(f"val[{at}] ") and f"copy 2, row {row} (m = {int(case['m'][row])}, place {2 * case['rows']} of class of 16 lanes, trip 0)" in said, said


# lanes: (rows of the class in a copy, copies): the figures the GPU test's sizes rest on
GRID_LOOP_SIZES = {4: (9, 14564), 8: (49, 1338), 16: (45, 729), 32: (43, 382), 64: (47, 131)}


@pytest.mark.parametrize("lanes", sorted(fr.GRID_LOOP_BASES))
def test_the_grid_loop_cases_reach_a_second_trip(lanes):
    """the coverage conditions of tests/test_gpu_fsai.py's later-trip test, without a GPU"""
    case = fr.grid_loop_case(lanes)
    k, rows, groups, grid = case["copies"], case["rows"], case["groups"], case["grid"]
    print(f"{lanes} lanes: {k} copies x {rows} rows = {k * rows}, {groups} groups a workgroup, {grid} workgroups: "
          f"{tiled.trips(k * rows, groups, grid)} trips; n = {k * case['n']}, nnz(A) = {k * len(case['cc'])}, nnz(G) = {k * case['ref'].nnz}")
    assert (rows, k) == GRID_LOOP_SIZES[lanes]
    assert k * rows > groups * grid >= (k - 1) * rows and (groups * grid) % rows != 0 and tiled.trips(k * rows, groups, grid) == 2
    assert groups == {4: 64, 8: 32, 16: 16, 32: 8, 64: 3}[lanes]
    m = case["m"][np.array([tiled.fsai_class_of(x) for x in case["m"]]) == tiled.fsai_lanes().index(lanes)]
    assert lanes // 2 < m.min() <= m.max() <= lanes if lanes > 4 else m.max() <= 4
    assert len(set(m.tolist())) > 1, "rows of different lengths follow one another in a group"


@pytest.mark.parametrize("system", fr.SOLVER_SYSTEMS)
def test_iteration_counts_of_the_twins(system):
    plain = fr.twin_iterations(system, 0)
    print(f"{system}: without a preconditioner {plain}")
    assert set(plain.values()) == {fr.UNPRECONDITIONED_ITERATIONS[system]}
    for level in (1, 2, 3):
        got = fr.twin_iterations(system, level)
        print(f"{system} level {level}: {got}")
        assert (min(got.values()), max(got.values())) == fr.TWIN_ITERATIONS[system, level]
        assert max(got.values()) < fr.UNPRECONDITIONED_ITERATIONS[system]
    assert solver_ref.F == 8.0  # (the factor the GPU gates multiply the bounds above with)
