"""The NumPy twin of spmv_spgemm / spmv_csr_transpose (tests/spgemm_ref.py) held to facts of its own: a scalar triple loop, the dense
product's pattern, scipy's bytes, the integer reference on dyadic inputs, amg_ref's coarse operator as a triple product - and
mutants of the definition, each of which must change bytes on the inputs the GPU tests use."""
import numpy as np
import pytest

import amg_ref
import exact
import spgemm_ref as sr
import tiled


def _dense(nrow, ncol, M):
    rp, cc, cv = M
    d = np.zeros((nrow, ncol))
    np.add.at(d, (np.repeat(np.arange(nrow), np.diff(rp)), cc), cv)
    return d


def _pattern(nrow, ncol, M):
    rp, cc, _ = M
    p = np.zeros((nrow, ncol), dtype=bool)
    p[np.repeat(np.arange(nrow), np.diff(rp)), cc] = True
    return p


SMALL = {
    "order_sensitive": sr.order_sensitive_pair,
    "cancelling": sr.cancelling_pair,
    "empty_rows": lambda: (6, 5, 7, sr.csr_of(6, [0, 0, 2, 5], [1, 3, 4, 1], [1.5, -2.0, 0.5, 3.0]), sr.csr_of(5, [1, 1, 4, 4], [6, 0, 2, 2], [1.0, 2.0, 3.0, 4.0])),
    "no_entries": lambda: (4, 3, 5, sr.csr_of(4, [], [], []), sr.random_rows(3, 5, 2, 5)),
    "one_row_runs": lambda: sr.one_row_case(17, False),
    "one_row_one_run": lambda: sr.one_row_case(17, True),
}


@pytest.mark.parametrize("name", sorted(SMALL))
def test_twin_equals_the_scalar_triple_loop_and_the_dense_pattern(name):
    m, k, n, A, B = SMALL[name]()
    rp, cc, cv, ub = sr.spgemm_twin(m, k, n, A, B)
    loops = sr.triple_loop(m, k, n, A, B)
    assert rp[0] == 0 and rp[-1] == len(cc) == len(cv) == sum(len(r) for r in loops)
    for i in range(m):
        cols = cc[rp[i]:rp[i + 1]]
        assert np.all(np.diff(cols) > 0), "columns ascend strictly"
        assert list(cols) == sorted(loops[i])
        assert cv[rp[i]:rp[i + 1]].tobytes() == np.array([loops[i][int(c)] for c in cols], dtype=np.float64).tobytes()
    assert np.array_equal(_pattern(m, n, (rp, cc, cv)), (_pattern(m, k, A).astype(np.int64) @ _pattern(k, n, B).astype(np.int64)) > 0)
    reach = np.repeat(np.arange(m), np.diff(A[0]))
    assert np.array_equal(ub, np.bincount(reach, weights=np.diff(B[0])[A[1]], minlength=m).astype(np.int64))


@pytest.mark.parametrize("name", sorted(SMALL))
def test_twin_equals_scipy_bytes(name):
    sp = pytest.importorskip("scipy.sparse")
    m, k, n, A, B = SMALL[name]()
    C = sp.csr_matrix((A[2], A[1], A[0]), shape=(m, k)) @ sp.csr_matrix((B[2], B[1], B[0]), shape=(k, n))
    C.sort_indices()
    # scipy drops a sum that is 0.0 from its result; the engine's pattern is structural.  Where zeros occur, scipy is the mutant
    # that removes them - and the twin must hold them
    rp, cc, cv, _ = sr.spgemm_twin(m, k, n, A, B)
    if 0.0 in cv:
        assert name == "cancelling"
        rp, cc, cv, _ = sr.spgemm_twin(m, k, n, A, B, mutate="cancelled_removed")
    assert np.array_equal(C.indptr, rp) and np.array_equal(C.indices, cc) and C.data.tobytes() == cv.tobytes()


def test_twin_is_exact_on_dyadic_inputs():
    m, k, n = 64, 48, 80
    A0, B0 = sr.random_rows(m, k, 8, 11), sr.random_rows(k, n, 9, 12)
    _, _, _, ub = sr.spgemm_twin(m, k, n, A0, B0)
    bits, e = exact.choose_bits(int(ub.max()))
    A, B = sr.random_rows(m, k, 8, 11, "dyadic", bits, e), sr.random_rows(k, n, 9, 12, "dyadic", bits, e)
    rp, cc, cv, _ = sr.spgemm_twin(m, k, n, A, B)
    want = exact.scaled(_dense(m, k, A), e).astype(object) @ exact.scaled(_dense(k, n, B), e).astype(object)
    got = exact.scaled(cv, 2 * e)
    rows = np.repeat(np.arange(m), np.diff(rp))
    assert all(int(want[i, j]) == int(g) for i, j, g in zip(rows, cc, got))
    assert np.array_equal(_pattern(m, n, (rp, cc, cv)), (_pattern(m, k, A).astype(np.int64) @ _pattern(k, n, B).astype(np.int64)) > 0)


def test_triple_product_equals_the_amg_coarse_operator():
    n, A = sr.laplacian_2d(32)
    agg, nc, _, _ = amg_ref.aggregate(n, *A)
    P = (np.arange(n + 1, dtype=np.int32), agg.astype(np.int32), np.ones(n))
    Pt = sr.transpose_twin(n, nc, P)
    AP = sr.spgemm_twin(n, n, nc, A, P)[:3]
    rp, cc, cv, _ = sr.spgemm_twin(nc, n, nc, Pt, AP)
    want = amg_ref.coarse_operator(n, *A, agg, nc)
    assert (nc, len(cc)) == (150, 906)
    assert np.array_equal(rp, want[0]) and np.array_equal(cc, want[1]) and cv.tobytes() == np.asarray(want[2]).tobytes()


def test_transpose_twin():
    m, n = 9, 6
    A = sr.random_rows(m, n, 5, 77)
    rp, cc, cv = sr.transpose_twin(m, n, A)
    assert np.array_equal(_dense(n, m, (rp, cc, cv)), _dense(m, n, A).T) and len(cc) == len(A[1])
    for j in range(n):
        assert np.all(np.diff(cc[rp[j]:rp[j + 1]]) >= 0)
    back = sr.transpose_twin(n, m, (rp, cc, cv))
    want = sr.sorted_columns(m, A)
    assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(back, want))


def test_block_diagonal_copies_tile_the_twin():
    """the oracle of the GPU test's later trips over the grid (tests/tiled.py): the twin of k copies is the twin of the base, tiled"""
    for copies, (m, k, n, A, B) in ((5, sr.order_sensitive_pair()), (3, sr.class_edge_pair()), (1, sr.cancelling_pair())):
        base = sr.spgemm_twin(m, k, n, A, B)
        got = sr.spgemm_twin(copies * m, copies * k, copies * n, tiled.tile_csr(copies, k, *A), tiled.tile_csr(copies, n, *B))
        assert tiled.tiled_mismatch(got[:3], base[:3], copies, n) is None
        assert np.array_equal(got[3], np.tile(base[3], copies))
        want = tiled.tile_csr(copies, n, *base[:3])
        assert all(np.asarray(g).dtype == w.dtype and np.asarray(g).tobytes() == w.tobytes() for g, w in zip(got[:3], want))


def test_the_grid_loop_case_reaches_later_trips_and_names_what_differs():
    """the coverage conditions of tests/test_gpu_spgemm.py's later-trip test, without a GPU, and its reporter: a tiled result with one
    value of the last copy moved by one ulp, one column changed, one row one entry short - each named by copy, row, class and trip"""
    case = sr.grid_loop_case()
    k, n, grid = case["copies"], case["n"], case["grid"]
    rp0, cc0, cv0, ub0 = case["twin"]
    assert tuple(int(u) for u in ub0) == sr.CLASS_EDGE_UB and len(cc0) > 0
    assert {c: v[0] for c, v in case["looping"].items()} == {2: "wave", 3: "block"}
    for label, rows, per_group in case["looping"].values():
        print(f"class {label}: {k * rows} rows, {per_group} a workgroup, {grid} workgroups: {tiled.trips(k * rows, per_group, grid)} trips")
        assert k * rows > per_group * grid and (per_group * grid) % rows != 0 and tiled.trips(k * rows, per_group, grid) >= 2
    assert any((k - 2) * rows <= per_group * grid for _, rows, per_group in case["looping"].values()), "no more copies than a second trip needs"
    good = tiled.tile_csr(k, n, rp0, cc0, cv0)
    assert tiled.tiled_mismatch(good, (rp0, cc0, cv0), k, n, case["where"]) is None
    wave_rows, block_rows = np.flatnonzero(case["cls"] == 2), np.flatnonzero(case["cls"] == 3)
    last = k - 1
    # a value of the last workgroup-class row of the last copy, one ulp off
    row, place = int(block_rows[-1]), last * len(block_rows) + len(block_rows) - 1
    val = good[2].copy()
    at = last * len(cc0) + int(rp0[row]) + 1
    val[at] = np.nextafter(val[at], np.inf)
    said = tiled.tiled_mismatch((good[0], good[1], val), (rp0, cc0, cv0), k, n, case["where"])
    assert said.startswith(f"val[{at}] ") and f"copy {last}, row {row} (place {place} of class block, trip {place // grid})" in said, said
    assert place // grid >= 1
    # a column of the last wavefront-class row of the last copy
    row, place = int(wave_rows[-1]), last * len(wave_rows) + len(wave_rows) - 1
    col = good[1].copy()
    at = last * len(cc0) + int(rp0[row + 1]) - 1
    col[at] += 1
    said = tiled.tiled_mismatch((good[0], col, good[2]), (rp0, cc0, cv0), k, n, case["where"])
    per_group = case["looping"][2][2]
    assert said.startswith(f"col[{at}] ") and f"copy {last}, row {row} (place {place} of class wave, trip {place // per_group // grid})" in said, said
    assert place // per_group // grid == 1
    # a row of copy 1 one entry short: the first row_ptr that differs closes that row
    rp = good[0].copy()
    rp[len(rp0) - 1 + row + 1:] -= 1
    said = tiled.tiled_mismatch((rp, good[1], good[2]), (rp0, cc0, cv0), k, n, case["where"])
    assert said.startswith("row_ptr[") and f"copy 1, row {row} (place {len(wave_rows) + len(wave_rows) - 1} of class wave, trip 0)" in said, said
    # another shape or type is said as such
    assert "int64" in tiled.tiled_mismatch((good[0].astype(np.int64), good[1], good[2]), (rp0, cc0, cv0), k, n)


@pytest.mark.parametrize("mutant", sr.MUTANTS)
def test_every_mutant_changes_bytes_on_the_gpu_tests_inputs(mutant):
    name = "cancelling" if mutant == "cancelled_removed" else "order_sensitive"
    m, k, n, A, B = SMALL[name]()
    good, bad = sr.spgemm_twin(m, k, n, A, B), sr.spgemm_twin(m, k, n, A, B, mutate=mutant)
    same = all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(good[:3], bad[:3]))
    assert not same, mutant
    if name == "order_sensitive":
        assert int(good[3].sum()) == 5760 and 3 * len(good[1]) < 5760  # more than three addends an entry on average
        if mutant in ("reversed", "fma"):
            assert len(good[2]) == len(bad[2]) and int(np.sum(good[2] != bad[2])) > 100  # runs of three and more addends
