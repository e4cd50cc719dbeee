"""spmv_spgemm and spmv_csr_transpose on the GPU against their NumPy twin (tests/spgemm_ref.py), as bytes: row_ptr, col and val of
every result under ROWS, SORT and AUTO, the result's own validation and its "spgemm_*" parameters; the class edges and the capacity
read from the settings header and from "spgemm_lds_products"; block-diagonal copies that take the wavefront and the workgroup class
on later trips over the grid (tests/tiled.py); a hub on the sort path spliced among short rows; the transpose; the
Galerkin product against spmv_amg_setup's level 1; the result as a handle; device memory around results and a refused call."""
import functools
import re
from pathlib import Path

import numpy as np
import pytest

import exact
import spgemm_ref as sr
import tiled

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
METHODS = (("ROWS", 1), ("SORT", 2), ("AUTO", 0))


def _dyadic_pair():
    m, k, n = 64, 48, 80
    _, _, _, ub = sr.spgemm_twin(m, k, n, sr.random_rows(m, k, 8, 11), sr.random_rows(k, n, 9, 12))
    bits, e = exact.choose_bits(int(ub.max()))
    return m, k, n, sr.random_rows(m, k, 8, 11, "dyadic", bits, e), sr.random_rows(k, n, 9, 12, "dyadic", bits, e)


def _squared(build):
    n, A = build()
    return n, n, n, A, A


def _tiny(n):
    A = sr.random_rows(n, n, 2, 40 + n)
    return n, n, n, A, A


def _empty_rows():
    # rows 1, 3 and 4 of A are empty; row 2 reaches only rows 0 and 2 of B, which are empty; the last rows of C are empty
    A = sr.csr_of(8, [0, 0, 2, 2, 5], [1, 3, 0, 2, 1], [1.5, -2.0, 0.5, 3.0, 0.7])
    B = sr.csr_of(5, [1, 1, 3, 3, 4], [6, 0, 2, 2, 5], [1.0, 2.0, 3.0, 4.0, 5.0])
    return 8, 5, 7, A, B


CASES = {
    "laplacian32_squared": lambda: _squared(lambda: sr.laplacian_2d(32)),
    "dyadic_64x48x80": _dyadic_pair,
    "arrow300_squared": lambda: _squared(lambda: (300, sr.arrow(300))),
    "n1": lambda: _tiny(1),
    "n2": lambda: _tiny(2),
    "n3": lambda: _tiny(3),
    "identity_times_a": lambda: (40, 40, 30, sr.identity(40), sr.random_unique_rows(40, 30, 12, 101)),
    "a_times_identity": lambda: (40, 30, 30, sr.random_unique_rows(40, 30, 12, 101), sr.identity(30)),
    "order_sensitive": sr.order_sensitive_pair,
    "cancelling": sr.cancelling_pair,
    "empty_rows": _empty_rows,
    "no_entries": lambda: (4, 3, 5, sr.csr_of(4, [], [], []), sr.random_rows(3, 5, 2, 5)),
    "tridiagonal_1048579_squared": lambda: _squared(lambda: (1048579, sr.tridiagonal(1048579))),
    "hub": sr.hub_case,
}
EXACT = ("laplacian32_squared", "dyadic_64x48x80", "arrow300_squared")


@functools.lru_cache(maxsize=None)
def _case(name):
    m, k, n, A, B = CASES[name]()
    return m, k, n, A, B, sr.spgemm_twin(m, k, n, A, B)


def _bytes_equal(got, want, what):
    for g, w, part in zip(got, want, ("row_ptr", "col", "val")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {part} has {g.shape} {g.dtype}, the twin {w.shape} {w.dtype}"
        if g.tobytes() != w.tobytes():
            at = int(np.flatnonzero(g.view(np.uint8).reshape(len(g), -1) != w.view(np.uint8).reshape(len(w), -1))[0]) // g.itemsize
            raise AssertionError(f"{what}: {part} differs from the twin, first at {at}: {g[at]!r} against {w[at]!r}")


def _product(ctx, m, k, n, A, B, method):
    dA, dB = ctx.csr(m, k, *A), ctx.csr(k, n, *B)
    return ctx.spgemm(dA, dB, method)


def _capacities():
    text = (ROOT / "arm-spmv_amd" / "csrc" / "spgemm_settings.hpp").read_text()
    caps = sorted(int(c) for _, c in re.findall(r"spgemm_class_info\{(\d+), (\d+)\}", text) if int(c) > 0)
    assert len(caps) >= 2, "at least two LDS classes"
    return caps


@pytest.mark.parametrize("name", list(CASES))
def test_product_equals_the_twin_as_bytes_under_every_method(ctx, name):
    m, k, n, A, B, (rp, cc, cv, ub) = _case(name)
    if name in EXACT:  # the twin itself against integers: every value of C is exact, so no order can matter
        dense = lambda r, c, M: np.bincount(np.repeat(np.arange(r), np.diff(M[0])) * c + M[1], weights=M[2], minlength=r * c).reshape(r, c)
        want = dense(m, k, A) @ dense(k, n, B)
        assert np.array_equal(want[np.repeat(np.arange(m), np.diff(rp)), cc], cv)
    if name in ("identity_times_a", "a_times_identity"):  # (no duplicates in this A: the product is A with sorted columns)
        _bytes_equal((rp, cc, cv), sr.sorted_columns(m, B if name == "identity_times_a" else A), name)
    cap = None
    for label, method in METHODS:
        C = _product(ctx, m, k, n, A, B, method)
        info = C.info
        assert (info.nrow, info.ncol, info.nnz) == (m, n, len(cc)), label
        _bytes_equal(C.download(), (rp, cc, cv), f"{name} under {label}")
        C.validate()
        assert C.get_param("spgemm_products") == int(ub.sum()), label
        cap = C.get_param("spgemm_lds_products")
        assert cap >= 2048
        on_sort = int(np.sum(ub > 0)) if label == "SORT" else int(np.sum(ub > cap))
        assert C.get_param("spgemm_rows_sorted") == on_sort and C.get_param("spgemm_rows_lds") == int(np.sum(ub > 0)) - on_sort, label
    if name == "hub":
        assert int(np.sum(ub > cap)) == 200 and int(ub.sum()) > 1_000_000 and 0 < int(np.sum((ub > 0) & (ub <= cap)))
    if name == "empty_rows":
        assert rp[-1] == rp[-3] and np.any(np.diff(rp) == 0)
    if name == "no_entries":
        assert len(cc) == 0


@pytest.mark.parametrize("one_column", [False, True], ids=["c_runs", "one_run_of_c"])
def test_class_edges_and_the_capacity(ctx, one_column):
    caps = _capacities()
    probe = _product(ctx, 1, 1, 1, *sr.one_row_case(1, False)[3:], 1)
    assert probe.get_param("spgemm_lds_products") == caps[-1], "the settings header and the parameter agree on the capacity"
    sizes = sorted({c + d for c in caps for d in (-1, 0, 1)})
    for c in sizes:
        m, k, n, A, B = sr.one_row_case(c, one_column)
        rp, cc, cv, ub = sr.spgemm_twin(m, k, n, A, B)
        assert int(ub[0]) == c and len(cc) == (1 if one_column else c)
        for label, method in METHODS:
            C = _product(ctx, m, k, n, A, B, method)
            _bytes_equal(C.download(), (rp, cc, cv), f"c = {c} under {label}")
            C.validate()
            sorted_rows = 1 if (label == "SORT" or c > caps[-1]) else 0
            assert (C.get_param("spgemm_rows_lds"), C.get_param("spgemm_rows_sorted")) == (1 - sorted_rows, sorted_rows), (c, label)
            assert C.get_param("spgemm_products") == c


def test_rows_on_a_later_trip_over_the_grid_repeat_the_first_trip(ctx):
    """spgemm_rows_kernel launches at most kMaxGrid workgroups and loops beyond: block-diagonal copies of sr.class_edge_pair put
    8200 rows into the wavefront class (4 a workgroup: two trips) and into the workgroup class (1 a workgroup: five), and C must
    be the base twin tiled (tests/tiled.py).  Five rows of a class a copy do not divide a trip's rows, so a workgroup meets rows of
    another length - another network size - on its later trips, and rows of different network sizes side by side."""
    case = sr.grid_loop_case()
    m0, k0, n0, grid, k = case["m"], case["k"], case["n"], case["grid"], case["copies"]
    rp0, cc0, cv0, ub0 = case["twin"]
    assert tuple(int(u) for u in ub0) == sr.CLASS_EDGE_UB, "the twin counts the products the rows were built for"
    caps = _capacities()
    assert caps == case["caps"]
    for c, (label, rows, per_group) in case["looping"].items():
        lo, hi = case["caps"][c - 2], case["caps"][c - 1]
        have = sorted(int(u) for u in ub0[case["cls"] == c])
        assert have[0] == lo + 1 and have[-1] == hi, f"both edges of class {label}: {have}"
        assert any(p in have and p + 1 in have for p in (1 << b for b in range(1, 12))), f"a full network and one over in class {label}: {have}"
        print(f"class {label}: {k} copies x {rows} rows = {k * rows} > {per_group} x {grid} = {per_group * grid}: "
              f"{tiled.trips(k * rows, per_group, grid)} trips")
        assert k * rows > per_group * grid, f"class {label} makes one trip over the grid: nothing of this test is left"
        assert (per_group * grid) % rows != 0, f"{rows} rows a copy divide a trip of class {label}: every trip holds the same rows"
    A, B = tiled.tile_csr(k, k0, *case["A"]), tiled.tile_csr(k, n0, *case["B"])
    products, nonempty = k * int(ub0.sum()), k * int(np.sum(ub0 > 0))
    assert int(ub0.max()) <= caps[-1]
    for label, method in METHODS:
        C = _product(ctx, k * m0, k * k0, k * n0, A, B, method)
        assert (C.info.nrow, C.info.ncol, C.info.nnz) == (k * m0, k * n0, k * len(cc0)), label
        bad = tiled.tiled_mismatch(C.download(), (rp0, cc0, cv0), k, n0, case["where"])
        assert bad is None, f"under {label}: {bad}"
        C.validate()
        on_sort = nonempty if label == "SORT" else 0
        assert C.get_param("spgemm_products") == products, label
        assert (C.get_param("spgemm_rows_lds"), C.get_param("spgemm_rows_sorted")) == (nonempty - on_sort, on_sort), label
        del C


@pytest.mark.parametrize("m, k, n", [(0, 3, 4), (3, 0, 4), (3, 2, 0), (0, 0, 0)])
def test_shapes_with_a_zero_are_allowed_as_the_upload_allows_them(ctx, m, k, n):
    A = sr.random_rows(m, k, 2, 3) if m and k else sr.csr_of(m, [], [], [])
    B = sr.random_rows(k, n, 2, 4) if k and n else sr.csr_of(k, [], [], [])
    rp, cc, cv, _ = sr.spgemm_twin(m, k, n, A, B)
    assert len(cc) == 0
    for label, method in METHODS:
        C = _product(ctx, m, k, n, A, B, method)
        assert (C.info.nrow, C.info.ncol, C.info.nnz) == (m, n, 0), label
        _bytes_equal(C.download(), (rp, cc, cv), f"{m} x {k} x {n} under {label}")
        C.validate()
    T = ctx.csr_transpose(ctx.csr(m, k, *A))
    assert (T.info.nrow, T.info.ncol, T.info.nnz) == (k, m, len(A[1]))
    _bytes_equal(T.download(), sr.transpose_twin(m, k, A), f"transpose of {m} x {k}")


def test_parameters_read_zero_on_other_handles(ctx):
    A = ctx.csr(3, 3, *sr.identity(3))
    for name in ("spgemm_products", "spgemm_rows_lds", "spgemm_rows_sorted", "spgemm_lds_products"):
        assert A.get_param(name) == 0, name
    assert ctx.csr_transpose(A).get_param("spgemm_lds_products") == 0


def test_transpose_equals_the_twin_and_the_transposed_product(ctx):
    m, n = 37, 23
    rng = np.random.default_rng(5)
    A = sr.random_rows(m, n, 9, 88, "dyadic", 6, 4)  # rectangular, duplicates, unsorted
    dA = ctx.csr(m, n, *A)
    dAt = ctx.csr_transpose(dA)
    want = sr.transpose_twin(m, n, A)
    assert (dAt.info.nrow, dAt.info.ncol, dAt.info.nnz) == (n, m, len(A[1]))
    _bytes_equal(dAt.download(), want, "transpose")
    dAt.validate()
    back = ctx.csr_transpose(dAt)
    _bytes_equal(back.download(), sr.sorted_columns(m, A), "transpose of the transpose")
    x = exact.dyadic(rng, m, 6, 4)
    dx, y1, y2 = ctx.vector_from(x), ctx.vector(n), ctx.vector(n)
    y1.fill(0.0)
    y2.fill(0.0)
    ctx.apply(dAt, dx, y1)
    ctx.apply_transpose(dA, dx, y2)
    ctx.sync()
    assert y1.download().tobytes() == y2.download().tobytes()
    # an empty matrix and one long column
    E = ctx.csr_transpose(ctx.csr(4, 6, *sr.csr_of(4, [], [], [])))
    assert (E.info.nrow, E.info.ncol, E.info.nnz) == (6, 4, 0) and not np.any(E.download()[0])
    col = (np.arange(3001, dtype=np.int32), np.zeros(3000, dtype=np.int32), rng.uniform(-1, 1, 3000))
    _bytes_equal(ctx.csr_transpose(ctx.csr(3000, 2, *col)).download(), sr.transpose_twin(3000, 2, col), "one column of 3000 entries")


def test_galerkin_product_equals_the_amg_set_ups_level_one(ctx):
    n, A = sr.laplacian_2d(32)
    dA = ctx.csr(n, n, *A)
    ctx.amg_setup(dA)
    levels, rows, _ = ctx.amg_info(dA)
    assert levels >= 2
    agg = ctx.amg_level(dA, 0)[0]
    nc = int(rows[1])
    dP = ctx.csr(n, nc, np.arange(n + 1, dtype=np.int32), agg, np.ones(n))
    for _, method in METHODS:
        C = ctx.spgemm(ctx.csr_transpose(dP), ctx.spgemm(dA, dP, method), method)
        _bytes_equal(C.download(), ctx.amg_level(dA, 1)[1:], "P^T (A P)")  # (integers: the order cannot matter)


def test_the_result_is_an_ordinary_handle(ctx):
    m, k, n = 64, 48, 80
    A, B = sr.random_rows(m, k, 8, 11, "dyadic", 4, 2), sr.random_rows(k, n, 9, 12, "dyadic", 4, 2)
    rp, cc, cv, _ = sr.spgemm_twin(m, k, n, A, B)
    rng = np.random.default_rng(9)
    dA, dB = ctx.csr(m, k, *A), ctx.csr(k, n, *B)
    C = ctx.spgemm(dA, dB)
    again = ctx.spgemm(dA, dB)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(C.download(), again.download())), "two runs, equal bytes"
    x = exact.dyadic(rng, n, 3, 1)  # 4-bit values on 2^-2 .. 2^2, x 3 bits on 2^-1 .. 2: A (B x) and C x stay far below 2^53, so exact in any order
    dx, t, y1, y2 = ctx.vector_from(x), ctx.vector(k), ctx.vector(m), ctx.vector(m)
    for v in (t, y1, y2):
        v.fill(0.0)
    ctx.apply(dB, dx, t)
    ctx.apply(dA, t, y1)
    ctx.apply(C, dx, y2)
    ctx.sync()
    dense = np.zeros((m, n))
    np.add.at(dense, (np.repeat(np.arange(m), np.diff(rp)), cc), cv)
    assert y1.download().tobytes() == y2.download().tobytes() == (dense @ x).tobytes()
    # as an input of another product: (A B) B^T against the twin
    Bt = sr.transpose_twin(k, n, B)
    D = ctx.spgemm(C, ctx.csr_transpose(dB))
    _bytes_equal(D.download(), sr.spgemm_twin(m, n, k, (rp, cc, cv), Bt)[:3], "(A B) B^T")


def test_device_memory_is_back_after_results_and_after_a_refused_call(ctx, pkg):
    m, k, n, A, B, _ = _case("hub")
    dA, dB = ctx.csr(m, k, *A), ctx.csr(k, n, *B)

    def round_trip():
        for _, method in METHODS:
            C = ctx.spgemm(dA, dB, method)
            T = ctx.csr_transpose(C)
            del C, T
        with pytest.raises(pkg.capi.SpmvError, match="the columns of A must be the rows of B"):
            ctx.spgemm(dA, dA)
        ctx.sync()

    round_trip()  # (what the context itself keeps grows on first use)
    before = ctx.mem_info()[0]
    round_trip()
    assert ctx.mem_info()[0] == before
