"""The reordering entry points on the GPU (csrc/reorder.hip): spmv_perm_rcm returns the twin's permutation integer for integer
(tests/rcm_ref.py), the permuted handle holds the twin's bytes and meets the bandwidth bound of a level-structure numbering, a
renumbered product is the same product bit for bit, vectors travel as bits, and nothing but the permutation stays allocated."""
import functools

import numpy as np
import pytest

import exact
import rcm_ref as rr

pytestmark = pytest.mark.gpu

CASES = {
    "n0": lambda: rr.from_edges(0, [], []),
    "n1": lambda: rr.from_edges(1, [], []),
    "n2": lambda: rr.from_edges(2, [0], [1]),
    "path1025": lambda: rr.shuffled(rr.path(1025), 1),               # more levels than any batch of levels
    "grid37x23": lambda: rr.shuffled(rr.grid(37, 23), 2),            # a regular mesh under a bad numbering
    "grid9x9x9": lambda: rr.grid(9, 9, 9),
    "star5000": lambda: rr.star(5000),                               # one vertex wider than a workgroup; 5000 equal keys
    "k70": lambda: rr.complete(70),
    "random20000": lambda: rr.random_graph(20000, 60000, 6),         # frontiers of thousands
    "random300": lambda: rr.shuffled(rr.random_graph(300, 200, 8), 9),  # many components and isolated vertices
    "random300_one_sided": lambda: rr.one_sided_noisy(rr.shuffled(rr.random_graph(300, 200, 8), 9), 10),
    "band2000": lambda: rr.shuffled(rr.band(2000, 40, 6, 3), 4),     # the workload of tools/bench_reorder.py
}
# a frontier wider than one trip of the breadth-first kernels over their grid, for 4, 16 and 64 lanes a vertex; the first two also
# hold more rows than one trip of the 16-lanes-a-row kernels (the adjacency, the permutation's keys, the bandwidth)
CASES.update({name: build for name, (build, _) in rr.GRID_LOOP_GRAPHS.items()})


@functools.lru_cache(maxsize=None)
def _case(name):
    A = CASES[name]()
    return A, rr.rcm_levelwise(*A[:3])


def _bytes_equal(got, want, what):
    for g, w, part in zip(got, want, ("row_ptr", "col", "val")):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), f"{what}: {part} differs"


@pytest.mark.parametrize("name", list(CASES))
def test_order_equals_the_twin_and_the_permuted_matrix_meets_the_bound(ctx, name):
    (n, rp, col, val), (order, inverse, counters, widths) = _case(name)
    if name in rr.GRID_LOOP_GRAPHS:  # the second trip is really taken: a changed generator or setting fails here
        lanes, widest, one_trip, one_trip_of_rows = rr.grid_loop_facts(n, rp, col, widths, counters["isolated"])
        print(f"{name}: n = {n}, {lanes} lanes a vertex, widest frontier {widest} > {one_trip}: {-(-widest // one_trip)} trips; "
              f"the row kernels loop beyond {one_trip_of_rows} rows: {-(-n // one_trip_of_rows)} trips")
        assert lanes == rr.GRID_LOOP_GRAPHS[name][1], f"{name} was built for {rr.GRID_LOOP_GRAPHS[name][1]} lanes a vertex"
        assert widest > one_trip, f"{name}: the breadth-first kernels make one trip over the grid: nothing of this case is left"
        later = rr.later_trip_children(n, rp, col, order, widths, one_trip)
        print(f"{name}: {later} vertices have their first parent beyond one trip: only the later trip can claim them")
        assert later > 0 or name == "random20000_deg40", f"{name}: the later trip has nothing to find"  # (hairy8300_deg38 is why)
    A = ctx.csr(n, n, rp, col, val)
    p = ctx.perm_rcm(A)
    got_order, got_inverse = p.download()
    assert np.array_equal(got_order, order), name
    assert np.array_equal(got_inverse, inverse), name
    assert p.info("n") == n
    for key, want in counters.items():
        assert p.info("rcm_" + key) == want, (name, key, p.info("rcm_" + key), want)
    if counters["components"]:
        assert p.info("rcm_launches") > 0 and p.info("rcm_transient_bytes") > 0
    again = ctx.perm_rcm(A)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again.download(), (got_order, got_inverse))), "two runs, equal bits"
    if name == "random300_one_sided":
        assert np.array_equal(order, _case("random300")[1][0]), "the order of the full pattern"
    # the bandwidth: spmv_csr_bandwidth is the twin's on A and on B, and B meets the bound of its level structures
    assert ctx.csr_bandwidth(A) == rr.bandwidth_profile(n, rp, col)
    B = ctx.csr_permute(A, p, p)
    B.validate()
    want_B = rr.permute_csr(n, n, rp, col, val, order, order)
    _bytes_equal(B.download(), want_B, name)
    bw, prof = ctx.csr_bandwidth(B)
    assert (bw, prof) == rr.bandwidth_profile(n, want_B[0], want_B[1])
    print(name, "bandwidth", ctx.csr_bandwidth(A)[0], "->", bw, "bound", rr.bandwidth_bound(widths), counters, "launches", p.info("rcm_launches"))
    assert bw <= rr.bandwidth_bound(widths), (name, bw, rr.bandwidth_bound(widths))


def test_a_permutation_made_by_hand_reports_n_alone(ctx):
    order = np.random.default_rng(1).permutation(777).astype(np.int32)
    p = ctx.perm(order)
    o, i = p.download()
    assert np.array_equal(o, order) and np.array_equal(i, rr.inverse_of(order)) and p.info("n") == 777
    for name in ("rcm_isolated", "rcm_components", "rcm_levels", "rcm_bfs", "rcm_launches", "rcm_transient_bytes"):
        assert p.info(name) == 0, name
    e = ctx.perm([])
    assert e.info("n") == 0 and e.download()[0].size == 0


def test_what_is_not_a_permutation_is_refused_with_its_position(ctx, pkg):
    good = np.random.default_rng(2).permutation(5000).astype(np.int32)
    repeat = good.copy()
    repeat[4321] = repeat[17]  # 4321 is the later of the two
    with pytest.raises(pkg.capi.SpmvError, match=r"position 4321\b") as e:
        ctx.perm(repeat)
    assert e.value.code == -1
    for value in (5000, -1):
        out = good.copy()
        out[[99, 4000]] = value
        with pytest.raises(pkg.capi.SpmvError, match=r"position 99\b") as e:
            ctx.perm(out)
        assert e.value.code == -1
    with pytest.raises(pkg.capi.SpmvError, match=r"position 1\b"):
        ctx.perm([0, 0])


def _unsorted_with_duplicates(m, n, per_row, seed):
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(m), per_row)
    c = rng.integers(0, n, m * per_row)  # (unsorted; per_row draws from n columns repeat some)
    keep = rng.random(m * per_row) < 0.8  # (rows of different lengths, some empty ones at m = 64)
    keep[:per_row] = False
    return rr.csr_from_entries(m, r[keep], c[keep], rng.standard_normal(int(keep.sum())))[1:]


@pytest.mark.parametrize("setting", ["rows_only", "columns_only", "both_on_a_rectangle", "duplicates_and_unsorted_columns"])
def test_permuted_handle_equals_the_twin_as_bytes(ctx, setting):
    m, n = (64, 48) if setting != "duplicates_and_unsorted_columns" else (50, 50)
    rng = np.random.default_rng(7)
    rp, col, val = _unsorted_with_duplicates(m, n, 12 if setting == "duplicates_and_unsorted_columns" else 5, 8)
    val[::7] = -0.0
    val[3] = np.float64(np.nan)
    if setting == "duplicates_and_unsorted_columns":
        r = np.repeat(np.arange(m), np.diff(rp))
        assert len(np.unique(r * n + col)) < len(col) and (np.diff(col)[np.diff(r) == 0] < 0).any()
    pr = rng.permutation(m).astype(np.int32) if setting != "columns_only" else None
    pc = rng.permutation(n).astype(np.int32) if setting != "rows_only" else None
    A = ctx.csr(m, n, rp, col, val)
    B = ctx.csr_permute(A, None if pr is None else ctx.perm(pr), None if pc is None else ctx.perm(pc))
    B.validate()
    assert (B.info.nrow, B.info.ncol, B.info.nnz) == (m, n, len(col))
    _bytes_equal(B.download(), rr.permute_csr(m, n, rp, col, val, pr, pc), setting)
    _bytes_equal(ctx.csr_permute(A).download(), rr.permute_csr(m, n, rp, col, val), "the identity orders the columns")


def test_permuting_by_the_inverse_returns_the_bytes(ctx):
    (n, rp, col, val), (order, inverse, _, _) = _case("grid37x23")  # rows sorted, no duplicates
    A = ctx.csr(n, n, rp, col, val)
    p, q = ctx.perm(order), ctx.perm(inverse)
    back = ctx.csr_permute(ctx.csr_permute(A, p, p), q, q)
    _bytes_equal(back.download(), (rp, col, val), "there and back")


@pytest.mark.parametrize("kernel", ["auto", "scalar"])
def test_the_renumbered_product_is_the_same_product_bit_for_bit(ctx, pkg, kernel):
    (n, rp, col, _), (order, _, _, _) = _case("band2000")
    entries_rows = np.repeat(np.arange(n), np.diff(rp))
    bits, e = exact.choose_bits(int(np.diff(rp).max()))
    rng = np.random.default_rng(12)
    val, x = exact.dyadic(rng, len(col), bits, e), exact.dyadic(rng, n, bits, e)
    want = exact.exact_product(n, entries_rows, col, val, x, e)  # A x in integers
    A = ctx.csr(n, n, rp, col, val)
    p = ctx.perm_rcm(A)
    assert np.array_equal(p.download()[0], order)
    B = ctx.csr_permute(A, p, p)
    if kernel == "scalar":
        A.set_kernel(pkg.capi.CSR_SCALAR)
        B.set_kernel(pkg.capi.CSR_SCALAR)
        assert B.info.kernel == pkg.capi.CSR_SCALAR
    dx, px, y, py, back = ctx.vector_from(x), ctx.vector(n), ctx.vector(n), ctx.vector(n), ctx.vector(n)
    y.fill(0.0)
    py.fill(0.0)
    ctx.apply(A, dx, y)
    ctx.vec_permute(p, dx, px)       # P x
    ctx.apply(B, px, py)             # B (P x)
    ctx.vec_permute(p, py, back, back=True)
    ctx.sync()
    assert y.download().tobytes() == want.tobytes(), "A x is the integer reference"
    assert py.download().tobytes() == want[order].tobytes(), "B (P x) = P (A x)"
    assert back.download().tobytes() == want.tobytes(), "and scattered back it is A x"


def test_the_permuted_handle_feeds_spgemm_and_cg(ctx, orc):
    import oracle_lib as ol

    # spgemm: (P A P^T)(P A P^T) = P (A A) P^T; the values are small integers, so every sum is exact in any order
    (n, rp, col, val), (order, _, _, _) = _case("grid37x23")
    A = ctx.csr(n, n, rp, col, val)
    p = ctx.perm(order)
    B = ctx.csr_permute(A, p, p)
    _bytes_equal(ctx.spgemm(B, B).download(), ctx.csr_permute(ctx.spgemm(A, A), p, p).download(), "the square of the permuted matrix")
    # cg: a 32 x 32 Laplacian, shuffled, then reordered; the tolerances of tests/test_gpu_solver.py for that system
    n, rp, col, val = rr.shuffled(rr.grid(32, 32), 21)
    A = ctx.csr(n, n, rp, col, val)
    p = ctx.perm_rcm(A)
    B = ctx.csr_permute(A, p, p)
    assert ctx.csr_bandwidth(B)[0] < ctx.csr_bandwidth(A)[0] // 8
    b_host = np.random.default_rng(2).uniform(-1, 1, n)
    b, pb, x, px, back = ctx.vector_from(b_host), ctx.vector(n), ctx.vector(n), ctx.vector(n), ctx.vector(n)
    tol = 1e-9
    x.fill(0.0)
    px.fill(0.0)
    _, relres = ctx.cg(A, b, x, max_iter=2000, rel_tol=tol)
    ctx.vec_permute(p, b, pb)
    _, relres_p = ctx.cg(B, pb, px, max_iter=2000, rel_tol=tol)
    ctx.vec_permute(p, px, back, back=True)
    ctx.sync()
    sol, sol_p = x.download(), back.download()
    ax = np.zeros(n)
    ol.csr_spmv(orc, rp, col, val, sol_p, ax)
    true_res = np.linalg.norm(b_host - ax) / np.linalg.norm(b_host)
    assert relres <= tol and relres_p <= tol and true_res <= 20 * tol, (relres, relres_p, true_res)
    # both iterates solve A x = b to 20 tol in the residual: they differ by at most 40 tol ||b|| / lambda_min, lambda_min(A) >= 8 sin^2(pi / 66)
    lam_min = 8.0 * np.sin(np.pi / 66.0) ** 2
    assert np.linalg.norm(sol - sol_p) <= 40 * tol * np.linalg.norm(b_host) / lam_min


def _with_odd_bits(n, seed):
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2**63, n, dtype=np.uint64)
    if n:
        bits[rng.integers(0, n, max(1, n // 50))] = np.uint64(0x7FF0000000000001) | rng.integers(0, 2**51, max(1, n // 50), dtype=np.uint64)  # NaNs, signalling ones too
        bits[rng.integers(0, n, max(1, n // 50))] = np.uint64(0x8000000000000000)  # -0.0
        bits[0] = np.uint64(0xFFF8DEADBEEF0001)
    return bits.view(np.float64)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4099, 1_050_627])
def test_vectors_travel_as_bits_in_both_directions(ctx, n):
    src = _with_odd_bits(n, n + 1)
    order = np.random.default_rng(n).permutation(n).astype(np.int32)
    p = ctx.perm(order)
    a, b, c = ctx.vector_from(src), ctx.vector(n), ctx.vector(n)
    if n:
        b.fill(1.0)
        c.fill(1.0)
    ctx.vec_permute(p, a, b)             # b[k] = a[order[k]]
    ctx.vec_permute(p, b, c, back=True)  # c[order[k]] = b[k]
    ctx.sync()
    assert b.download().tobytes() == src[order].tobytes(), "the gather is NumPy's indexing"
    assert c.download().tobytes() == src.tobytes(), "a gather followed by a scatter returns the bits"
    ctx.vec_permute(p, a, b, back=True)
    ctx.sync()
    want = np.empty(n)
    want[order] = src
    assert b.download().tobytes() == want.tobytes(), "the scatter is NumPy's indexed assignment"


def test_only_the_permutation_stays_on_the_device(ctx, pkg):
    n, rp, col, val = rr.random_graph(300_000, 900_000, 31)  # 8 n = 2.4 MB: visible in hipMemGetInfo
    A = ctx.csr(n, n, rp, col, val)
    bad = np.arange(n, dtype=np.int32)
    bad[-1] = 0

    def round_trip():
        p = ctx.perm_rcm(A)
        assert p.info("rcm_transient_bytes") > 40 * n
        B = ctx.csr_permute(A, p, p)
        del p, B
        with pytest.raises(pkg.capi.SpmvError, match="position"):
            ctx.perm(bad)
        ctx.sync()

    round_trip()  # (what the context itself keeps grows on first use)
    before = ctx.mem_info()[0]
    by_hand = ctx.perm(np.arange(n, dtype=np.int32))
    held_by_hand = before - ctx.mem_info()[0]  # two arrays of 4 n bytes, as the allocator rounds them
    del by_hand
    assert ctx.mem_info()[0] == before
    p = ctx.perm_rcm(A)
    held = before - ctx.mem_info()[0]
    assert held == held_by_hand and 8 * n <= held <= 8 * n + (4 << 20), (held, held_by_hand, 8 * n)
    with pytest.raises(pkg.capi.SpmvError, match="position"):
        ctx.perm(bad)
    assert before - ctx.mem_info()[0] == held, "a refused call leaves nothing"
    del p
    assert ctx.mem_info()[0] == before, "spmv_perm_destroy returns the 8 n bytes"
    round_trip()
    assert ctx.mem_info()[0] == before
