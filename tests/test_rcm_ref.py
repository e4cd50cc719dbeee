"""The NumPy twin of the reverse Cuthill-McKee ordering (tests/rcm_ref.py) against itself: the level-wise rule that the device runs is
the textbook queue algorithm, the result is a permutation that meets the bound of a level-structure numbering, and what the graph
ignores changes nothing.  No GPU."""
import numpy as np
import pytest

import rcm_ref as rr

FAMILIES = {
    "path": lambda: rr.shuffled(rr.path(257), 1),
    "grid": lambda: rr.shuffled(rr.grid(37, 23), 2),
    "grid3d": lambda: rr.grid(9, 9, 9),
    "band": lambda: rr.shuffled(rr.band(2000, 40, 6, 3), 4),
    "star": lambda: rr.shuffled(rr.star(500), 5),
    "complete": lambda: rr.complete(70),
    "random_connected": lambda: rr.shuffled(rr.random_graph(2000, 8000, 6), 7),
    "random_components": lambda: rr.shuffled(rr.random_graph(300, 200, 8), 9),
    "empty": lambda: rr.from_edges(0, [], []),
    "one": lambda: rr.from_edges(1, [], []),
    "no_edges": lambda: rr.from_edges(5, [], []),
}


@pytest.mark.parametrize("name", list(FAMILIES))
def test_queue_and_level_wise_sequences_are_equal_and_meet_the_bound(name):
    n, rp, col, val = FAMILIES[name]()
    order, inverse, counters, widths = rr.rcm_levelwise(n, rp, col)
    q_order, q_inverse, q_counters, q_widths = rr.rcm_queue(n, rp, col)
    assert np.array_equal(order, q_order) and np.array_equal(inverse, q_inverse)
    assert counters == q_counters and widths == q_widths
    assert np.array_equal(np.sort(order), np.arange(n)) and np.array_equal(order[inverse], np.arange(n))
    assert counters["isolated"] + sum(sum(w) for w in widths) == n
    assert counters["components"] == len(widths) and counters["levels"] == sum(len(w) for w in widths)
    assert 2 * counters["components"] + counters["components"] <= counters["bfs"] <= (rr.root_repeats() + 2) * counters["components"]
    B = rr.permute_csr(n, n, rp, col, val, order, order)
    bw, _ = rr.bandwidth_profile(n, B[0], B[1])
    assert bw <= rr.bandwidth_bound(widths), (name, bw, rr.bandwidth_bound(widths))
    print(name, "bandwidth", rr.bandwidth_profile(n, rp, col)[0], "->", bw, "bound", rr.bandwidth_bound(widths), counters)


def test_the_random_families_are_what_their_names_say():
    n, rp, col, _ = FAMILIES["random_connected"]()
    c = rr.rcm_levelwise(n, rp, col)[2]
    assert c["components"] == 1 and c["isolated"] == 1, c  # (connected, one vertex without an edge apart)
    n, rp, col, _ = FAMILIES["random_components"]()
    c = rr.rcm_levelwise(n, rp, col)[2]
    assert c["components"] == 24 and c["isolated"] == 82, c


@pytest.mark.parametrize("name", list(rr.GRID_LOOP_GRAPHS))
def test_the_grid_loop_graphs_reach_a_second_trip(name):
    """the coverage conditions of the wide-frontier cases of tests/test_gpu_reorder.py, without a GPU: the lanes a vertex that the
    mean degree selects, a frontier wider than one trip of those lanes over the grid, vertices that only the later trip can claim,
    and - all together - every lane count and more rows than one trip of the 16-lanes-a-row kernels"""
    build, want_lanes = rr.GRID_LOOP_GRAPHS[name]
    n, rp, col, val = build()
    order, _, counters, widths = rr.rcm_levelwise(n, rp, col)
    lanes, widest, one_trip, one_trip_of_rows = rr.grid_loop_facts(n, rp, col, widths, counters["isolated"])
    print(f"{name}: n = {n}, {len(col)} entries, {counters}, widths {widths[0] if len(widths) == 1 else len(widths)}, {lanes} lanes, "
          f"widest {widest} against {one_trip}, rows against {one_trip_of_rows}")
    assert lanes == want_lanes and widest > one_trip and counters["components"] == 1
    assert (n > one_trip_of_rows) == (name in ("broom131200", "random100000_deg10"))
    assert np.array_equal(np.sort(order), np.arange(n))
    assert sorted({l for _, l in rr.GRID_LOOP_GRAPHS.values()}) == [4, 16, 64]
    # what only a later trip can find: the vertices whose first parent stands beyond one trip in its frontier.  random20000_deg40
    # has none - about 29 parents a vertex, the first of them early - which is why hairy8300_deg38 stands beside it
    later = rr.later_trip_children(n, rp, col, order, widths, one_trip)
    print(f"{name}: {later} vertices are claimed on a later trip")
    assert later == {"broom131200": 254, "random100000_deg10": 1019, "random20000_deg40": 0, "hairy8300_deg38": 107}[name]
    if name == "hairy8300_deg38":  # a leaf, its parent, the root and the parent's siblings, the other children and the siblings' leaves, leaves
        assert widths[0][:2] == [1, 1] and widths[0][3] == 8299
    if name == "broom131200":  # a leaf, its parent, the root and the leaf's sibling, the other children, their leaves
        assert widths[0][:4] == [1, 1, 2, 131_199] and rr.bandwidth_profile(n, rp, col)[0] > n // 2
    if name == "random100000_deg10":
        assert widths == [[1, 1, 11, 120, 1227, 11394, 59115, 28065, 65]] and counters["isolated"] == 1
    if name == "random20000_deg40":
        assert widths == [[1, 19, 714, 14626, 4640]]


def test_a_shuffled_path_comes_back_with_bandwidth_one():
    n, rp, col, val = rr.shuffled(rr.path(1025), 11)
    assert rr.bandwidth_profile(n, rp, col)[0] > 100
    order, _, counters, widths = rr.rcm_levelwise(n, rp, col)
    B = rr.permute_csr(n, n, rp, col, val, order, order)
    assert rr.bandwidth_profile(n, B[0], B[1]) == (1, n - 1)
    assert widths == [[1] * n] and counters["levels"] == n and counters["components"] == 1


def test_one_sided_storage_duplicates_stored_zeros_and_self_loops_change_nothing():
    full = rr.shuffled(rr.random_graph(300, 200, 8), 9)
    noisy = rr.one_sided_noisy(full, 10)
    assert noisy[2].size != full[2].size and (noisy[3] == 0.0).any()
    r = np.repeat(np.arange(noisy[0]), np.diff(noisy[1]))
    assert not (r > noisy[2]).any(), "nothing below the diagonal is stored"
    a, b = rr.rcm_levelwise(*full[:3]), rr.rcm_levelwise(*noisy[:3])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]
    bare = rr.from_edges(full[0], r[r < noisy[2]], noisy[2][r < noisy[2]], diagonal=False)  # (and without any diagonal)
    assert np.array_equal(rr.rcm_levelwise(*bare[:3])[0], a[0])


def test_permute_csr_keeps_duplicates_in_stored_order_and_takes_rectangles():
    rng = np.random.default_rng(3)
    m, n = 5, 4
    rp = np.array([0, 3, 3, 5, 6, 9], dtype=np.int32)
    col = np.array([2, 0, 2, 3, 3, 1, 0, 3, 0], dtype=np.int32)
    val = np.arange(1.0, 10.0)
    pr, pc = rng.permutation(m), rng.permutation(n)
    b_rp, b_col, b_val = rr.permute_csr(m, n, rp, col, val, pr, pc)
    dense = lambda r, c, v: [[[float(v[e]) for e in range(r[i], r[i + 1]) if c[e] == j] for j in range(n)] for i in range(m)]
    A, B = dense(rp, col, val), dense(b_rp, b_col, b_val)
    for k in range(m):
        assert all(b_col[e] <= b_col[e + 1] for e in range(b_rp[k], b_rp[k + 1] - 1))
        for l in range(n):
            assert B[k][l] == A[pr[k]][pc[l]]
    ident = rr.permute_csr(m, n, rp, col, val)
    assert list(ident[1][:3]) == [0, 2, 2] and list(ident[2][:3]) == [2.0, 1.0, 3.0]


def test_bandwidth_and_profile():
    rp = np.array([0, 2, 2, 4, 5], dtype=np.int32)
    col = np.array([0, 3, 0, 2, 3], dtype=np.int32)
    assert rr.bandwidth_profile(4, rp, col) == (3, 2)
    assert rr.bandwidth_profile(3, np.zeros(4, np.int32), np.zeros(0, np.int32)) == (0, 0)
