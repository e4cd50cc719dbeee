"""The NumPy twin of aggregation AMG (tests/amg_ref.py) held to facts of its own, on the CPU: the aggregates partition the rows and
their roots keep their distance, the coarse operator is the Galerkin product, the cycle is a symmetric positive definite operator
that contracts the error in the energy norm, strength keeps aggregates inside the strong direction, the preconditioned counts fall
as the prototype's did, and three mutations of the method are each noticed.  Further down: the generators of
tests/test_gpu_amg_edges.py (the periodic tridiagonal matrix whose level 1 no LDS window holds, the fuzz systems), their coarse
operators against P^T A P in int64, and five mutations against the gate of that GPU test on every case it applies."""
import numpy as np
import pytest

import amg_ref as ar
import chebyshev_ref as cr
import exact
import ilu0_ref as ir

OMEGAS = (1.0, 1.5, 1.9)
SMALL = {"laplacian12x12": lambda: cr.laplacian_2d_csr(12), "laplacian6^3": lambda: ir.laplacian_3d(6)}
PATTERNS = {"laplacian32x32": lambda: cr.laplacian_2d_csr(32), "laplacian8^3": lambda: ir.laplacian_3d(8), "arrow300": lambda: ar.arrow(300),
            "nonsymmetric500": lambda: ar.random_nonsymmetric(500), "convdiff40": lambda: ir.convection_diffusion_2d(40)}
SYMMETRIC = ("laplacian32x32", "laplacian8^3", "arrow300")


def _fmix32(h):  # the finaliser once more, on Python integers
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def test_the_hash_and_the_priorities():
    ids = list(range(300)) + [2**20 + 3, 2**31 - 1]
    assert [int(v) for v in ar.hash32(np.array(ids, dtype=np.uint64))] == [_fmix32(i) for i in ids]
    assert _fmix32(0) == 0 and _fmix32(1) == 0x514E28B7
    p = ar.priorities(1000)
    assert p.dtype == np.uint64 and len(set(p.tolist())) == 1000 and int(p.min()) >= 1, "0 stays below every priority"
    assert [int(v) for v in p[:3]] == [(_fmix32(i) << 32 | i) + 1 for i in range(3)]


@pytest.mark.parametrize("name", list(PATTERNS))
def test_every_row_is_in_exactly_one_aggregate(name):
    n, rp, cc, cv = PATTERNS[name]()
    agg, nc, rounds, roots = ar.aggregate(n, rp, cc, cv)
    sizes = np.bincount(agg, minlength=nc)
    print(f"{name}: {nc} aggregates of {n} rows in {rounds} rounds, sizes {sizes.min()} .. {sizes.max()} (mean {sizes.mean():.2f})")
    assert agg.shape == (n,) and agg.min() == 0 and agg.max() == nc - 1 and np.all(sizes >= 1)
    assert len(roots) == nc and np.array_equal(agg[roots], np.arange(nc)), "roots take their ids in ascending row order"
    assert 1 <= rounds <= 12


@pytest.mark.parametrize("name", SYMMETRIC)
def test_no_two_roots_are_within_two_hops_on_symmetric_patterns(name):
    n, rp, cc, cv = PATTERNS[name]()
    roots = ar.aggregate(n, rp, cc, cv)[3]
    adj = ar.dense_of(n, rp, cc, np.ones(len(cc))) != 0
    np.fill_diagonal(adj, False)
    near = adj | ((adj.astype(np.int32) @ adj.astype(np.int32)) > 0)
    np.fill_diagonal(near, False)
    assert not near[np.ix_(roots, roots)].any()
    # and every other row has a root within two hops: the set is maximal
    others = np.setdiff1d(np.arange(n), roots)
    assert near[np.ix_(others, roots)].any(axis=1).all()


@pytest.mark.parametrize("name", ("laplacian32x32", "nonsymmetric500"))
def test_coarse_row_sums_are_the_aggregated_fine_row_sums_exactly(name):
    n, rp, cc, _ = PATTERNS[name]()
    bits, e = exact.choose_bits(4096)
    cv = exact.dyadic(np.random.default_rng(17), len(cc), bits, e)
    agg, nc, _, _ = ar.aggregate(n, rp, cc, cv)
    rp_c, cc_c, cv_c = ar.coarse_operator(n, rp, cc, cv, agg, nc)
    rows = np.repeat(np.arange(n), np.diff(rp))
    fine = np.zeros(nc, dtype=np.int64)
    np.add.at(fine, agg[rows], exact.scaled(cv, e))
    coarse = np.zeros(nc, dtype=np.int64)
    np.add.at(coarse, np.repeat(np.arange(nc), np.diff(rp_c)), exact.scaled(cv_c, e))
    assert np.array_equal(fine, coarse)
    assert all(np.all(np.diff(cc_c[rp_c[i]:rp_c[i + 1]]) > 0) for i in range(nc)), "columns ascend within a coarse row"


def test_the_coarse_operator_is_the_galerkin_product():
    n, rp, cc, cv = cr.laplacian_2d_csr(12)
    H = ar.Hierarchy(n, rp, cc, cv, coarse_max=8)
    assert len(H.levels) >= 3
    for l in range(len(H.levels) - 1):
        L, C = H.levels[l], H.levels[l + 1]
        P = H.prolongator(l)
        assert np.array_equal(ar.dense_of(C.n, C.rp, C.cc, C.cv), P.T @ ar.dense_of(L.n, L.rp, L.cc, L.cv) @ P)  # (integers: exact)


def test_the_dense_inverse():
    n, rp, cc, cv = ir.convection_diffusion_2d(12)
    inv = ar.dense_inverse(n, rp, cc, cv)
    assert np.max(np.abs(inv @ ar.dense_of(n, rp, cc, cv) - np.eye(n))) <= 1e-13
    n, rp, cc, cv = cr.tridiagonal(40)
    cv = cv.copy()
    cv[0] = cv[-1] = 1.0  # rows sum to zero: singular
    with pytest.raises(ValueError, match="singular coarsest operator"):
        ar.dense_inverse(n, rp, cc, cv)


@pytest.mark.parametrize("omega", OMEGAS)
@pytest.mark.parametrize("name", list(SMALL))
def test_the_cycle_is_symmetric_positive_definite(name, omega):
    n, rp, cc, cv = SMALL[name]()
    H = ar.Hierarchy(n, rp, cc, cv, coarse_max=8, overcorrection=omega)
    assert len(H.levels) >= 2
    B = H.dense_operator()
    asym = np.max(np.abs(B - B.T)) / np.max(np.abs(B))
    lo = np.linalg.eigvalsh(0.5 * (B + B.T)).min()
    print(f"{name} omega {omega}: rows {H.rows}, asymmetry {asym:.2e}, smallest eigenvalue {lo:.3e}")
    assert asym <= 1e-13 and lo > 0.0


@pytest.mark.parametrize("omega", OMEGAS)
@pytest.mark.parametrize("name", list(SMALL))
def test_the_two_level_error_propagator_contracts_in_the_energy_norm(name, omega):
    n, rp, cc, cv = SMALL[name]()
    H = ar.Hierarchy(n, rp, cc, cv, max_levels=2, coarse_max=8, overcorrection=omega)
    assert len(H.levels) == 2
    A = ar.dense_of(n, rp, cc, cv)
    w, V = np.linalg.eigh(A)
    half, inv_half = (V * np.sqrt(w)) @ V.T, (V / np.sqrt(w)) @ V.T
    E = np.eye(n) - H.dense_operator() @ A
    norm = np.linalg.norm(half @ E @ inv_half, 2)
    print(f"{name} omega {omega}: ||I - B A||_A = {norm:.4f}")
    assert norm < 1.0


def test_strength_keeps_aggregates_inside_a_grid_line():
    m = 16
    n, rp, cc, cv = ar.anisotropic_2d(m)  # x coupling 1, y coupling 0.01, row i = y * m + x
    for theta, grouped in ((0.5, False), (0.25, True)):  # 1 < 0.5^2 2.02^2: nothing is strong; 1 >= 0.25^2 2.02^2 > 0.01^2: the x couplings are
        agg, nc, _, _ = ar.aggregate(n, rp, cc, cv, theta)
        lines = [set((np.flatnonzero(agg == I) // m).tolist()) for I in range(nc)]
        assert all(len(s) == 1 for s in lines), theta
        assert (nc < n) == grouped
    agg, nc, _, _ = ar.aggregate(n, rp, cc, cv, 0.0)
    assert any(len(set((np.flatnonzero(agg == I) // m).tolist())) > 1 for I in range(nc)), "without strength aggregates cross the lines"


def test_preconditioned_cg_takes_a_third_of_the_iterations_at_most():
    plain = ar.run_twin("cg_laplacian64", amg=False)[1]
    for omega in (1.0, 1.5):
        iters = ar.run_twin("cg_laplacian64", overcorrection=omega)[1]
        print(f"64 x 64, omega {omega}: {iters} iterations against {plain}")
        assert 3 * iters <= plain


@pytest.mark.parametrize("system", list(ar.SYSTEMS))
def test_iteration_counts_of_the_twins(system):
    assert ar.run_twin(system)[1] == ar.TWIN_ITERATIONS[system]
    assert ar.run_twin(system, amg=False)[1] == ar.UNPRECONDITIONED_ITERATIONS[system]


def test_the_overcorrection_table():
    """the figures of DESIGN.md 18: CG to 1e-8 with b = default_rng(1).uniform(-1, 1), plain and under the default hierarchy"""
    table = {"64x64": (lambda: cr.laplacian_2d_csr(64), (193, 23, 19, 19)), "24^3": (lambda: ir.laplacian_3d(24), (93, 14, 13, 14))}
    for name, (build, want) in table.items():
        n, rp, cc, cv = build()
        b = np.random.default_rng(1).uniform(-1, 1, n)
        mv = lambda x: ir.csr_mv(n, rp, cc, cv, x)
        got = [ir.run_cg(mv, lambda r: r.copy(), b, 1e-8, 5000)[1]]
        got += [ir.run_cg(mv, ar.Hierarchy(n, rp, cc, cv, overcorrection=omega).apply, b, 1e-8, 500)[1] for omega in (1.0, 1.5, 1.6)]
        assert tuple(got) == want, (name, got)


# ---- mutations: each changes the aggregates or breaks a property above ---------------------------------------------------------------
def test_mutation_of_the_tie_rule_changes_the_aggregates():
    """where the row lists are not symmetric a row can see two roots (on a symmetric pattern roots are more than two hops apart,
    and pass 1 never meets a tie: the assertion below says so)"""
    n, rp, cc, cv = ar.random_nonsymmetric(500)
    assert not np.array_equal(ar.aggregate(n, rp, cc, cv)[0], ar.aggregate(n, rp, cc, cv, mutate="tie")[0])
    n, rp, cc, cv = cr.laplacian_2d_csr(32)
    assert np.array_equal(ar.aggregate(n, rp, cc, cv)[0], ar.aggregate(n, rp, cc, cv, mutate="tie")[0])


def test_mutation_to_a_sum_over_strong_entries_breaks_the_galerkin_product():
    n, rp, cc, cv = ar.anisotropic_2d(16)
    agg, nc, _, _ = ar.aggregate(n, rp, cc, cv, 0.25)
    P = np.zeros((n, nc))
    P[np.arange(n), agg] = 1.0
    galerkin = P.T @ ar.dense_of(n, rp, cc, cv) @ P
    right = ar.coarse_operator(n, rp, cc, cv, agg, nc, 0.25)
    wrong = ar.coarse_operator(n, rp, cc, cv, agg, nc, 0.25, mutate="strong_sum")
    assert np.max(np.abs(ar.dense_of(nc, *right) - galerkin)) <= 1e-14
    assert np.max(np.abs(ar.dense_of(nc, *wrong) - galerkin)) >= 0.009  # (the y couplings are gone)


def test_mutation_of_the_post_smoother_breaks_symmetry():
    n, rp, cc, cv = cr.laplacian_2d_csr(12)
    B = ar.Hierarchy(n, rp, cc, cv, coarse_max=8, mutate="post_degree").dense_operator()
    assert np.max(np.abs(B - B.T)) / np.max(np.abs(B)) >= 1e-4


# ---- the generators of tests/test_gpu_amg_edges.py ------------------------------------------------------------------------------------
WINDOW_ROWS, WINDOW_CAPACITY = 256, 16384  # kWinRows and kWinDoubles of csrc/kernels_csr.hip: the LDS-window kernel's block and tile


def _widest_window(n, rp, cc):
    """the widest span of columns, last - first + 1, over the blocks of 256 rows"""
    spans = [int(cc[rp[i]:rp[min(i + WINDOW_ROWS, n)]].max()) - int(cc[rp[i]:rp[min(i + WINDOW_ROWS, n)]].min()) + 1
             for i in range(0, n, WINDOW_ROWS) if rp[min(i + WINDOW_ROWS, n)] > rp[i]]
    return max(spans)


def test_the_periodic_tridiagonal_matrix():
    n, rp, cc, cv = ar.periodic_tridiagonal(7)
    want = 2.5 * np.eye(7) - np.roll(np.eye(7), 1, axis=1) - np.roll(np.eye(7), -1, axis=1)
    assert np.array_equal(ar.dense_of(n, rp, cc, cv), want) and list(cc[:6]) == [0, 1, 6, 0, 1, 2] and len(cc) == 21
    n, rp, cc, cv = ar.periodic_tridiagonal(ar.PERIODIC)
    assert np.array_equal(np.diff(rp), np.full(n, 3)) and np.all(np.diff(cc.reshape(n, 3), axis=1) > 0), "columns ascend"


def test_the_reproducers_level_1_is_wider_than_the_lds_window_and_level_2_is_not():
    """what makes a forced LDS-window kernel fail on level 1 alone: a block of 256 rows there spans every column"""
    H = ar.Hierarchy(*ar.periodic_tridiagonal(ar.PERIODIC))
    assert H.rows == [100000, 27529, 7601, 2091, 574, 154]
    spans = [_widest_window(L.n, L.rp, L.cc) for L in H.levels]
    print("widest windows:", spans)
    assert spans[1] == 27529 > WINDOW_CAPACITY and all(s <= WINDOW_CAPACITY for s in spans[2:])


@pytest.mark.parametrize("seed", ar.FUZZ_SEEDS)
def test_the_fuzz_systems_are_what_they_say(seed):
    n, rp, cc, cv = ar.fuzz_system(seed)
    assert n in ar.FUZZ_SIZES and len(rp) == n + 1 and rp[0] == 0 and rp[-1] == len(cc) == len(cv) and cc.dtype == np.int32
    assert np.array_equal(ar.fuzz_system(seed)[3], cv), "the same system on every call"
    iv = exact.scaled(cv, ar.FUZZ_E)
    for i in range(n):
        c, v, f = cc[rp[i]:rp[i + 1]], iv[rp[i]:rp[i + 1]], cv[rp[i]:rp[i + 1]]
        off = c != i
        assert len(set(c[off].tolist())) <= min(6, n - 1) and c.min() >= 0 and c.max() < n
        assert all(count <= 2 for count in np.bincount(c[off], minlength=1)), "an off-diagonal entry is stored twice at most"
        odd = np.abs(v[off & (v != 0)])
        odd = odd // (odd & -odd)  # the mantissa: at most 10 bits, and the exponent within -10 .. 0
        assert np.all(odd < 2**10) and np.all(np.abs(f[off]) < 2**10)
        assert 1 <= int((~off).sum()) <= 2 and v[~off].sum() > np.abs(v[off]).sum(), "a positive, strictly dominant diagonal"
    ar.Hierarchy(n, rp, cc, cv, **ar.fuzz_setup(seed))  # the twin raises on none of them: no zero diagonal, no singular operator


def test_the_fuzz_systems_cover_what_csr_allows():
    sizes, setups = set(), set()
    entries = doubled = zeros = rows = split = unsorted = 0
    for seed in ar.FUZZ_SEEDS:
        n, rp, cc, cv = ar.fuzz_system(seed)
        sizes.add(n)
        setups.add(tuple(ar.fuzz_setup(seed).values()))
        r = np.repeat(np.arange(n), np.diff(rp))
        off = r != cc
        pairs = r[off].astype(np.int64) * n + cc[off]
        entries += len(set(pairs.tolist()))
        doubled += len(pairs) - len(set(pairs.tolist()))
        zeros += int((cv[off] == 0.0).sum())
        rows += n
        split += int((~off).sum()) - n
        unsorted += sum(bool(np.any(np.diff(cc[rp[i]:rp[i + 1]]) < 0)) for i in range(n))
        if n >= 17:
            pattern = ar.dense_of(n, rp, cc, np.ones(len(cc))) != 0
            assert not np.array_equal(pattern, pattern.T), "a structurally nonsymmetric pattern"
    print(f"{entries} off-diagonal positions, {doubled} stored twice, {zeros} stored zeros; {rows} rows, {split} with a split diagonal, {unsorted} unsorted")
    assert sizes == set(ar.FUZZ_SIZES) and {s[0] for s in setups} == {0.0, 0.1, 0.5} and {s[1] for s in setups} == {1, 8, 256}
    assert 0.12 <= doubled / entries <= 0.18 and 0.07 <= zeros / entries <= 0.13 and 0.45 <= split / rows <= 0.55 and unsorted >= rows // 2


# ---- the Galerkin product in integers --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ar.FUZZ_SEEDS)
def test_fuzz_coarse_operators_are_the_galerkin_products_in_integers(seed):
    """every coarse value is P^T A P computed in int64 by a scatter that knows nothing of the twin's ordering, the stored pattern
    is the pattern of the products, and the sum of all stored entries - 1^T A 1, which P^T . P keeps - is one integer on every
    level"""
    n, rp, cc, cv = ar.fuzz_system(seed)
    H = ar.Hierarchy(n, rp, cc, cv, **ar.fuzz_setup(seed))
    total = int(exact.scaled(cv, ar.FUZZ_E).sum())
    for l in range(len(H.levels) - 1):
        L, C = H.levels[l], H.levels[l + 1]
        want, stored = ar.galerkin_int64(L.n, L.rp, L.cc, L.cv, L.agg, L.nc)
        rows = np.repeat(np.arange(C.n), np.diff(C.rp))
        got = np.zeros((C.n, C.n), dtype=np.int64)
        got[rows, C.cc] = exact.scaled(C.cv, ar.FUZZ_E)
        held = np.zeros((C.n, C.n), dtype=bool)
        held[rows, C.cc] = True
        assert len(set(zip(rows.tolist(), C.cc.tolist()))) == C.nnz, "a coarse entry is stored once"
        assert np.array_equal(got, want) and np.array_equal(held, stored), (seed, l)
        assert int(exact.scaled(C.cv, ar.FUZZ_E).sum()) == total, (seed, l)
        d = ar.diagonal_of(C.n, C.rp, C.cc, C.cv)
        assert np.all(d > 0) and np.all(2 * d > np.bincount(rows, weights=np.abs(C.cv), minlength=C.n)), "row dominance survives"


def test_the_level_0_smoother_can_be_replaced():
    n, rp, cc, cv = cr.laplacian_2d_csr(12)
    H = ar.Hierarchy(n, rp, cc, cv, coarse_max=8)
    lmin, lmax = cr.laplacian_2d_bounds(12)
    G = ar.Hierarchy(n, rp, cc, cv, coarse_max=8, level0_smoother=(3, False, lmin, lmax))
    assert G.rows == H.rows and G.launches() == H.launches() + 4
    same = ar.Hierarchy(n, rp, cc, cv, coarse_max=8, level0_smoother=(2, True, 2.0 / 30.0, 2.0))  # (the default set-up, spelled out)
    r = np.random.default_rng(3).uniform(-1, 1, n)
    assert same.apply(r).tobytes() == H.apply(r).tobytes() and G.apply(r).tobytes() != H.apply(r).tobytes()
    # levels 1 and below keep their smoothers: the two differ by level 0's polynomial alone
    assert all(a.cheby()[1] == b.cheby()[1] for a, b in zip(G.levels[1:], H.levels[1:]))
    B = G.dense_operator()
    assert np.max(np.abs(B - B.T)) / np.max(np.abs(B)) <= 1e-13 and np.linalg.eigvalsh(0.5 * (B + B.T)).min() > 0.0


# ---- sensitivity: what the gate of tests/test_gpu_amg_edges.py would notice ------------------------------------------------------------
_ONE_LEVEL = "one level: nothing is aggregated, restricted or prolonged, and no smoother follows a correction"
_SYMMETRIC = "a symmetric pattern: roots are more than two hops apart, no row sees two of them"
_ONE_ROOT = "one aggregate: there is one root to join"
_ALL_STRONG = "theta = 0: every stored off-diagonal entry is strong"
# (mutation, case): why the mutation cannot change the case.  Held below: the mutated twin returns the unmutated twin's bytes.
EXEMPT = {(m, case): _ONE_LEVEL for m in ar.MUTATIONS
          for case in ("anisotropic16x16", "anisotropic16x16_degree1", "diagonal257", "diagonal257_degree1", "fuzz00", "fuzz05", "fuzz09",
                       "fuzz10", "fuzz13", "fuzz21", "tridiagonal1024", "tridiagonal1025")}
EXEMPT.update({("tie", case): _SYMMETRIC for case in ("arrow300", "arrow300_degree1", "anisotropic16x16_quarter", "anisotropic16x16_quarter_degree1",
                                                      "tridiagonal257", "tridiagonal257_degree1", "laplacian32x32", "laplacian32x32_unscaled3",
                                                      "periodic100000")})
EXEMPT.update({("tie", case): _ONE_ROOT for case in ("fuzz03", "fuzz19")})
EXEMPT.update({("strong_sum", case): _ALL_STRONG for case in ("arrow300", "arrow300_degree1", "nonsymmetric500", "nonsymmetric500_degree1",
                                                              "tridiagonal257", "tridiagonal257_degree1", "laplacian32x32", "laplacian32x32_unscaled3",
                                                              "periodic100000", "fuzz03", "fuzz06", "fuzz12", "fuzz15", "fuzz18")})
EXEMPT[("strong_sum", "fuzz19")] = "two rows: the one weak entry is a stored zero"


@pytest.mark.parametrize("name", list(ar.EDGE_CASES))
def test_every_mutation_moves_every_application(name):
    """each of the five mutations moves Hierarchy.apply away from the unmutated twin by more than the gate the GPU test holds the
    engine to (oracle_lib.REL_TOL x max |want|), on every case that test applies - or is listed in EXEMPT with its reason"""
    import copy

    import oracle_lib as ol

    build, kw = ar.EDGE_CASES[name]
    if kw.get("max_levels") == 1:  # (one level by its arguments: the inverse of 1024 rows need not be built to know)
        assert all(EXEMPT[m, name] == _ONE_LEVEL for m in ar.MUTATIONS)
        return
    n, rp, cc, cv = build()
    H = ar.Hierarchy(n, rp, cc, cv, **kw)
    r = ar.edge_rhs(name, n)
    want = H.apply(r)
    gate = ol.REL_TOL * np.max(np.abs(want))
    for m in ar.MUTATIONS:
        if m in ("tie", "strong_sum"):  # these change the hierarchy
            M = ar.Hierarchy(n, rp, cc, cv, mutate=m, **kw)
        else:  # these the cycle alone
            M = copy.copy(H)
            M.mutate = m
        got = M.apply(r)
        moved = float(np.max(np.abs(got - want)))
        if (m, name) in EXEMPT:
            assert got.tobytes() == want.tobytes(), (m, name, "is listed as exempt and moved", moved)
            if EXEMPT[m, name] == _ONE_LEVEL:
                assert len(H.levels) == 1
            continue
        print(f"{name}, {m}: moved by {moved / np.max(np.abs(want)):.3e} of max |want|")
        assert moved > gate, (m, name, moved, gate)


def test_every_mutation_is_caught_by_some_case():
    """(the test above holds every pair that is not exempt to the gate)"""
    assert set(case for _, case in EXEMPT) <= set(ar.EDGE_CASES) and set(m for m, _ in EXEMPT) <= set(ar.MUTATIONS)
    for m in ar.MUTATIONS:
        caught = [case for case in ar.EDGE_CASES if (m, case) not in EXEMPT]
        print(f"{m}: caught by {len(caught)} of {len(ar.EDGE_CASES)} cases")
        assert caught
