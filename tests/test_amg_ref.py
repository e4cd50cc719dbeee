"""The NumPy twin of aggregation AMG (tests/amg_ref.py) held to facts of its own, on the CPU: the aggregates partition the rows and
their roots keep their distance, the coarse operator is the Galerkin product, the cycle is a symmetric positive definite operator
that contracts the error in the energy norm, strength keeps aggregates inside the strong direction, the preconditioned counts fall
as the prototype's did, and three mutations of the method are each noticed."""
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
