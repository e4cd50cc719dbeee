"""The NumPy twin of smoothed-aggregation AMG (tests/amg_sa_ref.py) held to facts of its own on the CPU: R = P^T and A_c = P^T A P
densely, the partition of unity on rows whose filtered row sum is zero, the filter's exact row sums, the symmetry and definiteness of
B, the two-level error propagator, an int64 reference on the family where 8 P and 64 A_c are integers, the iteration table, and
five mutations of the definition, each of which must move every application the GPU tests compare - or be listed with the reason
why it cannot."""
import numpy as np
import pytest

import amg_ref as ar
import amg_sa_ref as sa
import chebyshev_ref as cr
import ilu0_ref as ir
import oracle_lib as ol

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _case(name, **extra):
    system = _once(("system", name), sa.CASES[name][0])
    kw = dict(sa.CASES[name][1], **extra)
    return system, _once(("twin", name, tuple(sorted(kw.items()))), lambda: sa.Hierarchy(*system, **kw))


DENSE_CASES = ("tridiagonal257", "laplacian32x32", "laplacian12^3", "convdiff40", "nonsymmetric500", "anisotropic16x16_quarter", "fuzz04", "fuzz22",
               "arrow65")


# ---- 1. the transfer operators ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DENSE_CASES)
def test_restriction_is_the_transpose_and_the_coarse_operator_is_galerkin(name):
    _, H = _case(name)
    assert len(H.levels) > 1
    for l, L in enumerate(H.levels[:-1]):
        N = H.levels[l + 1]
        P, R = sa.dense_rect(L.n, L.nc, *L.P), sa.dense_rect(L.nc, L.n, *L.R)
        assert np.array_equal(R, P.T), (name, l)
        assert np.all(np.diff(L.P[0]) >= 1) and all(np.all(np.diff(L.P[1][a:b]) > 0) for a, b in zip(L.P[0][:-1], L.P[0][1:])), "P: ascending columns"
        assert L.P[1].max() < L.nc and np.all(sa.dense_rect(L.n, L.nc, L.P[0], L.P[1], np.ones(len(L.P[1])))[np.arange(L.n), L.agg] == 1.0), \
            "every row of P holds the column of its own aggregate"
        want = P.T @ ar.dense_of(L.n, L.rp, L.cc, L.cv) @ P
        got = ar.dense_of(N.n, N.rp, N.cc, N.cv)
        err = np.max(np.abs(got - want)) / np.max(np.abs(want))
        print(f"{name} level {l}: |A_c - P^T A P| / |A_c| = {err:.2e}")
        assert err <= 1e-13, (name, l, err)


@pytest.mark.parametrize("name", ("laplacian32x32", "laplacian12^3"))
def test_rows_of_p_sum_to_one_where_the_filtered_row_sum_is_zero(name):
    _, H = _case(name)
    L = H.levels[0]
    AF = sa.filtered(L.n, L.rp, L.cc, L.cv, H.theta)
    rows = np.repeat(np.arange(L.n), np.diff(AF[0]))
    zero = np.bincount(rows, weights=AF[2], minlength=L.n) == 0.0  # (integers: the sums are exact)
    p_sum = np.bincount(np.repeat(np.arange(L.n), np.diff(L.P[0])), weights=L.P[2], minlength=L.n)
    assert zero.sum() >= (30 * 30 if name == "laplacian32x32" else 10**3), "the interior rows"
    assert np.max(np.abs(p_sum[zero] - 1.0)) <= 8 * 2.0**-52, np.max(np.abs(p_sum[zero] - 1.0))
    assert np.all(np.abs(p_sum[~zero] - 1.0) > 1e-3), "a boundary row loses mass"


def _dyadic_anisotropic():
    return ar.anisotropic_2d(16, ax=1.0, ay=2.0**-6)


@pytest.mark.parametrize("theta", (0.25, 0.5, 0.0))
def test_the_filter_keeps_the_row_sums_exactly_on_dyadic_values(theta):
    systems = [_dyadic_anisotropic()] + [ar.fuzz_system(seed) for seed in (2, 4, 7, 16, 17)]
    lumped = 0
    for n, rp, cc, cv in systems:
        rp_f, cc_f, cv_f = sa.filtered(n, rp, cc, cv, theta)
        if theta <= 0.0:
            assert rp_f is rp or np.array_equal(rp_f, rp) and cc_f.tobytes() == np.asarray(cc).tobytes() and cv_f.tobytes() == cv.tobytes()
            continue
        own = np.bincount(np.repeat(np.arange(n), np.diff(rp)), weights=cv, minlength=n)
        kept = np.bincount(np.repeat(np.arange(n), np.diff(rp_f)), weights=cv_f, minlength=n)
        assert own.tobytes() == kept.tobytes()  # (every partial sum is a multiple of 2^-10 below 2^20: exact)
        _, mask = ar.neighbour_mask(n, rp, cc, cv, theta)
        rows = np.repeat(np.arange(n), np.diff(rp))
        weak_rows = np.unique(rows[~mask & (rows != cc)])
        lumped += len(weak_rows)
        # one more entry in exactly the rows that hold a weak entry, and it is the last one, on the diagonal
        assert np.array_equal(np.diff(rp_f), np.bincount(rows[mask | (rows == cc)], minlength=n) + np.isin(np.arange(n), weak_rows))
        assert np.all(cc_f[rp_f[1:][weak_rows] - 1] == weak_rows)
    assert theta <= 0.0 or lumped > 100


# ---- 2. the operator B -----------------------------------------------------------------------------------------------------------------
SPD = {"laplacian12x12": lambda: cr.laplacian_2d_csr(12), "laplacian6^3": lambda: ir.laplacian_3d(6)}


@pytest.mark.parametrize("omega", (1.0, 1.5))
@pytest.mark.parametrize("name", list(SPD))
def test_b_is_symmetric_positive_definite(name, omega):
    n, rp, cc, cv = SPD[name]()
    H = sa.Hierarchy(n, rp, cc, cv, coarse_max=8, overcorrection=omega)
    assert len(H.levels) >= 3
    B = H.dense_operator()
    asym = np.max(np.abs(B - B.T)) / np.max(np.abs(B))
    low = np.linalg.eigvalsh((B + B.T) / 2).min()
    print(f"{name} omega {omega}: rows {H.rows}, |B - B^T| / |B| = {asym:.2e}, smallest eigenvalue {low:.3e}")
    assert asym <= 1e-13 and low > 0.0


def _a_norm_of_error_propagator(A, B):
    w, V = np.linalg.eigh(A)
    half, inv_half = (V * np.sqrt(w)) @ V.T, (V / np.sqrt(w)) @ V.T
    return np.linalg.norm(half @ (np.eye(len(A)) - B @ A) @ inv_half, 2)


def test_the_two_level_error_propagator_contracts_and_beats_plain_aggregation():
    out = {}
    for m in (12, 16):
        n, rp, cc, cv = cr.laplacian_2d_csr(m)
        A = ar.dense_of(n, rp, cc, cv)
        smoothed = sa.Hierarchy(n, rp, cc, cv, max_levels=2, coarse_max=8)
        plain = ar.Hierarchy(n, rp, cc, cv, max_levels=2, coarse_max=8)
        assert len(smoothed.levels) == 2 == len(plain.levels)
        out[m] = (_a_norm_of_error_propagator(A, smoothed.dense_operator()), _a_norm_of_error_propagator(A, plain.dense_operator()))
        print(f"{m} x {m}: ||E||_A smoothed {out[m][0]:.4f}, plain {out[m][1]:.4f}")
        assert out[m][0] < 1.0
    assert out[16][0] < out[16][1]


# ---- 3. the exact family ---------------------------------------------------------------------------------------------------------------
def test_the_exact_family_equals_the_integer_reference():
    """the 2-D Laplacian under prolong_damping = 1.0 and max_levels = 2: lam = 2, d = 4, c = 1/8; 8 P and 64 A_1 are integers"""
    m = 32
    n, rp, cc, cv = cr.laplacian_2d_csr(m)
    H = sa.Hierarchy(n, rp, cc, cv, max_levels=2, prolong_damping=1.0)
    L, N = H.levels
    assert L.lam == 2.0 and L.nc == 150
    assert np.all(8.0 * L.P[2] == np.round(8.0 * L.P[2])) and np.all(64.0 * N.cv == np.round(64.0 * N.cv))
    P8, A64, pattern_p, pattern_c = sa.exact_family_int64(m, L.agg, L.nc)
    assert P8.dtype == np.int64 == A64.dtype
    for got, want in ((L.P, sa.csr_of_dense(P8, pattern_p, 8.0)), ((N.rp, N.cc, N.cv), sa.csr_of_dense(A64, pattern_c, 64.0))):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2].tobytes() == want[2].tobytes()


# ---- 4. the iteration table -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("system", list(ar.SYSTEMS))
def test_iteration_counts_of_the_twins(system):
    x, iters = sa.run_twin(system)
    solver, n, rp, cc, cv, b = ar.solver_system(system)
    true = np.linalg.norm(b - ir.csr_mv(n, rp, cc, cv, x)) / np.linalg.norm(b)
    print(f"{system}: {iters} iterations (plain aggregation {ar.TWIN_ITERATIONS[system]}), residual {true:.2e}")
    assert iters == sa.TWIN_ITERATIONS[system], "the recorded count moved"
    assert iters <= ar.TWIN_ITERATIONS[system] and true <= 10 * ar.REL_TOL


# ---- 5. mutations ---------------------------------------------------------------------------------------------------------------------
def _compared():
    """(name, extra arguments) of every application tests/test_gpu_amg_sa.py compares with the twin, the large one aside"""
    return [(name, {}) for name in sa.SMALL] + [(name, extra) for name in sa.CONFIG_SYSTEMS for extra in sa.CONFIGS]


@pytest.mark.parametrize("mutation", sa.MUTATIONS)
def test_every_mutation_moves_every_application_or_cannot(mutation):
    moved, excused = 0, {}
    for name, extra in _compared():
        (n, rp, cc, cv), H = _case(name, **extra)
        r = sa.case_rhs(name, n)
        want = _once(("want", name, tuple(sorted(extra.items()))), lambda: H.apply(r))
        reason = sa.cannot_move(H, mutation)
        M = sa.Hierarchy(n, rp, cc, cv, **dict(sa.CASES[name][1], **extra), mutate=mutation)
        got = M.apply(r)
        err = np.max(np.abs(got - want)) / max(np.max(np.abs(want)), 1e-300) if M.rows == H.rows else np.inf
        if reason is None:
            assert err > 100 * ol.REL_TOL, (mutation, name, extra, err)
            moved += 1
        else:
            assert err <= ol.REL_TOL, (mutation, name, extra, reason, err)  # (nothing the gate could see)
            excused[reason] = excused.get(reason, 0) + 1
    print(f"{mutation}: moved {moved} applications beyond 100 gates; unmoved: {excused}")
    assert moved >= 8  # (omega_dropped: the eight applications under omega = 1.5; the others: most of them)


def test_the_coarsest_level_cases_have_the_rows_they_are_named_for():
    for rows in (1024, 1025):
        n, rp, cc, cv = sa.coarsest_rows_case(rows)
        agg, nc, _, _ = ar.aggregate(n, rp, cc, cv)
        assert nc == rows


# ---- 6. the fuzz systems ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ar.FUZZ_SEEDS)
def test_no_fuzz_system_raises(seed):
    """strictly dominant rows with a positive diagonal: d_i >= 1 after lumping, no coarse diagonal is zero"""
    n, rp, cc, cv = ar.fuzz_system(seed)
    H = sa.Hierarchy(n, rp, cc, cv, **ar.fuzz_setup(seed))
    for L in H.levels[:-1]:
        AF = sa.filtered(L.n, L.rp, L.cc, L.cv, H.theta)
        if L is H.levels[0]:
            assert sa.filtered_diagonal(L.n, *AF).min() >= 1.0
    assert np.all(np.isfinite(H.apply(sa.case_rhs(f"fuzz{seed:02d}", n))))
