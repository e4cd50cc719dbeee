"""Smoothed-aggregation AMG on the GPU (spmv_amg_setup_smoothed, spmv_amg_prolongator; the cycle behind spmv_amg_solve and
SPMV_PRECOND_AMG) against the NumPy twin tests/amg_sa_ref.py, which tests/test_amg_sa_ref.py holds to facts of its own on the CPU.

Prolongators, aggregates and operators of every level are compared exactly (indices equal, values equal bytes: spmv_spgemm defines
every sum and the row bound is a maximum); applications within oracle_lib.REL_TOL = 1e-10, norm-wise, the gate tests/test_gpu_amg.py
holds the plain cycle to; iteration counts one either side of the twin's.

Shapes: those of amg_sa_ref.CASES - n = 1, 2, 3 and 257 tridiagonal and diagonal; the 32 x 32 and 12^3 Laplacians; the 40 x 40
convection-diffusion system; 500 structurally nonsymmetric rows; the anisotropic 16 x 16 stencil at theta = 0.25 and 0.5 (the
filtered path: weak entries lumped); the 24 fuzz systems (duplicates, stored zeros, split diagonals, unsorted columns; theta 0, 0.1,
0.5); arrow matrices of 63 .. 300 rows (one aggregate: R is one row of n entries, P is n rows of one entry - the strided loop of
the restriction, its tail, and the one-lane prolongation); and the 1,048,579-row tridiagonal system with two levels (the grid-stride
loops' second trip; its twin takes about five seconds, once)."""
import numpy as np
import pytest

import amg_ref as ar
import amg_sa_ref as sa
import chebyshev_ref as cr
import oracle_lib as ol

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _system(name):
    return _once(("system", name), sa.CASES[name][0])


def _twin(name, **extra):
    kw = dict(sa.CASES[name][1], **extra)
    return _once(("twin", name, tuple(sorted(kw.items()))), lambda: sa.Hierarchy(*_system(name), **kw))


def _device_vector(ctx, host, aligned):
    """host on the device, 256-byte aligned or 8 bytes past a 16-byte boundary (wide_ok false)"""
    n = len(host)
    if aligned:
        v = ctx.vector_from(host)
        assert v.device_ptr % 16 == 0
        return v, None
    base = ctx.vector(n + 1)
    base.fill(0.0)
    v = ctx.wrap_vector(base.device_ptr + 8, n)
    v.upload(host)
    return v, base


def _apply(ctx, A, r_host, aligned=True):
    r, keep_r = _device_vector(ctx, r_host, aligned)
    z, keep_z = _device_vector(ctx, np.full(len(r_host), 7.0), aligned)  # (whatever z holds is ignored)
    ctx.amg_solve(A, r, z)
    ctx.sync()
    assert r.download().tobytes() == r_host.tobytes(), "the application wrote into r"
    return z.download()


def _close(got, want, what):
    err = np.max(np.abs(got - want)) / max(np.max(np.abs(want)), 1e-300)
    print(f"{what}: {err:.3e}")
    assert err <= ol.REL_TOL, (what, err)


def _same_csr(got, want, what):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what
    assert np.asarray(got[2]).tobytes() == np.asarray(want[2], dtype=np.float64).tobytes(), what


def _assert_hierarchy(ctx, A, H, name):
    levels, rows, nnz = ctx.amg_info(A)
    print(f"{name}: rows {rows.tolist()}, entries {nnz.tolist()}, P entries {[len(L.P[1]) for L in H.levels[:-1]]}")
    assert levels == len(H.levels) == A.get_param("amg_levels") and list(rows) == H.rows and list(nnz) == H.nnz
    assert A.get_param("amg_mis_rounds") == H.mis_rounds and A.get_param("amg_ready") == 1 and A.get_param("amg_smoothed") == 1
    assert A.get_param("amg_launches") == H.launches()
    for l, L in enumerate(H.levels):
        agg, rp, cc, cv = ctx.amg_level(A, l)
        if l + 1 < levels:
            assert np.array_equal(agg, L.agg), (name, l)
            _same_csr(ctx.amg_prolongator(A, l), L.P, (name, l, "P"))
        else:
            assert agg is None
        _same_csr((rp, cc, cv), (L.rp, L.cc, L.cv), (name, l, "A"))


# ---- 1. the hierarchy as bytes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sa.CASES))
def test_hierarchy_equals_the_twins(ctx, name):
    n, rp, cc, cv = _system(name)
    A = ctx.csr(n, n, rp, cc, cv)
    ctx.amg_setup_smoothed(A, **sa.CASES[name][1])
    _assert_hierarchy(ctx, A, _twin(name), name)


@pytest.mark.parametrize("m", (32, 64))
def test_the_exact_family_equals_the_integer_reference(ctx, m):
    """prolong_damping = 1.0 on the 2-D Laplacian: lam = 2, d = 4, c = 1/8; 8 P and 64 A_1 are integers"""
    n, rp, cc, cv = cr.laplacian_2d_csr(m)
    A = ctx.csr(n, n, rp, cc, cv)
    ctx.amg_setup_smoothed(A, max_levels=2, prolong_damping=1.0)
    agg = ctx.amg_level(A, 0)[0]
    nc = int(ctx.amg_info(A)[1][1])
    P8, A64, pattern_p, pattern_c = sa.exact_family_int64(m, agg, nc)
    _same_csr(ctx.amg_prolongator(A, 0), sa.csr_of_dense(P8, pattern_p, 8.0), (m, "P"))
    _same_csr(ctx.amg_level(A, 1)[1:], sa.csr_of_dense(A64, pattern_c, 64.0), (m, "A_1"))


# ---- 2. the application against the twin ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sa.SMALL)
def test_application_matches_the_twin(ctx, name):
    """every system, its own arguments, both alignments; the arrows are the row-length edges of the two cycle kernels"""
    n, rp, cc, cv = _system(name)
    A = ctx.csr(n, n, rp, cc, cv)
    ctx.amg_setup_smoothed(A, **sa.CASES[name][1])
    H = _twin(name)
    assert list(ctx.amg_info(A)[1]) == H.rows
    if name.startswith("arrow"):
        assert H.rows == [n, 1] and len(H.levels[0].R[1]) == n and len(H.levels[0].P[1]) == n
    r_host = sa.case_rhs(name, n)
    want = H.apply(r_host)
    for aligned in (True, False):
        _close(_apply(ctx, A, r_host, aligned), want, f"{name}, rows {H.rows}, aligned {aligned}")


@pytest.mark.parametrize("config", range(len(sa.CONFIGS)))
@pytest.mark.parametrize("name", sa.CONFIG_SYSTEMS)
def test_application_matches_the_twin_under_other_arguments(ctx, name, config):
    """degree 1 and 3, omega 1.0 and 1.5, damping 1.0 and 4/3, a two-grid hierarchy and coarse_max = 1"""
    extra = sa.CONFIGS[config]
    n, rp, cc, cv = _system(name)
    A = ctx.csr(n, n, rp, cc, cv)
    ctx.amg_setup_smoothed(A, **dict(sa.CASES[name][1], **extra))
    H = _twin(name, **extra)
    assert list(ctx.amg_info(A)[1]) == H.rows and A.get_param("amg_launches") == H.launches()
    r_host = sa.case_rhs(name, n)
    want = H.apply(r_host)
    for aligned in (True, False):
        _close(_apply(ctx, A, r_host, aligned), want, f"{name} {extra}, rows {H.rows}, aligned {aligned}")


@pytest.mark.parametrize("rows", (1024, 1025))
def test_the_coarsest_level_at_the_dense_limit(ctx, rows):
    """1024 rows on the coarsest level: the dense inverse; 1025: one Chebyshev application"""
    n, rp, cc, cv = sa.coarsest_rows_case(rows)
    A = ctx.csr(n, n, rp, cc, cv)
    ctx.amg_setup_smoothed(A, max_levels=2)
    H = _once(("coarsest", rows), lambda: sa.Hierarchy(n, rp, cc, cv, max_levels=2))
    assert H.rows == [n, rows] == list(ctx.amg_info(A)[1]) and (H.inv is not None) == (rows == 1024)
    assert A.get_param("amg_launches") == H.launches() == (15 + 1 if rows == 1024 else 15 + 5)
    r_host = np.random.default_rng(rows).uniform(-1, 1, n)
    want = H.apply(r_host)
    for aligned in (True, False):
        _close(_apply(ctx, A, r_host, aligned), want, f"{rows} coarsest rows, aligned {aligned}")


def test_application_matches_the_twin_beyond_one_trip_of_the_grid(ctx):
    name = "tridiagonal_big"
    n, rp, cc, cv = _system(name)
    A = ctx.csr(n, n, rp, cc, cv)
    ctx.amg_setup_smoothed(A, **sa.CASES[name][1])
    H = _twin(name)
    r_host = sa.case_rhs(name, n)
    _close(_apply(ctx, A, r_host), H.apply(r_host), f"n = {n}, rows {H.rows}")


# ---- 3. symmetry, determinism ---------------------------------------------------------------------------------------------------------
def test_the_cycle_is_symmetric_on_the_device(ctx):
    n, rp, cc, cv = _system("laplacian32x32")
    A = ctx.csr(n, n, rp, cc, cv)
    ctx.amg_setup_smoothed(A, coarse_max=8)
    rng = np.random.default_rng(31)
    u, v = rng.uniform(0.5, 1.5, n), rng.uniform(0.5, 1.5, n)
    LD = np.longdouble
    ubv, vbu = np.dot(u.astype(LD), _apply(ctx, A, v).astype(LD)), np.dot(v.astype(LD), _apply(ctx, A, u).astype(LD))
    print(f"u.Bv = {float(ubv)!r}, v.Bu = {float(vbu)!r}")
    assert ubv > 0 and abs(ubv - vbu) <= 1e-12 * abs(ubv)


def test_two_setups_and_two_applications_give_the_same_bits(ctx, pkg):
    n, rp, cc, cv = cr.laplacian_2d_csr(64)
    r_host = np.random.default_rng(29).uniform(-1, 1, n)
    out, operators = [], []
    for _ in range(2):
        A = ctx.csr(n, n, rp, cc, cv)
        A.set_kernel(pkg.capi.CSR_SCALAR)
        A.set_param("amg_level_kernel", pkg.capi.CSR_SCALAR)
        assert pkg.capi.CSR_SCALAR == 3 == A.get_param("amg_level_kernel")
        for _ in range(2):
            ctx.amg_setup_smoothed(A, coarse_max=8)
            out += [_apply(ctx, A, r_host).tobytes(), _apply(ctx, A, r_host).tobytes()]
            levels = ctx.amg_info(A)[0]
            operators.append(b"".join(np.ascontiguousarray(a).tobytes() for l in range(levels - 1)
                                      for a in ctx.amg_level(A, l) + ctx.amg_prolongator(A, l)))
    assert len(set(out)) == 1 and len(set(operators)) == 1


# ---- 4. the solvers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("system", list(ar.SYSTEMS))
def test_preconditioned_solvers_take_the_iterations_of_the_twins(ctx, pkg, system):
    capi = pkg.capi
    solver, n, rp, cc, cv, b_host = ar.solver_system(system)
    A = ctx.csr(n, n, rp, cc, cv)
    b, x = ctx.vector_from(b_host), ctx.vector(n)
    solve = {"cg": ctx.cg, "bicgstab": ctx.bicgstab, "gmres": ctx.gmres}[solver]
    x.fill(0.0)
    ctx.amg_setup_smoothed(A)
    iters, res = solve(A, b, x, max_iter=2000, rel_tol=ar.REL_TOL, precond=capi.PRECOND_AMG)
    assert A.get_param("amg_smoothed") == 1, "the solver replaced the state it was given"
    LD = np.longdouble
    rows = np.repeat(np.arange(n), np.diff(rp))
    ax = np.zeros(n, dtype=LD)
    np.add.at(ax, rows, cv.astype(LD) * x.download().astype(LD)[cc])
    true = float(np.sqrt(np.sum((b_host.astype(LD) - ax) ** 2)) / np.sqrt(np.sum(b_host.astype(LD) ** 2)))
    recorded = sa.TWIN_ITERATIONS[system]
    print(f"{system}: {iters} iterations (smoothed twin {recorded}, plain twin {ar.TWIN_ITERATIONS[system]}), reported {res:.3e}, true {true:.3e}")
    assert abs(iters - recorded) <= 1, (iters, recorded)
    assert res <= ar.REL_TOL and true <= ar.REL_TOL, (res, true)


# ---- 5. state -----------------------------------------------------------------------------------------------------------------------
def _neumann_1d(n):
    """the singular 1-D Laplacian with natural boundary rows; under prolong_damping = 1.0 (lam = 2, every c dyadic) the rows of P sum
    to 1 exactly and every coarse operator keeps the zero row sums exactly"""
    n, rp, cc, cv = cr.tridiagonal(n)
    cv = cv.copy()
    cv[0] = cv[-1] = 1.0
    return n, rp, cc, cv


def test_parameters_bytes_and_the_plain_state_again(ctx, pkg):
    capi = pkg.capi
    n, rp, cc, cv = _system("laplacian32x32")
    A = ctx.csr(n, n, rp, cc, cv)
    before = A.get_param("device_bytes")
    assert A.get_param("amg_smoothed") == 0

    def expect(call, code, word):
        with pytest.raises(capi.SpmvError) as e:
            call()
        assert e.value.code == code and word in str(e.value), (code, word, e.value)

    expect(lambda: ctx.amg_prolongator(A, 0), INVALID, "not set up")
    ctx.amg_setup(A, coarse_max=8)
    plain_bytes, plain_rows = A.get_param("amg_bytes"), list(ctx.amg_info(A)[1])
    plain_levels = [ctx.amg_level(A, l) for l in range(len(plain_rows))]
    assert A.get_param("amg_smoothed") == 0
    expect(lambda: ctx.amg_prolongator(A, 0), INVALID, "plain aggregation")
    r_host = sa.case_rhs("laplacian32x32", n)
    z_plain = _apply(ctx, A, r_host)
    # the smoothed state replaces it
    ctx.amg_setup_smoothed(A, coarse_max=8)
    H = _twin("laplacian32x32")
    grown, cheby = A.get_param("amg_bytes"), A.get_param("cheby_bytes")
    print(f"amg_bytes: plain {plain_bytes}, smoothed {grown} (arrays and vectors alone: {H.state_bytes()})")
    assert A.get_param("amg_smoothed") == 1 and A.get_param("amg_launches") == H.launches() == 3 * 15 + 1
    assert grown >= H.state_bytes() and A.get_param("device_bytes") == before + grown + cheby
    levels = ctx.amg_info(A)[0]
    expect(lambda: ctx.amg_prolongator(A, levels - 1), INVALID, "coarsest")
    expect(lambda: ctx.amg_prolongator(A, levels), INVALID, f"level={levels}")
    z = _apply(ctx, A, r_host)
    # refused set-ups leave it: on the host (damping 2.0) and on the device (a zero diagonal is found before anything is replaced)
    expect(lambda: ctx.amg_setup_smoothed(A, coarse_max=8, prolong_damping=2.0), INVALID, "prolong_damping=2")
    assert A.get_param("amg_bytes") == grown and A.get_param("amg_smoothed") == 1 and _apply(ctx, A, r_host).tobytes() == z.tobytes()
    # the plain set-up gives the plain hierarchy's bytes again
    ctx.amg_setup(A, coarse_max=8)
    assert A.get_param("amg_smoothed") == 0 and A.get_param("amg_bytes") == plain_bytes and list(ctx.amg_info(A)[1]) == plain_rows
    for l, want in enumerate(plain_levels):
        got = ctx.amg_level(A, l)
        assert all((g is None and w is None) or np.asarray(g).tobytes() == np.asarray(w).tobytes() for g, w in zip(got, want)), l
    assert _apply(ctx, A, r_host).tobytes() == z_plain.tobytes()
    other = capi.Context(0)
    expect(lambda: other.amg_setup_smoothed(A), INVALID, "context")
    other.close()


def test_lanes_follow_the_rule_and_the_transfers_run_by_themselves(ctx, pkg):
    """"amg_lanes_p<level>" / "amg_lanes_r<level>" are the rule of amg_sa_settings.hpp on the twin's P; spmv_amg_transfer_timed runs the
    four variants and every number of lanes, leaves the state's applications as they were and refuses what it documents.  No timing
    is asserted"""
    capi = pkg.capi
    n, rp, cc, cv = _system("laplacian12^3")
    A = ctx.csr(n, n, rp, cc, cv)
    ctx.amg_setup_smoothed(A, coarse_max=8)
    H = _twin("laplacian12^3")

    def rule(entries, rows):
        g = 1
        while g < 64 and 4 * g * rows <= entries:
            g *= 2
        return g

    for l, L in enumerate(H.levels[:-1]):
        assert A.get_param(f"amg_lanes_p{l}") == rule(len(L.P[1]), L.n) and A.get_param(f"amg_lanes_r{l}") == rule(len(L.P[1]), L.nc), l
    assert A.get_param("amg_lanes_r0") >= 8, "rows of R hold about 57 entries in 3-D"
    with pytest.raises(capi.SpmvError):
        A.get_param(f"amg_lanes_p{len(H.levels) - 1}")
    r_host = sa.case_rhs("laplacian12^3", n)
    z = _apply(ctx, A, r_host)
    v = ctx.vector(n)
    v.fill(0.0)
    for what in (capi.AMG_RESTRICT_FUSED, capi.AMG_RESTRICT_UNFUSED, capi.AMG_PROLONG_FUSED, capi.AMG_PROLONG_UNFUSED):
        assert ctx.amg_transfer_timed(A, 0, what, v, 2) > 0.0
    for lanes in (1, 2, 4, 8, 16, 32, 64):
        assert ctx.amg_transfer_timed(A, 0, capi.AMG_RESTRICT_FUSED, v, 1, lanes) > 0.0
        assert ctx.amg_transfer_timed(A, 0, capi.AMG_PROLONG_FUSED, v, 1, lanes) > 0.0
    assert np.all(np.isfinite(v.download()))
    assert _apply(ctx, A, r_host).tobytes() == z.tobytes()
    for call, word in ((lambda: ctx.amg_transfer_timed(A, len(H.levels) - 1, 0, v, 1), "coarsest"),
                       (lambda: ctx.amg_transfer_timed(A, 0, 4, v, 1), "what=4"),
                       (lambda: ctx.amg_transfer_timed(A, 0, 0, v, 1, 3), "lanes=3"),
                       (lambda: ctx.amg_transfer_timed(A, 0, 0, ctx.vector(n + 1), 1), "entries")):
        with pytest.raises(capi.SpmvError) as e:
            call()
        assert e.value.code == INVALID and word in str(e.value), (word, e.value)
    ctx.amg_setup(A, coarse_max=8)
    with pytest.raises(capi.SpmvError) as e:
        ctx.amg_transfer_timed(A, 0, 0, v, 1)
    assert e.value.code == INVALID and "plain aggregation" in str(e.value)


def test_a_singular_coarsest_operator_leaves_the_earlier_state(ctx, pkg):
    capi = pkg.capi
    n, rp, cc, cv = _neumann_1d(1100)
    A = ctx.csr(n, n, rp, cc, cv)
    ctx.amg_setup_smoothed(A, max_levels=1)  # one level, served by Chebyshev: the singular operator is never inverted
    grown, total = A.get_param("amg_bytes"), A.get_param("device_bytes")
    assert ctx.amg_info(A)[0] == 1 and A.get_param("amg_launches") == 5 and A.get_param("amg_smoothed") == 1
    r_host = np.random.default_rng(6).uniform(-1, 1, n)
    z = _apply(ctx, A, r_host)
    with pytest.raises(ValueError):
        sa.Hierarchy(n, rp, cc, cv, smooth_degree=3, prolong_damping=1.0)
    with pytest.raises(capi.SpmvError) as e:
        ctx.amg_setup_smoothed(A, smooth_degree=3, prolong_damping=1.0)
    assert e.value.code == INVALID and "singular coarsest operator" in str(e.value)
    assert A.get_param("amg_bytes") == grown and A.get_param("device_bytes") == total and ctx.amg_info(A)[0] == 1
    assert A.get_param("cheby_degree") == 2 and A.get_param("amg_smoothed") == 1 and _apply(ctx, A, r_host).tobytes() == z.tobytes()


def test_destroying_the_handle_frees_everything(ctx):
    """free device memory (hipMemGetInfo) around two handles of 262,147 rows with their smoothed hierarchies: equal before the
    second set-up and after its handle is gone (the first pass also grows what the context keeps)"""
    n, rp, cc, cv = cr.tridiagonal(262147)
    r = ctx.vector_from(np.ones(n))
    z = ctx.vector(n)
    free = []
    for _ in range(2):
        ctx.sync()
        free.append(ctx.mem_info()[0])
        A = ctx.csr(n, n, rp, cc, cv)
        ctx.amg_setup_smoothed(A)
        ctx.amg_solve(A, r, z)
        ctx.sync()
        held, inside = A.get_param("device_bytes"), ctx.mem_info()[0]
        assert A.get_param("amg_bytes") >= 8 * n
        del A
    ctx.sync()
    free.append(ctx.mem_info()[0])
    print(f"free device memory around two handles: {free}, inside the second {inside}, its device_bytes {held}")
    assert free[1] - inside >= held // 2 and free[2] == free[1]
