"""The Chebyshev polynomial preconditioner / smoother and the Lanczos estimate on the GPU (spmv_chebyshev_*, spmv_lanczos;
SPMV_PRECOND_CHEBYSHEV in spmv_cg, spmv_bicgstab and spmv_gmres) against the NumPy twin tests/chebyshev_ref.py, which
tests/test_chebyshev_ref.py holds to facts of its own on the CPU.

Shapes, for the paths of the kernels: n = 0, 1, 2, 3 and 257, diagonal and tridiagonal; n = 2 kMaxGrid kBlock + 3 = 1,048,579
tridiagonal (the grid-stride loop's second trip and an odd tail); n = (8 << 20) + 3 = 8,388,611 tridiagonal (from 8 << 20 rows on the
wide step reads and writes w and t nontemporally: all eight instantiations, scaled x first x last); r and z 8 bytes past a 16-byte boundary (the narrow path), alone
and mixed with aligned vectors; degree 1 (the first and the last term in one launch), 2 and 9; scaled and unscaled; a CSR handle
forced to the row-parallel kernel and one left to AUTO; an ELL and a COO handle with explicit bounds."""
import numpy as np
import pytest

import chebyshev_ref as cr
import ilu0_ref as ir
import oracle_lib as ol
import solver_ref

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
BIG = 2 * 2048 * 256 + 3
DEGREES = (1, 2, 9)
ALIGNMENTS = ((True, True), (False, False), (True, False), (False, True))  # (r, z) 16-byte aligned
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _mv(n, rp, cc, cv):
    rows = np.repeat(np.arange(n), np.diff(rp))
    return lambda x: np.bincount(rows, weights=cv * x[cc], minlength=n)


def _matrix(kind, n):
    def make():
        if kind == "diagonal":
            return cr.diagonal(np.random.default_rng(100 + n).uniform(0.5, 2.0, n))
        if kind == "tridiagonal":
            return cr.tridiagonal(n)
        if kind == "laplacian24":
            return ir.laplacian_3d(24)
        if kind == "laplacian32x32":
            return cr.laplacian_2d_csr(32)
        raise KeyError(kind)

    return _once(("matrix", kind, n), make)


def _device_vector(ctx, host, aligned):
    """host on the device, 256-byte aligned or 8 bytes past a 16-byte boundary (a wrapped pointer into a vector of n + 1)"""
    n = len(host)
    if aligned:
        v = ctx.vector_from(host)
        assert v.device_ptr % 16 == 0
        return v, None
    base = ctx.vector(n + 1)
    base.fill(0.0)
    v = ctx.wrap_vector(base.device_ptr + 8, n)
    assert (base.device_ptr + 8) % 16 == 8
    v.upload(host)
    return v, base


def _close(got, want, what):
    err = np.max(np.abs(got - want)) / max(np.max(np.abs(want)), 1e-300)
    print(f"{what}: {err:.3e}")
    assert err <= ol.REL_TOL, (what, err)


def _twin_apply(n, rp, cc, cv, info, r):
    degree, scaled, lmin, lmax = info
    s = cr.inverse_diagonal(n, rp, cc, cv) if scaled else None
    c0, c1, c2 = cr.coefficients(degree, lmin, lmax)
    return cr.apply(_mv(n, rp, cc, cv), s, r, c0, c1, c2)


def _apply(ctx, A, r_host, aligned=(True, True)):
    r, keep_r = _device_vector(ctx, r_host, aligned[0])
    z, keep_z = _device_vector(ctx, np.full(len(r_host), 7.0), aligned[1])  # (whatever z holds is ignored)
    ctx.chebyshev_solve(A, r, z)
    ctx.sync()
    assert r.download().tobytes() == r_host.tobytes(), "the application wrote into r"
    return z.download()


# ---- 1. the application against the twin ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 2, 3, 257))
@pytest.mark.parametrize("kind", ("diagonal", "tridiagonal"))
def test_application_matches_the_twin_on_small_shapes(ctx, kind, n):
    _, rp, cc, cv = _matrix(kind, n)
    A = ctx.csr(n, n, rp, cc, cv)
    r_host = np.random.default_rng(200 + n).uniform(-1, 1, n)
    unscaled_lmax = cr.row_bound(n, rp, cc, cv)
    for degree in DEGREES:
        for scaled in (True, False):
            if scaled:
                ctx.chebyshev_setup(A, degree)  # lmax the row bound, lmin a thirtieth of it
                s = cr.inverse_diagonal(n, rp, cc, cv)
                assert ctx.chebyshev_info(A) == (degree, True, cr.row_bound(n, rp, cc, cv, s) / 30.0, cr.row_bound(n, rp, cc, cv, s))
            else:
                ctx.chebyshev_setup(A, degree, scaled=False, lmin=0.1, lmax=unscaled_lmax)
                assert ctx.chebyshev_info(A) == (degree, False, 0.1, unscaled_lmax)
            assert A.get_param("cheby_launches") == 2 * degree + 1 and A.get_param("cheby_degree") == degree
            want = _twin_apply(n, rp, cc, cv, ctx.chebyshev_info(A), r_host)
            for aligned in ALIGNMENTS:
                _close(_apply(ctx, A, r_host, aligned), want, f"{kind} n = {n}, degree {degree}, scaled {scaled}, aligned {aligned}")


def test_an_empty_system(ctx):
    A = ctx.csr(0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    ctx.chebyshev_setup(A, 3)
    assert ctx.chebyshev_info(A)[0] == 3 and A.get_param("cheby_bytes") == 0
    ctx.chebyshev_solve(A, ctx.vector(0), ctx.vector(0))
    ctx.chebyshev(A, ctx.vector(0), ctx.vector(0))
    assert ctx.lanczos(A, 4)[4] == 0
    ctx.sync()


@pytest.mark.parametrize("aligned", ALIGNMENTS[:3], ids=["aligned", "narrow", "mixed"])
def test_application_matches_the_twin_beyond_one_trip_of_the_grid(ctx, aligned):
    n, rp, cc, cv = _matrix("tridiagonal", BIG)
    A = _once(("handle", "big"), lambda: ctx.csr(n, n, rp, cc, cv))
    ctx.chebyshev_setup(A, 2)
    assert ctx.chebyshev_info(A) == (2, True, 2.0 / 30.0, 2.0)
    r_host = _once(("r", "big"), lambda: np.random.default_rng(7).uniform(-1, 1, n))
    want = _once(("want", "big"), lambda: _twin_apply(n, rp, cc, cv, (2, True, 2.0 / 30.0, 2.0), r_host))
    _close(_apply(ctx, A, r_host, aligned), want, f"n = {n}, aligned {aligned}")


# From kChebyNtRows = 8 << 20 rows on the wide step kernel reads w and t and writes t with nontemporal accesses: eight instantiations
# (scaled x first x last) that the sizes above never reach and the benchmarked sizes always do.  One matrix, one r, one handle.
NT_ROWS = (8 << 20) + 3


def _nt(ctx):
    def make():
        n, rp, cc, cv = _matrix("tridiagonal", NT_ROWS)
        r_host = np.random.default_rng(11).uniform(-1, 1, n)
        return n, rp, cc, cv, r_host, ctx.csr(n, n, rp, cc, cv), ctx.vector_from(r_host)

    return _once(("nt", "system"), make)


def _nt_setup(ctx, A, n, rp, cc, cv, degree, scaled):
    """the default scaled set-up, or unscaled on [0.1, the row bound]; returns chebyshev_info"""
    if scaled:
        ctx.chebyshev_setup(A, degree)
        assert ctx.chebyshev_info(A) == (degree, True, 2.0 / 30.0, 2.0)
    else:
        ctx.chebyshev_setup(A, degree, scaled=False, lmin=0.1, lmax=cr.row_bound(n, rp, cc, cv))
        assert ctx.chebyshev_info(A) == (degree, False, 0.1, 4.0)
    return ctx.chebyshev_info(A)


@pytest.mark.parametrize("scaled", (True, False), ids=["scaled", "unscaled"])
@pytest.mark.parametrize("degree", (1, 3))
def test_application_matches_the_twin_on_the_nontemporal_path(ctx, degree, scaled):
    """degree 1: the first and the last term in one launch; degree 3: a first, a middle and a last one"""
    n, rp, cc, cv, r_host, A, r = _nt(ctx)
    info = _nt_setup(ctx, A, n, rp, cc, cv, degree, scaled)
    want = _once(("nt", "want", degree, scaled), lambda: _twin_apply(n, rp, cc, cv, info, r_host))
    z = ctx.vector(n)
    z.fill(7.0)  # (whatever z holds is ignored)
    assert r.device_ptr % 16 == 0 and z.device_ptr % 16 == 0 and n >= 8 << 20
    ctx.chebyshev_solve(A, r, z)
    ctx.sync()
    _close(z.download(), want, f"n = {n}, degree {degree}, scaled {scaled}, kernel {A.info.kernel}")


def test_a_narrow_z_of_that_size_takes_the_plain_path(ctx):
    """for contrast: 8 bytes past a 16-byte boundary there is no wide path, so no nontemporal one; the same numbers"""
    n, rp, cc, cv, r_host, A, r = _nt(ctx)
    info = _nt_setup(ctx, A, n, rp, cc, cv, 3, True)
    want = _once(("nt", "want", 3, True), lambda: _twin_apply(n, rp, cc, cv, info, r_host))
    z, keep = _device_vector(ctx, np.full(n, 7.0), False)
    ctx.chebyshev_solve(A, r, z)
    ctx.sync()
    _close(z.download(), want, f"n = {n}, degree 3, scaled, z narrow")


def test_the_smoother_follows_the_twin_on_the_nontemporal_path(ctx):
    """x += M^-1 (b - A x): the residual is the state's own t, so no step is a FIRST one, and the start adds into x"""
    n, rp, cc, cv, r_host, A, b = _nt(ctx)
    info = _nt_setup(ctx, A, n, rp, cc, cv, 2, True)
    c0, c1, c2 = cr.coefficients(2, info[2], info[3])
    s, mv = cr.inverse_diagonal(n, rp, cc, cv), _mv(n, rp, cc, cv)
    twin = np.random.default_rng(12).uniform(-1, 1, n)
    x = ctx.vector_from(twin)
    assert x.device_ptr % 16 == 0
    for call in range(2):
        ctx.chebyshev(A, b, x)
        ctx.sync()
        twin = cr.smooth(mv, s, r_host, twin, c0, c1, c2)
        _close(x.download(), twin, f"n = {n}, degree 2, call {call}: x against the twin's")
    assert b.download().tobytes() == r_host.tobytes()


@pytest.mark.parametrize("scaled", (False, True), ids=["unscaled", "scaled"])
@pytest.mark.parametrize("degree", DEGREES)
def test_diagonal_family_follows_the_closed_form(ctx, degree, scaled):
    """within 8 E_d of the closed form in longdouble, E_d what the float64 twin leaves (chebyshev_ref.E_D); 8 is the factor
    tests/test_gpu_ilu0.py grants over what its reference leaves (solver_ref.F): fma against separate rounding"""
    lmin, lmax = cr.DIAGONAL_BOUNDS
    lam = cr.diagonal_family(lmin, lmax)
    n = len(lam)
    r_host = np.random.default_rng(5).uniform(0.5, 1.5, n)
    A = ctx.csr(*((n, n) + cr.diagonal(lam)[1:]))
    ctx.chebyshev_setup(A, degree, scaled=scaled, lmin=lmin, lmax=lmax)
    z = _apply(ctx, A, r_host)
    LD = np.longdouble
    if scaled:  # B = I up to the rounding of (1 / a) a: every eigenvalue is 1, and z_i / r_i = s_i p_d(1)
        want = cr.closed_form(np.ones(n), degree, lmin, lmax) / lam.astype(LD)
    else:
        want = cr.closed_form(lam, degree, lmin, lmax)
    err = float(np.max(np.abs(z.astype(LD) / r_host - want) / np.abs(want)))
    print(f"degree {degree}, scaled {scaled}: {err:.3e} against 8 E_d = {solver_ref.F * cr.E_D[degree]:.3e}")
    assert err <= solver_ref.F * cr.E_D[degree]


@pytest.mark.parametrize("which", ("csr_vector", "csr_auto", "ell", "coo"))
def test_application_matches_the_twin_through_every_product(ctx, pkg, which):
    capi = pkg.capi
    n, rp, cc, cv = _matrix("laplacian24", 0)
    r_host = _once(("r", "lap24"), lambda: np.random.default_rng(9).uniform(-1, 1, n))
    A = ctx.csr(n, n, rp, cc, cv)
    if which == "csr_vector":
        A.set_kernel(capi.CSR_VECTOR)
    elif which == "csr_auto":
        print("AUTO chose kernel", A.info.kernel)
    elif which == "ell":
        A = ctx.csr_to_ell(A)
    else:
        A = ctx.coo(n, n, np.repeat(np.arange(n, dtype=np.int32), np.diff(rp)), cc, cv)
    for degree in (1, 4):
        if which.startswith("csr"):
            ctx.chebyshev_setup(A, degree)
            assert ctx.chebyshev_info(A) == (degree, True, 2.0 / 30.0, 2.0)
        else:
            ctx.chebyshev_setup(A, degree, scaled=False, lmin=0.4, lmax=12.0)
            assert ctx.chebyshev_info(A) == (degree, False, 0.4, 12.0)
        want = _twin_apply(n, rp, cc, cv, ctx.chebyshev_info(A), r_host)
        _close(_apply(ctx, A, r_host), want, f"{which}, degree {degree}")


# ---- 2. reproducibility, parameters -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("csr_vector", "csr_auto"))
def test_two_setups_and_two_applications_give_the_same_bits(ctx, pkg, which):
    n, rp, cc, cv = _matrix("laplacian24", 0)
    r_host = np.random.default_rng(29).uniform(-1, 1, n)
    out = []
    for _ in range(2):
        A = ctx.csr(n, n, rp, cc, cv)
        if which == "csr_vector":
            A.set_kernel(pkg.capi.CSR_VECTOR)
        ctx.chebyshev_setup(A, 5)
        out += [_apply(ctx, A, r_host).tobytes(), _apply(ctx, A, r_host).tobytes()]
        ctx.chebyshev_setup(A, 5)
        out.append(_apply(ctx, A, r_host).tobytes())
    assert len(set(out)) == 1


def test_parameters_and_device_bytes(ctx):
    n, rp, cc, cv = _matrix("laplacian24", 0)
    A = ctx.csr(n, n, rp, cc, cv)
    before, plan, kernel = A.get_param("device_bytes"), A.get_plan(), A.info.kernel
    assert A.get_param("cheby_ready") == 0 and A.get_param("cheby_bytes") == 0 and A.get_param("cheby_launches") == 0
    assert A.get_param("cheby_degree") == 4 and A.get_param("cheby_lanczos_steps") == 0 and ctx.chebyshev_info(A) == (0, False, 0.0, 0.0)
    ctx.chebyshev_setup(A, 3)
    grown = A.get_param("cheby_bytes")
    assert grown >= 8 * 4 * n and A.get_param("cheby_ready") == 1 and A.get_param("cheby_launches") == 7
    assert A.get_param("device_bytes") == before + grown and A.info.device_bytes == before + grown
    ctx.chebyshev_setup(A, 9, scaled=False, lmin=0.5, lmax=12.0)
    grown = A.get_param("cheby_bytes")
    assert 8 * 3 * n <= grown < 8 * 4 * n and A.get_param("cheby_launches") == 19 and A.get_param("cheby_degree") == 9
    assert A.get_param("device_bytes") == before + grown
    assert A.get_plan() == plan and A.info.kernel == kernel
    A.set_param("cheby_lanczos_steps", 16)
    assert A.get_param("cheby_lanczos_steps") == 16
    for name, value in (("cheby_lanczos_steps", 65), ("cheby_lanczos_steps", -1), ("cheby_ratio", 1), ("cheby_degree", 0), ("cheby_degree", 65)):
        with pytest.raises(Exception):
            A.set_param(name, value)


# ---- 3. the set-up ----------------------------------------------------------------------------------------------------------------------
def test_setup_chooses_its_bounds(ctx, pkg):
    capi = pkg.capi
    for kind, size in (("laplacian24", 0), ("laplacian32x32", 0)):
        n, rp, cc, cv = _matrix(kind, size)
        A = ctx.csr(n, n, rp, cc, cv)
        ctx.chebyshev_setup(A)
        assert ctx.chebyshev_info(A) == (4, True, 2.0 / 30.0, 2.0) and A.get_param("cheby_lmax_source") == 1
        ctx.chebyshev_setup(A, 4, lmin=0.123, lmax=1.987)
        assert ctx.chebyshev_info(A) == (4, True, 0.123, 1.987) and A.get_param("cheby_lmax_source") == 0
        A.set_param("cheby_ratio", 10)
        ctx.chebyshev_setup(A, 4, lmax=1.5)
        assert ctx.chebyshev_info(A) == (4, True, 1.5 / 10.0, 1.5)
        A.set_param("cheby_ratio", 30)
        A.set_param("cheby_lanczos_steps", 16)
        ritz_max = ctx.lanczos(A, 16, scaled=True, seed=1)[1]
        ctx.chebyshev_setup(A)
        want = min(2.0, 1.05 * ritz_max)
        print(f"{kind}: 1.05 ritz_max = {1.05 * ritz_max:.6f}, the row bound 2")
        assert ctx.chebyshev_info(A) == (4, True, want / 30.0, want)
        assert A.get_param("cheby_lmax_source") == (2 if want < 2.0 else 1)
    # a handle without CSR arrays: the Lanczos value alone, or nothing
    n, rp, cc, cv = _matrix("laplacian32x32", 0)
    E = ctx.csr_to_ell(ctx.csr(n, n, rp, cc, cv))

    def expect(call, code, word):
        with pytest.raises(capi.SpmvError) as e:
            call()
        assert e.value.code == code and word in str(e.value), (code, word, e.value)

    expect(lambda: ctx.chebyshev_setup(E, 4), INVALID, "CSR")
    expect(lambda: ctx.chebyshev_setup(E, 4, scaled=False), UNSUPPORTED, "no source for lmax")
    assert E.get_param("cheby_ready") == 0 and ctx.chebyshev_info(E)[0] == 0
    expect(lambda: ctx.chebyshev_solve(E, ctx.vector(n), ctx.vector(n)), INVALID, "not set up")
    expect(lambda: ctx.chebyshev(E, ctx.vector(n), ctx.vector(n)), INVALID, "not set up")
    E.set_param("cheby_lanczos_steps", 12)
    ritz_max = ctx.lanczos(E, 12, scaled=False, seed=1)[1]
    ctx.chebyshev_setup(E, 4, scaled=False)
    assert ctx.chebyshev_info(E) == (4, False, 1.05 * ritz_max / 30.0, 1.05 * ritz_max) and E.get_param("cheby_lmax_source") == 2
    # a zero diagonal entry; a failed set-up leaves the earlier state
    rows = np.repeat(np.arange(n), np.diff(rp))
    Z = ctx.csr(n, n, rp, cc, np.where((rows == cc) & (rows == 5), 0.0, cv))
    ctx.chebyshev_setup(Z, 2, scaled=False, lmin=0.5, lmax=8.0)
    before = Z.get_param("device_bytes")
    expect(lambda: ctx.chebyshev_setup(Z, 4), INVALID, "diagonal")
    assert ctx.chebyshev_info(Z) == (2, False, 0.5, 8.0) and Z.get_param("device_bytes") == before
    expect(lambda: ctx.lanczos(Z, 4, scaled=True), INVALID, "diagonal")
    N = ctx.csr(n, n, rp, cc, np.where(rows == cc, -cv, cv))
    expect(lambda: ctx.lanczos(N, 4, scaled=True), INVALID, "not positive")
    other = capi.Context(0)
    expect(lambda: other.chebyshev_setup(Z, 4), INVALID, "context")
    other.close()


# ---- 4. Lanczos -----------------------------------------------------------------------------------------------------------------------
def _twin_lanczos(pkg, n, rp, cc, cv, scaled, m, seed=1):
    s = cr.inverse_diagonal(n, rp, cc, cv) if scaled else None
    return cr.lanczos(_mv(n, rp, cc, cv), s, pkg.synth.vec_uniform(n, seed=seed), m)


@pytest.mark.parametrize("scaled", (False, True), ids=["unscaled", "scaled"])
@pytest.mark.parametrize("m", (8, 16))
def test_lanczos_matches_the_twin(ctx, pkg, m, scaled):
    n, rp, cc, cv = _matrix("laplacian32x32", 0)
    A = ctx.csr(n, n, rp, cc, cv)
    lo, hi, alpha, beta, done = ctx.lanczos(A, m, scaled=scaled)
    ta, tb, tdone, tlo, thi = _twin_lanczos(pkg, n, rp, cc, cv, scaled, m)
    assert done == tdone == m
    dev = max(np.max(np.abs(alpha - ta)), np.max(np.abs(beta - tb))) / thi
    print(f"m = {m}, scaled {scaled}: coefficients within {dev:.3e} of the twin's (relative to ritz_max); Ritz extremes {lo:.6f}, {hi:.6f}")
    assert dev <= ol.REL_TOL
    assert abs(lo - tlo) <= ol.REL_TOL * thi and abs(hi - thi) <= ol.REL_TOL * thi
    lmin, lmax = cr.laplacian_2d_bounds(32)
    assert hi <= (lmax / 4.0 if scaled else lmax) and lo >= (lmin / 4.0 if scaled else lmin)
    again = ctx.lanczos(A, m, scaled=scaled)
    assert (again[0], again[1], again[4]) == (lo, hi, done) and again[2].tobytes() == alpha.tobytes() and again[3].tobytes() == beta.tobytes()


def test_lanczos_breakdown(ctx, pkg):
    n = 257
    eps = np.spacing(1.0)
    I = ctx.csr(*((n, n) + cr.diagonal(np.ones(n))[1:]))
    lo, hi, alpha, beta, done = ctx.lanczos(I, 8)
    print(f"identity: {done} step(s), Ritz values {lo!r}, {hi!r}, beta {beta}")
    # alpha_0 = v_0 . v_0, 1 up to the rounding of the normalisation and of a sum of n terms
    assert done == 1 and lo == hi == alpha[0] and abs(lo - 1.0) <= 2 * (n + 4) * eps
    diag = np.repeat([1.0, 1.25, 1.75], [100, 90, 67])
    D = ctx.csr(*((n, n) + cr.diagonal(diag)[1:]))
    for scaled in (False, True):  # (scaled: B = I up to rounding, one step)
        lo, hi, alpha, beta, done = ctx.lanczos(D, 8, scaled=scaled)
        ta, tb, tdone, tlo, thi = _twin_lanczos(pkg, *cr.diagonal(diag), scaled, 8)
        print(f"three values, scaled {scaled}: {done} steps, Ritz extremes {lo!r}, {hi!r} (twin {tlo!r}, {thi!r})")
        assert done == tdone == (1 if scaled else 3)
        assert abs(lo - tlo) <= ol.REL_TOL * thi and abs(hi - thi) <= ol.REL_TOL * thi
        if not scaled:
            assert abs(lo - 1.0) <= 2 * (n + 4) * eps * 1.75 and abs(hi - 1.75) <= 2 * (n + 4) * eps * 1.75


def test_lanczos_beyond_one_trip_of_the_grid(ctx, pkg):
    n, rp, cc, cv = _matrix("tridiagonal", BIG)
    A = _once(("handle", "big"), lambda: ctx.csr(n, n, rp, cc, cv))
    for scaled in (False, True):
        lo, hi, alpha, beta, done = ctx.lanczos(A, 4, scaled=scaled)
        ta, tb, tdone, tlo, thi = _twin_lanczos(pkg, n, rp, cc, cv, scaled, 4)
        dev = max(np.max(np.abs(alpha - ta)), np.max(np.abs(beta - tb))) / thi
        print(f"n = {n}, scaled {scaled}: coefficients within {dev:.3e}")
        assert done == tdone == 4 and dev <= ol.REL_TOL and abs(hi - thi) <= ol.REL_TOL * thi and abs(lo - tlo) <= ol.REL_TOL * thi


# ---- 5. the smoother ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", (1, 3, 8))
def test_the_smoother_contracts_the_error_and_follows_the_twin(ctx, degree):
    n, rp, cc, cv = _matrix("laplacian32x32", 0)
    lmin, lmax = cr.laplacian_2d_bounds(32)
    mv = _mv(n, rp, cc, cv)
    rng = np.random.default_rng(41)
    exact, x0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    b_host = mv(exact)
    solution = _once(("solution", "lap32"), lambda: exact + np.linalg.solve(_dense(n, rp, cc, cv), b_host - mv(exact)))
    A = ctx.csr(n, n, rp, cc, cv)
    ctx.chebyshev_setup(A, degree, scaled=False, lmin=lmin, lmax=lmax)
    c0, c1, c2 = cr.coefficients(degree, lmin, lmax)
    bound = cr.contraction(degree, lmin, lmax)
    for aligned in ((True, True), (False, False)):
        b, keep_b = _device_vector(ctx, b_host, aligned[0])
        x, keep_x = _device_vector(ctx, x0, aligned[1])
        twin = x0
        for call in range(3):
            before = np.linalg.norm(x.download() - solution)
            ctx.chebyshev(A, b, x)
            ctx.sync()
            got = x.download()
            ratio = np.linalg.norm(got - solution) / before
            twin = cr.smooth(mv, None, b_host, twin, c0, c1, c2)
            print(f"degree {degree}, call {call}: the error contracts by {ratio:.6e}, bound 1 / T_{degree + 1}(sigma) = {bound:.6e}")
            assert ratio <= bound * (1 + 1e-12)
            _close(got, twin, f"degree {degree}, aligned {aligned}, call {call}: x against the twin's")
        assert b.download().tobytes() == b_host.tobytes()


def _dense(n, rp, cc, cv):
    dense = np.zeros((n, n))
    np.add.at(dense, (np.repeat(np.arange(n), np.diff(rp)), cc), cv)
    return dense


# ---- 6. the solvers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", cr.DEGREES)
@pytest.mark.parametrize("system", list(cr.SYSTEMS))
def test_preconditioned_solvers_take_the_iterations_of_the_twins(ctx, pkg, system, degree):
    capi = pkg.capi
    solver, n, rp, cc, cv, b_host = cr.solver_system(system)
    A = ctx.csr(n, n, rp, cc, cv)
    A.set_param("cheby_degree", degree)
    b, x = ctx.vector_from(b_host), ctx.vector(n)
    solve = {"cg": ctx.cg, "bicgstab": ctx.bicgstab, "gmres": ctx.gmres}[solver]
    x.fill(0.0)
    iters, res = solve(A, b, x, max_iter=2000, rel_tol=cr.REL_TOL, precond=capi.PRECOND_CHEBYSHEV)
    assert ctx.chebyshev_info(A) == (degree, True, 2.0 / 30.0, 2.0), "the solver's own set-up: the defaults"
    mv = _mv(n, rp, cc, cv)
    true = np.linalg.norm(b_host - mv(x.download())) / np.linalg.norm(b_host)
    twin_x, twin_iters = cr.run_twin(system, degree)
    twin_true = np.linalg.norm(b_host - mv(twin_x)) / np.linalg.norm(b_host)
    x.fill(0.0)
    plain = solve(A, b, x, max_iter=2000, rel_tol=cr.REL_TOL)[0]
    print(f"{system} degree {degree}: {iters} iterations (twin {twin_iters}, recorded {cr.TWIN_ITERATIONS[system, degree]}), plain {plain} "
          f"(twin {cr.UNPRECONDITIONED_ITERATIONS[system]}), reported {res:.3e}, true {true:.3e} (twin's {twin_true:.3e})")
    assert twin_iters == cr.TWIN_ITERATIONS[system, degree]
    assert abs(iters - twin_iters) <= 1, (iters, twin_iters)
    assert 2 * iters < plain, (iters, plain)
    assert res <= cr.REL_TOL and true <= solver_ref.F * max(cr.REL_TOL, twin_true), (res, true, twin_true)
    # a handle that was set up explicitly is used as it stands
    ctx.chebyshev_setup(A, 2, lmin=0.1, lmax=2.0)
    x.fill(0.0)
    solve(A, b, x, max_iter=2000, rel_tol=cr.REL_TOL, precond=capi.PRECOND_CHEBYSHEV)
    assert ctx.chebyshev_info(A) == (2, True, 0.1, 2.0)


def test_solvers_on_other_formats_and_refusals(ctx, pkg):
    capi = pkg.capi
    solver, n, rp, cc, cv, b_host = cr.solver_system("cg_laplacian12")
    E = ctx.csr_to_ell(ctx.csr(n, n, rp, cc, cv))
    b, x = ctx.vector_from(b_host), ctx.vector(n)
    x.fill(0.0)
    with pytest.raises(capi.SpmvError) as e:  # not set up: the set-up's own error
        ctx.cg(E, b, x, precond=capi.PRECOND_CHEBYSHEV)
    assert e.value.code == INVALID and "CSR" in str(e.value)
    ctx.chebyshev_setup(E, 4, scaled=False, lmin=12.0 / 30.0, lmax=12.0)
    for solve in (ctx.cg, ctx.bicgstab, ctx.gmres):
        x.fill(0.0)
        iters, res = solve(E, b, x, max_iter=500, rel_tol=cr.REL_TOL, precond=capi.PRECOND_CHEBYSHEV)
        true = np.linalg.norm(b_host - ir.csr_mv(n, rp, cc, cv, x.download())) / np.linalg.norm(b_host)
        print(f"ELL, {solve.__name__}: {iters} iterations, reported {res:.3e}, true {true:.3e}")
        assert res <= cr.REL_TOL and true <= solver_ref.F * cr.REL_TOL and iters <= cr.TWIN_ITERATIONS["cg_laplacian12", 4] + 1
    with pytest.raises(capi.SpmvError) as e:
        ctx.cg_multi(E, ctx.vector(2 * n), ctx.vector(2 * n), 2, precond=capi.PRECOND_CHEBYSHEV)
    assert e.value.code == UNSUPPORTED and "Chebyshev" in str(e.value)
    with pytest.raises(capi.SpmvError) as e:
        ctx.cg(E, b, x, precond=7)
    assert e.value.code == INVALID and "unknown preconditioner" in str(e.value)


def test_cg_with_an_upper_bound_that_is_too_small_returns(ctx, pkg):
    """lmax a quarter of the row bound: the polynomial is indefinite on part of the spectrum; spmv_cg reports r.M^-1 r <= 0 or
    converges, and returns either way (the kernels run in bounds whatever the bounds of the spectrum are)"""
    capi = pkg.capi
    solver, n, rp, cc, cv, b_host = cr.solver_system("cg_laplacian12")
    A = ctx.csr(n, n, rp, cc, cv)
    ctx.chebyshev_setup(A, 4, lmax=0.5)
    b, x = ctx.vector_from(b_host), ctx.vector(n)
    x.fill(0.0)
    try:
        iters, res = ctx.cg(A, b, x, max_iter=500, rel_tol=cr.REL_TOL, precond=capi.PRECOND_CHEBYSHEV)
        print(f"returned after {iters} iterations at {res:.3e}")
    except capi.SpmvError as e:
        print("refused:", e)
        assert e.code == INVALID
