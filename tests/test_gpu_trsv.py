"""The triangular solves with a caller's matrix (spmv_trsv_*; csrc/sptrsv.hip) on the GPU: held to EQUALITY on the dyadic LU products
of tests/ilu0_ref.py - one and k right-hand sides, transposed, past one trip of the grid - to np.longdouble substitution on general
inputs, to spmv_ilu0_solve on ILU(0)'s own factors, and to their refusals and their hygiene.

The exact family: the combined LU array of an exact case (`expected`: duplicates, stored zeros, random order inside a row) uploaded on
the case's own pattern.  With r = A z, z integers, trsv(LOWER | UNIT) then trsv(UPPER) must return z: every term of every sum is on one
dyadic grid far inside 2^53 (trsv_ref.assert_trsv_budget; tests/test_trsv_ref.py checks every case on the CPU), so no lane tree and
no order of a sum moves a bit.  The cases cover 1, 4 and 16 lanes, folded runs from first_level = 2, levels with launches of their own
(cliques_mixed, cliques_tiny) and 5000 one-row levels (band_*).

A case's matrices, right-hand sides and references are computed once and shared.  test_every_case_ran asserts at the end that
every case ran."""
from collections import defaultdict

import numpy as np
import pytest

import ilu0_ref as ir
import oracle_lib as ol
import trsv_ref as tr

pytestmark = pytest.mark.gpu

L, U, UNIT, T = tr.TRSV_LOWER, tr.TRSV_UPPER, tr.TRSV_UNIT, tr.TRSV_TRANSPOSE
INVALID, UNSUPPORTED = -1, -5
EXACT_NAMES = list(ir.EXACT_CLIQUES) + list(ir.EXACT_BANDS)
TRANSPOSED_NAMES = ("band_3_3", "band_1_20", "cliques_12")
EXACT_KS = (1, 3, 8, 16, 17, 33, 64)
GENERAL_KS = (1, 2, 3, 5, 8, 16, 17, 64)
GENERAL = [(n, per_row) for n in (1, 2, 63, 64, 65, 257, 5000) for per_row in (1, 6, 40)] + [("laplacian", 3)]
RUNS = defaultdict(int)
RATIOS = {}
_CASE = {}


def _case(name):
    """(n, rp, cc, cv, expected, Z: 64 integer columns, column 0 the case's own z, R = A Z from the original values)"""
    if name not in _CASE:
        n, rp, cc, cv, expected, z = ir.exact_case(name)
        seed = (ir.EXACT_CLIQUES.get(name) or ir.EXACT_BANDS[name])[-1]
        Z = np.stack([ir.integer_vector(n, seed + c) for c in range(64)], axis=1)
        assert np.array_equal(Z[:, 0], z)
        R = np.stack([ir.csr_mv(n, rp, cc, cv, Z[:, c]) for c in range(64)], axis=1)
        _CASE[name] = (n, rp, cc, cv, expected, Z, R)
    return _CASE[name]


def _same(got, want, what):
    """equality by value (-0.0 == 0.0), the differences counted and the first ones shown"""
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    bad = np.flatnonzero(~(got == want))
    print(f"{what}: {len(bad)} of {len(want)} differ")
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())


def _solve(ctx, A, flags, b_host, in_place=False):
    b = ctx.vector_from(b_host)
    x = b if in_place else ctx.vector(len(b_host))
    if not in_place:
        x.fill(7.0)  # (whatever x holds is ignored)
    ctx.trsv_solve(A, b, x, flags)
    ctx.sync()
    return x.download()


def _solve_multi(ctx, A, flags, B_host, in_place=False):
    n, k = B_host.shape
    B = ctx.vector_from(np.ascontiguousarray(B_host).ravel())
    X = B if in_place else ctx.vector(n * k)
    if not in_place:
        X.fill(7.0)
    ctx.trsv_solve_multi(A, B, X, k, flags)
    ctx.sync()
    return X.download().reshape(n, k)


def _multi_launches(A):
    return A.get_param("trsv_multi_launches"), A.get_param("trsv_multi_level_launches")


# ---- 1. exact, bit for bit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EXACT_NAMES)
def test_exact_lu_solves(ctx, name):
    n, rp, cc, cv, expected, Z, R = _case(name)
    A = ctx.csr(n, n, rp, cc, expected)
    z, r = Z[:, 0], R[:, 0]
    got = _solve(ctx, A, U, _solve(ctx, A, L | UNIT, r))
    _same(got, z, f"{name}: out of place")
    again = _solve(ctx, A, U, _solve(ctx, A, L | UNIT, r))
    assert again.tobytes() == got.tobytes(), "two runs differ"
    in_place = _solve(ctx, A, U, _solve(ctx, A, L | UNIT, r, in_place=True), in_place=True)
    _same(in_place, z, f"{name}: in place")
    assert in_place.tobytes() == got.tobytes()
    # levels, lanes and launches: what the schedule rule makes of this pattern
    want = ir.level_sizes(n, rp, cc, order=np.arange(n), merged=False)
    infos = [ctx.trsv_info(A, L | UNIT), ctx.trsv_info(A, U)]
    assert ctx.trsv_info(A, L) == infos[0], "UNIT and non-UNIT solves share the analysis"
    for info, which, lanes in zip(infos, ("lower", "upper"), want["lanes"]):
        assert (info["levels"], info["lanes"], info["launches"]) == (len(want[which]), lanes, tr.launches(want[which], lanes)[0]), (info, which)
    assert infos[0]["launches"] + infos[1]["launches"] == want["launches"]
    assert A.get_param("trsv_ready") == 0b0011 and A.get_param("trsv_bytes") == infos[0]["bytes"] + infos[1]["bytes"]
    RUNS["exact"] += 1


# ---- 2. exact, k columns ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EXACT_NAMES)
def test_exact_lu_solves_of_k_columns(ctx, name):
    n, rp, cc, cv, expected, Z, R = _case(name)
    A = ctx.csr(n, n, rp, cc, expected)
    hist = ir.level_sizes(n, rp, cc, order=np.arange(n), merged=False)
    for k in EXACT_KS:
        width = tr.width_of(k)
        Y = _solve_multi(ctx, A, L | UNIT, R[:, :k])
        lower_launches = _multi_launches(A)
        X = _solve_multi(ctx, A, U, Y, in_place=(k == 17))
        upper_launches = _multi_launches(A)
        _same(X, Z[:, :k], f"{name}: k = {k}")
        want = tr.launches(hist["lower"], width), tr.launches(hist["upper"], width)
        print(f"{name} k = {k} (T = {width}): launches (all, own level) lower {lower_launches}, upper {upper_launches}")
        assert (lower_launches, upper_launches) == want, (k, want)
        if width == 16:
            if name == "cliques_tiny":
                assert hist["lower"][0] == 6000 and lower_launches[1] >= 1 and upper_launches[1] >= 1
            elif name == "cliques_mixed":
                assert tr.schedule(hist["lower"], 16)[:2] == [(0, 1), (1, 1)] and lower_launches[1] >= 2 and lower_launches[0] > lower_launches[1]
            elif name == "cliques_130" or name.startswith("band"):
                assert lower_launches == (1, 0) and upper_launches == (1, 0)
    RUNS["exact_multi"] += 1


# ---- 3. exact, transposed --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TRANSPOSED_NAMES)
def test_exact_transposed_solves(ctx, name):
    n, rp, cc, cv, expected, Z, R = _case(name)
    A = ctx.csr(n, n, rp, cc, expected)
    for flags in (L | UNIT | T, U | T, L | T, U | UNIT | T):
        ptr, col, val, diag, has, lower = tr.extract(n, rp, cc, expected, flags)
        unit = bool(flags & UNIT)
        bits, B = tr.assert_trsv_budget(n, ptr, col, val, diag, Z[:, :17], unit=unit)  # b = T^T x in integer arithmetic
        what = f"{name} {tr.flag_name(flags)} ({bits:.1f} bits)"
        _same(_solve(ctx, A, flags, B[:, 0]), Z[:, 0], what)
        _same(_solve(ctx, A, flags, B[:, 1], in_place=True), Z[:, 1], what + ", in place")
        for k in (1, 8, 17):
            _same(_solve_multi(ctx, A, flags, B[:, :k]), Z[:, :k], what + f", k = {k}")
        info = ctx.trsv_info(A, flags)
        hist = tr.level_hist(n, ptr, col, lower)
        lanes = tr.lanes_of(n, len(col))
        assert (info["levels"], info["lanes"], info["launches"]) == (len(hist), lanes, tr.launches(hist, lanes)[0]), info
    assert A.get_param("trsv_ready") == 0b1100
    RUNS["transposed"] += 1


# ---- 4. general inputs against np.longdouble ---------------------------------------------------------------------------------------
def _general_system(n, per_row):
    if n == "laplacian":
        return ir.laplacian_3d(12)
    return tr.random_system(n, per_row, 1000 * n + per_row)


@pytest.mark.parametrize("n,per_row", GENERAL, ids=[f"{n}-{p}" for n, p in GENERAL])
def test_general_inputs_against_longdouble(ctx, n, per_row):
    """every flag combination on one handle: the hard gate is oracle_lib.REL_TOL norm-wise against np.longdouble substitution; the
    error is also held to the rounding envelope of the three float64 twins (trsv_ref.ENVELOPE_*); every column of a k-column solve has
    the bits of the k = 1 solve of that column, and those of spmv_trsv_solve where that runs 1 lane"""
    what_n = n
    n, rp, cc, cv = _general_system(n, per_row)
    A = ctx.csr(n, n, rp, cc, cv)
    B = np.random.default_rng([n, per_row, 7]).uniform(-1, 1, (n, 64))
    for flags in tr.ALL_FLAGS:
        ptr, col, val, diag, has, lower = tr.extract(n, rp, cc, cv, flags)
        unit = bool(flags & UNIT)
        ref = tr.solve_longdouble(n, ptr, col, val, diag, lower, B[:, 0], unit)
        envelope = max(tr.rel_error(tr.solve_twin(n, ptr, col, val, diag, lower, B[:, 0], unit, lanes), ref) for lanes in (1, 4, 16))
        single = _solve(ctx, A, flags, B[:, 0])
        err = tr.rel_error(single, ref)
        ratio = err / max(envelope, tr.UNIT_ROUNDOFF)
        RATIOS[(what_n, per_row, flags)] = ratio
        info = ctx.trsv_info(A, flags)
        print(f"n = {what_n} per_row = {per_row} {tr.flag_name(flags)}: error {err:.3e}, envelope {envelope:.3e}, ratio {ratio:.3f}; "
              f"{info['levels']} levels, {info['lanes']} lane(s), {info['launches']} launch(es)")
        assert info["lanes"] == tr.lanes_of(n, len(col)) and info["levels"] == len(tr.level_hist(n, ptr, col, lower))
        assert err <= ol.REL_TOL, (tr.flag_name(flags), err)
        assert ratio <= tr.ENVELOPE_MEASURED * tr.ENVELOPE_SLACK, (tr.flag_name(flags), err, envelope, ratio)
        assert _solve(ctx, A, flags, B[:, 0], in_place=True).tobytes() == single.tobytes(), "in place differs"
        # the k-column solve: column by column the k = 1 solve
        ones = np.stack([_solve_multi(ctx, A, flags, B[:, c:c + 1])[:, 0] for c in range(64)], axis=1)
        assert tr.rel_error(ones[:, 0], ref) <= ol.REL_TOL
        if info["lanes"] == 1:
            assert ones[:, 0].tobytes() == single.tobytes(), "k = 1 differs from spmv_trsv_solve at 1 lane"
        for k in GENERAL_KS:
            X = _solve_multi(ctx, A, flags, B[:, :k], in_place=(k == 5))
            assert X.tobytes() == np.ascontiguousarray(ones[:, :k]).tobytes(), (tr.flag_name(flags), k, int(np.sum(X != ones[:, :k])))
    assert A.get_param("trsv_ready") == 0b1111
    RUNS["general"] += 1


# ---- 5. past one trip and past 256 workgroups ------------------------------------------------------------------------------------------
def test_a_million_rows_in_eight_levels(ctx):
    n, rp, cc, cv, x = tr.lower_bidiagonal_gaps(1_048_583)
    ptr, col, val, diag, has, lower = tr.extract(n, rp, cc, cv, L)
    X = np.stack([x, x[::-1], -2.0 * x], axis=1)
    bits, B = tr.assert_trsv_budget(n, ptr, col, val, diag, X, unit=False)
    A = ctx.csr(n, n, rp, cc, cv)
    _same(_solve(ctx, A, L, B[:, 0]), x, f"n = {n}: one right-hand side ({bits:.1f} bits)")
    info = ctx.trsv_info(A, L)
    assert (info["levels"], info["lanes"], info["launches"]) == (8, 1, 8), info  # 8 levels of 131,072 rows or more: 512 workgroups each
    _same(_solve_multi(ctx, A, L, B), X, f"n = {n}: k = 3")
    assert _multi_launches(A) == (8, 8)  # 4 lanes per row: 2048 workgroups a level
    RUNS["large"] += 1


# ---- 6. against ILU(0) -------------------------------------------------------------------------------------------------------------------
def test_the_factors_of_ilu0_solve_as_ilu0_does(ctx):
    n, rp, cc, cv = ir.laplacian_3d(12)
    A = ctx.csr(n, n, rp, cc, cv)
    A.set_param("ilu0_order", 0)
    F = ctx.csr(n, n, rp, cc, ctx.ilu0_factors(A))  # the combined LU array on A's own pattern
    r_host = np.random.default_rng(61).uniform(-1, 1, n)
    r, z = ctx.vector_from(r_host), ctx.vector(n)
    ctx.ilu0_solve(A, r, z)
    ctx.sync()
    want = z.download()
    got = _solve(ctx, F, U, _solve(ctx, F, L | UNIT, r_host))
    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
    print(f"trsv over ilu0_factors against ilu0_solve: {err:.3e}")
    assert err <= ol.REL_TOL
    RUNS["ilu0"] += 1


# ---- 7. refusals and state -------------------------------------------------------------------------------------------------------------
def test_refusals(ctx, pkg):
    capi = pkg.capi

    def expect(call, code, word):
        with pytest.raises(capi.SpmvError) as e:
            call()
        assert e.value.code == code and word in str(e.value), (code, word, e.value)

    n, rp, cc, cv = ir.tridiagonal_8()
    A = ctx.csr(n, n, rp, cc, cv)
    b, x = ctx.vector_from(np.ones(n)), ctx.vector(n)
    E = ctx.csr_to_ell(A)
    expect(lambda: ctx.trsv_setup(E, L), UNSUPPORTED, "CSR")
    expect(lambda: ctx.trsv_solve(E, b, x, L), UNSUPPORTED, "CSR")
    expect(lambda: ctx.trsv_solve_multi(E, ctx.vector(2 * n), ctx.vector(2 * n), 2, U), UNSUPPORTED, "CSR")
    R = ctx.csr(3, 4, np.arange(4, dtype=np.int32), np.array([0, 1, 2], np.int32), np.ones(3))
    expect(lambda: ctx.trsv_setup(R, L), INVALID, "square")
    expect(lambda: ctx.trsv_solve(R, ctx.vector(3), ctx.vector(3), L), INVALID, "square")
    S = ctx.csr_shard(4, 8, n, rp.astype(np.int64), cc, cv)  # rows 4..7 of the 8 x 8 matrix
    expect(lambda: ctx.trsv_setup(S, U), INVALID, "square")
    nb = 1_000_000
    P = ctx.gen_csr_uniform(0, nb, nb, 16, seed=31)
    P.set_kernel(capi.CSR_PANEL)
    P.set_param("panel_keep_csr", 0)
    assert P.get_param("panel_keep_csr") == 0
    expect(lambda: ctx.trsv_setup(P, L | UNIT), INVALID, "arrays")
    expect(lambda: ctx.trsv_solve(P, ctx.vector(nb), ctx.vector(nb), L | UNIT), INVALID, "arrays")
    # vectors, k, flags
    expect(lambda: ctx.trsv_solve(A, b, ctx.vector(n + 1), L), INVALID, "entries")
    expect(lambda: ctx.trsv_solve(A, ctx.vector(n - 1), x, L), INVALID, "entries")
    expect(lambda: ctx.trsv_solve_multi(A, ctx.vector(2 * n), ctx.vector(3 * n), 2, L), INVALID, "entries")
    for k in (0, 65, -1):
        expect(lambda: ctx.trsv_solve_multi(A, ctx.vector(n * max(k, 0)), ctx.vector(n * max(k, 0)), k, L), INVALID, "k =")
    big = ctx.vector(4 * n)
    part = ctx.wrap_vector(big.device_ptr + 8 * 3, n)  # entries 3 .. 3 + n of big
    head = ctx.wrap_vector(big.device_ptr, n)
    expect(lambda: ctx.trsv_solve(A, head, part, L), INVALID, "overlap")
    expect(lambda: ctx.trsv_solve_multi(A, ctx.wrap_vector(big.device_ptr, 2 * n), ctx.wrap_vector(big.device_ptr + 8 * n, 2 * n), 2, L), INVALID, "overlap")
    for flags in (8, 16, 1 << 31, 0xFFFFFFF8):
        expect(lambda: ctx.trsv_setup(A, flags), INVALID, "flag")
        expect(lambda: ctx.trsv_solve(A, b, x, flags), INVALID, "flag")
        expect(lambda: ctx.trsv_solve_multi(A, b, x, 1, flags), INVALID, "flag")
        expect(lambda: ctx.trsv_info(A, flags), INVALID, "flag")
    expect(lambda: ctx.trsv_info(A, L), INVALID, "not set up")
    assert A.get_param("trsv_ready") == 0 and A.get_param("trsv_bytes") == 0, "a refused call left state behind"
    other = capi.Context(0)
    expect(lambda: other.trsv_setup(A, L), INVALID, "context")
    expect(lambda: other.trsv_solve(A, b, x, L), INVALID, "context")
    other.close()
    RUNS["refusals"] += 1


def test_diagonals_that_only_unit_solves_take(ctx, pkg):
    """a zero diagonal (its two stored parts cancel) in row 5 and a missing one in row 3: the set-up without UNIT names the smallest
    such row and leaves nothing behind; the same handle solves with UNIT, and goes on refusing without"""
    capi = pkg.capi
    n, rp, cc, cv = tr.random_system(65, 6, 77)
    rows = np.repeat(np.arange(n), np.diff(rp))
    cv = cv.copy()
    on5 = np.flatnonzero((rows == 5) & (cc == 5))
    cv[on5] = [0.5, -0.5]
    for bad_row, (rp2, cc2, cv2) in ((5, (rp, cc, cv)), (3, _without_diagonal(n, rp, cc, cv, 3))):
        A = ctx.csr(n, n, rp2, cc2, cv2)
        before = A.get_param("device_bytes")
        for flags in (L, U, L | T, U | T):
            with pytest.raises(capi.SpmvError) as e:
                ctx.trsv_setup(A, flags)
            assert e.value.code == INVALID and f"row {bad_row}" in str(e.value) and "diagonal" in str(e.value), e.value
            assert A.get_param("trsv_ready") == 0 and A.get_param("trsv_bytes") == 0 and A.get_param("device_bytes") == before
        with pytest.raises(capi.SpmvError) as e:
            ctx.trsv_solve(A, ctx.vector(n), ctx.vector(n), U)
        assert e.value.code == INVALID and f"row {bad_row}" in str(e.value)
        b = np.random.default_rng(5).uniform(-1, 1, n)
        for flags in (L | UNIT, U | UNIT | T):
            ptr, col, val, diag, has, lower = tr.extract(n, rp2, cc2, cv2, flags)
            assert tr.bad_diagonal_row(diag, has) == bad_row
            ref = tr.solve_longdouble(n, ptr, col, val, diag, lower, b, True)
            assert tr.rel_error(_solve(ctx, A, flags, b), ref) <= ol.REL_TOL
        assert A.get_param("trsv_ready") == 0b1001
        with pytest.raises(capi.SpmvError) as e:  # the analysis is there; the diagonal still is not
            ctx.trsv_solve(A, ctx.vector(n), ctx.vector(n), L)
        assert e.value.code == INVALID and f"row {bad_row}" in str(e.value)
        assert A.get_param("trsv_ready") == 0b1001
    RUNS["diagonals"] += 1


def _without_diagonal(n, rp, cc, cv, row):
    rows = np.repeat(np.arange(n), np.diff(rp))
    keep = ~((rows == row) & (cc == row))
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int32)
    return rp2, cc[keep], cv[keep]


def test_no_rows(ctx):
    E = ctx.csr(0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    for flags in tr.ALL_FLAGS:
        ctx.trsv_setup(E, flags)
        ctx.trsv_solve(E, ctx.vector(0), ctx.vector(0), flags)
        ctx.trsv_solve_multi(E, ctx.vector(0), ctx.vector(0), 3, flags)
    ctx.sync()
    assert E.get_param("trsv_ready") == 0 and E.get_param("trsv_bytes") == 0
    RUNS["no_rows"] += 1


def test_a_setup_leaves_the_other_states_alone(ctx):
    n, rp, cc, cv = ir.laplacian_3d(12)
    A = ctx.csr(n, n, rp, cc, cv)
    A.set_param("ilu0_order", 0)
    ctx.ilu0_setup(A)
    ctx.symgs_order(A)
    x_host = np.random.default_rng(71).uniform(-1, 1, n)

    def snapshot():
        x, y = ctx.vector_from(x_host), ctx.vector(n)
        y.fill(0.0)
        ctx.apply(A, x, y)
        r, z = ctx.vector_from(x_host), ctx.vector(n)
        ctx.ilu0_solve(A, r, z)
        ctx.sync()
        params = {p: A.get_param(p) for p in ("ilu0_ready", "ilu0_bytes", "ilu0_launches", "symgs_launches", "symgs_colours", "symgs_bytes",
                                              "symgs_levels_forward", "symgs_levels_backward", "transpose_ready")}
        return y.download().tobytes(), z.download().tobytes(), A.get_plan(), params, A.info.kernel

    before, bytes_before = snapshot(), A.get_param("device_bytes")
    assert A.get_param("trsv_ready") == 0 and A.get_param("trsv_bytes") == 0
    total = 0
    for i, flags in enumerate((L, U | UNIT, L | T | UNIT, U | T)):
        ctx.trsv_setup(A, flags)
        ctx.trsv_setup(A, flags ^ UNIT)  # idempotent, and shared by UNIT and non-UNIT
        total += ctx.trsv_info(A, flags)["bytes"]
        assert A.get_param("trsv_ready") == (1 << (i + 1)) - 1
        assert A.get_param("trsv_bytes") == total and A.get_param("device_bytes") == bytes_before + total
    assert snapshot() == before
    assert A.info.device_bytes == bytes_before + total
    RUNS["state"] += 1


# ---- 8. coverage -----------------------------------------------------------------------------------------------------------------------
def test_every_case_ran():
    expect = {"exact": len(EXACT_NAMES), "exact_multi": len(EXACT_NAMES), "transposed": len(TRANSPOSED_NAMES), "general": len(GENERAL), "large": 1,
              "ilu0": 1, "refusals": 1, "diagonals": 1, "no_rows": 1, "state": 1}
    if any(RUNS[k] != c for k, c in expect.items()):
        pytest.skip(f"the coverage check needs every test of this module (ran {dict(RUNS)}, expected {expect})")
    assert set(_CASE) == set(ir.EXACT_CLIQUES) | set(ir.EXACT_BANDS)
    assert len(RATIOS) == 8 * len(GENERAL)
    print(f"largest engine error / envelope over {len(RATIOS)} general solves: {max(RATIOS.values()):.3f} at {max(RATIOS, key=RATIOS.get)}")
