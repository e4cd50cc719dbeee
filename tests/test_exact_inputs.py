"""The exact-input method of tests/exact.py, checked against the oracle on the CPU (no GPU).

On dyadic inputs within the 2^53 budget the oracle's CSR / CSC / COO / ELL / DIA products, in both fma flavours and in any
order of the entries, equal exact_product bit for bit; the budget guard raises where it must; a result with one term left out
passes the parity gate and fails the exact comparison; poisoning the x entries nobody reads changes nothing.
"""
import numpy as np
import pytest

import exact as ex
import oracle_lib as ol


def _random_coo(rng, nrow, ncol, nnz):
    return rng.integers(0, nrow, nnz).astype(np.int32), rng.integers(0, ncol, nnz).astype(np.int32)


@pytest.mark.parametrize("seed", range(8))
def test_oracle_products_equal_the_integer_sum(orc, seed):
    rng = np.random.default_rng(100 + seed)
    nrow, ncol = int(rng.choice([1, 7, 300, 2000])), int(rng.choice([1, 5, 400, 3000]))
    nnz = int(rng.choice([0, 1, 50, 6000]))
    row, col = _random_coo(rng, nrow, ncol, nnz)
    if nnz > 10:
        row[: nnz // 4] = row[0]  # a long row
    terms = max(ex.max_terms(row, nrow), ex.max_terms(col, ncol))
    bits, e = ex.choose_bits(terms, reps=2)
    val = ex.dyadic(rng, nnz, bits, e)
    val[rng.random(nnz) < 0.05] = 0.0  # explicit zeros
    x, xt = ex.dyadic(rng, ncol, bits, e), ex.dyadic(rng, nrow, bits, e)
    y0, yt0 = ex.dyadic(rng, nrow, bits, e), ex.dyadic(rng, ncol, bits, e)
    want = ex.exact_product(nrow, row, col, val, x, e, y0=y0, reps=2)
    want_t = ex.exact_product(ncol, *ex.transposed((row, col, val)), xt, e, y0=yt0, reps=2)

    def twice(fn, y):
        y = y.copy()
        fn(y)
        fn(y)
        return y

    rp, cc, cv = ol.coo_to_csr(orc, nrow, row, col, val)
    cp, cr, cw = ol.coo_to_csc(orc, ncol, row, col, val)
    assert np.array_equal(ex.exact_product(nrow, *ex.csr_entries(rp, cc, cv), x, e, y0=y0, reps=2), want)
    assert np.array_equal(ex.exact_product(nrow, *ex.csc_entries(cp, cr, cw), x, e, y0=y0, reps=2), want)
    for fma in (False, True):
        assert np.array_equal(twice(lambda y: ol.csr_spmv(orc, rp, cc, cv, x, y, fma=fma), y0), want), ("csr", fma)
        assert np.array_equal(twice(lambda y: ol.csc_spmv(orc, cp, cr, cw, x, y, fma=fma), y0), want), ("csc", fma)
        for _ in range(3):  # COO: the entries in shuffled orders
            p = rng.permutation(nnz)
            r, c, v = ol.i32(row[p]), ol.i32(col[p]), ol.f64(val[p])
            assert np.array_equal(twice(lambda y: ol.coo_spmv(orc, r, c, v, x, y, fma=fma), y0), want), ("coo", fma)
        # the transposed product: the same arrays with rows and columns swapped
        assert np.array_equal(twice(lambda y: ol.csc_spmv(orc, rp, cc, cv, xt, y, fma=fma), yt0), want_t), ("csr^T", fma)
        assert np.array_equal(twice(lambda y: ol.csr_spmv(orc, cp, cr, cw, xt, y, fma=fma), yt0), want_t), ("csc^T", fma)
        assert np.array_equal(twice(lambda y: ol.coo_spmv(orc, ol.i32(col), ol.i32(row), ol.f64(val), xt, y, fma=fma), yt0), want_t)
    # ELL (padding included: column 0, value 0) and its slot list
    k, ec, ev = ol.coo_to_ell(orc, nrow, row, col, val)
    ent = ex.ell_entries(nrow, k, ec, ev)
    assert np.array_equal(ex.exact_product(nrow, *ent, x, e, y0=y0, reps=2), want)
    for fma in (False, True):
        assert np.array_equal(twice(lambda y: ol.ell_spmv(orc, nrow, k, ec, ev, x, y, fma=fma), y0), want), ("ell", fma)
        slot_rows = ol.i32(ent[0])
        wt = ex.exact_product(ncol, *ex.transposed(ent), xt, e, y0=yt0, reps=2)
        assert np.array_equal(twice(lambda y: ol.coo_spmv(orc, ec, slot_rows, ev, xt, y, fma=fma), yt0), wt), ("ell^T", fma)


@pytest.mark.parametrize("seed", range(6))
def test_oracle_dia_equals_the_integer_sum(orc, seed):
    rng = np.random.default_rng(200 + seed)
    nrow = int(rng.choice([1, 17, 256, 1000]))
    ncol = int(rng.choice([nrow, max(1, nrow // 2), nrow + 30]))
    span = int(rng.choice([2, 40, max(2, nrow)]))
    offs = ol.i32(np.sort(rng.choice(np.arange(-span, span + 1), size=min(int(rng.integers(1, 12)), 2 * span + 1), replace=False)))
    bits, e = ex.choose_bits(len(offs), reps=1)
    val = ex.dyadic(rng, nrow * len(offs), bits, e)
    x, y0 = ex.dyadic(rng, ncol, bits, e), ex.dyadic(rng, nrow, bits, e)
    ent = ex.dia_entries(nrow, ncol, offs, val)
    want = ex.exact_product(nrow, *ent, x, e, y0=y0)
    # the oracle reads x[i + off_d] for every in-range j < nrow: x beyond the forward column bound padded with zeros
    jmax = min(nrow, ncol)
    xpad = np.zeros(max(nrow, ncol) + 1)
    xpad[:jmax] = x[:jmax]
    for fma in (False, True):
        y = y0.copy()
        ol.dia_spmv(orc, nrow, offs, val, xpad, y, fma=fma)
        assert np.array_equal(y, want), fma
    # the terms in (j, d) order of the transposed product: the same entry list swapped
    xt, yt0 = ex.dyadic(rng, nrow, bits, e), ex.dyadic(rng, ncol, bits, e)
    r, c, v = ex.transposed(ent)
    y = yt0.copy()
    ol.coo_spmv(orc, ol.i32(r), ol.i32(c), ol.f64(v), xt, y, fma=True)
    assert np.array_equal(y, ex.exact_product(ncol, r, c, v, xt, e, y0=yt0))


def test_choose_bits_prefers_the_widest_range_and_keeps_the_budget():
    assert ex.choose_bits(1) == (6, 10)
    for terms, reps in ((1, 1), (64, 3), (3000, 2), (100_000, 1), (4_000_000, 1)):
        b, e = ex.choose_bits(terms, reps)
        assert terms * reps * 2.0 ** (2 * b + 4 * e) + 2.0 ** (b + 3 * e) < 2.0**53
        # nothing wider fits
        assert e == ex.E_MAX or terms * reps * 2.0 ** (2 + 4 * (e + 1)) >= 2.0**53
    # outputs of up to 600 terms x 3 calls span 2^40 between the smallest and the largest term; beyond, the smallest
    # term still sits below the parity gate (1e-10) of an output holding one largest term up to 30k terms
    assert ex.choose_bits(600, 3)[1] == 10
    for terms in (1, 64, 3000, 30_000):
        b, e = ex.choose_bits(terms, 3)
        assert (2**b - 1) ** 2 * 2.0 ** (4 * e) > 1e10, (terms, b, e)


def test_choose_bits_dot_keeps_the_whole_dot_within_the_budget():
    for total, nout, reps in ((1, 1, 1), (50, 7, 3), (6000, 300, 3), (400_000, 90_000, 3), (2_300_000, 600_000, 3), (3_000_001, 3_000_001, 1)):
        b, e = ex.choose_bits_dot(total, nout, reps)
        assert 2.0 ** (b + 2 * e) * (total * reps * 2.0 ** (2 * b + 4 * e) + nout * 2.0 ** (b + 3 * e)) < 2.0**53
        assert e <= ex.choose_bits(total, reps)[1]  # never a wider range than one output of that many terms may have
        assert e == ex.E_MAX or 2.0 ** (1 + 2 * (e + 1)) * (total * reps * 2.0 ** (2 + 4 * (e + 1)) + nout * 2.0 ** (1 + 3 * (e + 1))) >= 2.0**53
    with pytest.raises(ValueError):
        ex.choose_bits_dot(2**52, 1)


@pytest.mark.parametrize("seed", range(6))
def test_exact_dot_is_the_float64_sum_in_any_order(orc, seed):
    """w . (y0 + reps * A x) on inputs from choose_bits_dot: the integer sum, the oracle's dot (both flavours) and a float64 sum in
    shuffled orders, forward, reversed and pairwise, all return the same bits"""
    rng = np.random.default_rng(400 + seed)
    nrow, ncol = int(rng.choice([1, 7, 300, 20_000])), int(rng.choice([1, 5, 400, 3000]))
    nnz = int(rng.choice([0, 1, 50, 6000, 200_000]))
    reps = 3
    row, col = _random_coo(rng, nrow, ncol, nnz)
    bits, e = ex.choose_bits_dot(nnz, nrow, reps)
    val, x = ex.dyadic(rng, nnz, bits, e), ex.dyadic(rng, ncol, bits, e)
    y0, w = ex.dyadic(rng, nrow, bits, e), ex.dyadic(rng, nrow, bits, e)
    for y in (ex.exact_product(nrow, row, col, val, x, e), ex.exact_product(nrow, row, col, val, x, e, y0=y0, reps=reps)):
        want = ex.exact_dot(w, y, e, 2 * e)
        assert want == ol.dot(orc, w, y) == ol.dot(orc, w, y, fma=True)
        t = w * y
        assert want == float(np.sum(t)) == float(np.cumsum(t)[-1]) == float(np.cumsum(t[::-1])[-1])
        for _ in range(4):
            p = rng.permutation(nrow)
            assert want == float(np.cumsum(t[p])[-1]) == ol.dot(orc, ol.f64(w[p]), ol.f64(y[p]), fma=True)
        # 32 partial sums over interleaved rows, then their sum: the shape of the slotted accumulator
        assert want == float(sum(float(np.sum(t[s::32])) for s in range(32)))
    # one term left out changes the bits; a sum beyond the budget raises
    if nnz:
        y = ex.exact_product(nrow, row, col, val, x, e, y0=y0, reps=reps)
        less = y.copy()
        less[row[0]] -= val[0] * x[col[0]]
        assert ex.exact_dot(w, less, e, 2 * e) != ex.exact_dot(w, y, e, 2 * e)
    with pytest.raises(ValueError, match="budget"):
        ex.exact_dot(np.full(1 << 12, 2.0**20), np.full(1 << 12, 2.0**22), 0, 0)
    with pytest.raises(ValueError):
        ex.exact_dot(np.ones(3), np.array([1.0, np.nan, 1.0]), 0, 0)
    assert ex.exact_dot(np.zeros(0), np.zeros(0), 3, 6) == 0.0


def test_the_budget_guard_raises():
    # one output of 2^20 terms of 2^34 each (scaled by 2^2E): 2^54 > 2^53
    e = 10
    n = 1 << 20
    val = np.full(n, 2.0**7)
    x = np.full(4, 2.0**7)
    with pytest.raises(ValueError, match="budget"):
        ex.exact_product(1, np.zeros(n, np.int64), np.zeros(n, np.int64), val, x, e)
    # the same sum under the budget, accumulated over enough calls to pass it
    ok = ex.exact_product(1, np.zeros(1024, np.int64), np.zeros(1024, np.int64), val[:1024], x, e)
    assert ok[0] == 1024 * 2.0**14
    with pytest.raises(ValueError, match="budget"):
        ex.exact_product(1, np.zeros(1024, np.int64), np.zeros(1024, np.int64), val[:1024], x, e, reps=1 << 10)
    # a single product beyond 53 bits, and values off the grid
    with pytest.raises(ValueError):
        ex.exact_product(1, [0], [0], [2.0**20], [2.0**20], e)
    with pytest.raises(ValueError, match="dyadic"):
        ex.exact_product(1, [0], [0], [0.1], [1.0], e)
    with pytest.raises(ValueError):
        ex.exact_product(1, [0], [0], [1.0], [np.nan], e)
    with pytest.raises(ValueError):
        ex.choose_bits(2**60)


def test_the_exact_gate_sees_what_the_parity_gate_cannot(orc):
    """a row of one largest and one smallest term: leaving the smallest out passes ol.assert_parity and fails the exact comparison"""
    rng = np.random.default_rng(5)
    nrow, per = 200, 20
    bits, e = ex.choose_bits(per, reps=1)
    assert e == ex.E_MAX
    rp = (np.arange(nrow + 1) * per).astype(np.int32)
    cc = rng.integers(0, 1000, nrow * per).astype(np.int32)
    cv = ex.dyadic(rng, nrow * per, bits, e)
    x = ex.dyadic(rng, 1000, bits, e)
    cv[0], x[cc[0]] = 2.0**-e, 2.0**-e  # the smallest term: 2^-2E
    cv[1] = (2**bits - 1) * 2.0**e  # and a large one beside it
    x[cc[1]] = (2**bits - 1) * 2.0**e
    if cc[1] == cc[0]:
        cc[1] = (cc[0] + 1) % 1000
        x[cc[1]] = (2**bits - 1) * 2.0**e
    want = ex.exact_product(nrow, *ex.csr_entries(rp, cc, cv), x, e)
    got = np.zeros(nrow)
    ol.csr_spmv(orc, rp, cc, cv, x, got)
    assert np.array_equal(got, want)
    dropped = cv.copy()
    dropped[0] = 0.0  # one term left out
    bad = np.zeros(nrow)
    ol.csr_spmv(orc, rp, cc, dropped, x, bad)
    scale = np.zeros(nrow)
    ol.csr_abs_row_sums(orc, rp, cc, cv, x, scale)
    ol.assert_parity(bad, want, scale, "one smallest term dropped")  # the old gate does not see it
    assert not np.array_equal(bad, want)  # the new one does
    assert abs(bad[0] - want[0]) == 2.0 ** (-2 * e)


@pytest.mark.parametrize("seed", range(4))
def test_poisoned_x_leaves_the_oracle_unchanged(orc, seed):
    rng = np.random.default_rng(300 + seed)
    nrow, ncol, nnz = 500, 4000, 3000
    row, col = _random_coo(rng, nrow, ncol, nnz)
    col = ex.avoid_columns(col, ncol, panel_cols=(7000, 20_000)) if seed % 2 else col
    bits, e = ex.choose_bits(ex.max_terms(row, nrow))
    val = ex.dyadic(rng, nnz, bits, e)
    val[::37] = 0.0  # explicit zeros: their columns count as read
    x = ex.dyadic(rng, ncol, bits, e)
    xp = ex.poison(x, col)
    assert np.isnan(xp).sum() + np.isinf(xp).sum() == ncol - len(np.unique(col))
    if seed % 2:
        assert not np.isfinite(xp[0]) and not np.isfinite(xp[-1]) and not np.isfinite(xp[::16]).any()
    want = ex.exact_product(nrow, row, col, val, x, e)
    assert np.array_equal(ex.exact_product(nrow, row, col, val, xp, e), want)
    rp, cc, cv = ol.coo_to_csr(orc, nrow, row, col, val)
    cp, cr, cw = ol.coo_to_csc(orc, ncol, row, col, val)
    for fma in (False, True):
        for run in (lambda y: ol.csr_spmv(orc, rp, cc, cv, xp, y, fma=fma), lambda y: ol.coo_spmv(orc, row, col, val, xp, y, fma=fma),
                    lambda y: ol.csc_spmv(orc, cp, cr, cw, xp, y, fma=fma)):
            y = np.zeros(nrow)
            run(y)
            assert np.array_equal(y, want)
    # and a read of one poisoned entry shows: NaN where that column's row is
    y = np.zeros(nrow)
    bad = xp.copy()
    bad[col[0]] = np.inf if val[0] != 0.0 else bad[col[0]]
    ol.csr_spmv(orc, rp, cc, cv, bad, y)
    if val[0] != 0.0:
        assert not np.isfinite(y[row[0]])
