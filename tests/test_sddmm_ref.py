"""The NumPy twins of spmv_sddmm (tests/sddmm_ref.py) against a dense U @ V.T sampled on the pattern, and against each other on dyadic
inputs."""
import numpy as np
import pytest

import exact
import sddmm_ref as sr


def random_pattern(rng, nrow, ncol, max_len):
    """CSR pattern with row lengths 0 .. max_len, the first and last row empty, columns ascending and distinct"""
    lens = rng.integers(0, max_len + 1, size=nrow)
    lens[0] = lens[-1] = 0
    rp = np.zeros(nrow + 1, np.int32)
    rp[1:] = np.cumsum(lens)
    col = np.concatenate([np.sort(rng.choice(ncol, size=n, replace=False)) for n in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    return rp, col


@pytest.mark.parametrize("k", [1, 3, 8, 17])
@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (-2.0, 0.5), (0.5, -1.0)])
def test_twins_equal_the_dense_product_sampled_on_the_pattern(k, alpha, beta):
    rng = np.random.default_rng(100 + k)
    nrow, ncol = 37, 29
    rp, col = random_pattern(rng, nrow, ncol, 12)
    U, V, out0, e = sr.dyadic_inputs(rng, nrow, ncol, len(col), k)
    rows = sr.entry_rows(rp)
    dense = U @ V.T  # exact: every partial sum of dyadic products stays below 2^53 on the grid
    want = alpha * dense[rows, col] + (beta * out0 if beta != 0.0 else 0.0)
    got = sr.sddmm_exact(rp, col, U, V, e, alpha, beta, out0)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    ld, mag = sr.sddmm_longdouble(rp, col, U, V, alpha, beta, out0)
    assert np.array_equal(ld.astype(np.float64), want)  # int64 and longdouble agree on dyadic inputs
    assert np.all(mag >= np.abs(ld))


def test_longdouble_twin_on_rounded_inputs_and_beta_zero_ignores_out0():
    rng = np.random.default_rng(5)
    nrow, ncol, k = 20, 31, 6
    rp, col = random_pattern(rng, nrow, ncol, 9)
    U, V = rng.uniform(-1, 1, (nrow, k)), rng.uniform(-1, 1, (ncol, k))
    rows = sr.entry_rows(rp)
    ld, mag = sr.sddmm_longdouble(rp, col, U, V, 1.5, 0.0, np.full(len(col), np.nan))
    want = 1.5 * (U @ V.T)[rows, col]
    assert np.all(np.isfinite(ld.astype(np.float64)))
    assert np.all(np.abs(ld.astype(np.float64) - want) <= (k + 3) * 2.0**-53 * mag.astype(np.float64))


def test_one_dimensional_inputs_mean_k_1_and_empty_patterns_work():
    rng = np.random.default_rng(6)
    rp, col = random_pattern(rng, 9, 7, 5)
    U, V, out0, e = sr.dyadic_inputs(rng, 9, 7, len(col), 1)
    a = sr.sddmm_exact(rp, col, U[:, 0], V[:, 0], e)
    assert np.array_equal(a, U[sr.entry_rows(rp), 0] * V[col, 0])
    assert sr.sddmm_exact(np.zeros(4, np.int32), np.zeros(0, np.int32), U[:3], V, e).shape == (0,)


def test_exact_twin_refuses_what_is_not_exact():
    rp, col = np.array([0, 1], np.int32), np.array([0], np.int32)
    with pytest.raises(ValueError):
        sr.sddmm_exact(rp, col, np.array([[1.0]]), np.array([[1.0]]), 2, alpha=3.0)
    with pytest.raises(ValueError):
        sr.sddmm_exact(rp, col, np.array([[0.1]]), np.array([[1.0]]), 2)
    big = np.array([[2.0**26]])
    with pytest.raises(ValueError):
        sr.sddmm_exact(rp, col, big, big, 1)
    assert exact.choose_bits(terms=8 * 64)[0] >= 1
