"""The NumPy twin of single-precision value storage (tests/csr_f32_ref.py) held to facts that need no GPU: dyadic values demote
without a change, widening a demoted array and demoting again changes nothing, the statistics on a hand-made array with one value of
each class, the entry word, and the arithmetic of refinement on the scaled Laplacian the GPU tests use."""
import numpy as np
import pytest

import csr_f32_ref as ref
import exact


def test_dyadic_values_demote_without_a_change():
    rng = np.random.default_rng(1)
    for bits, e in ((exact.B_MAX, exact.E_MAX), (10, 20), (1, 0), exact.choose_bits(1000)):
        v = exact.dyadic(rng, 5000, bits, e)  # at most 10 mantissa bits, exponents within +-20: floats, every one
        f, inexact, under, rel = ref.demote(v)
        assert (inexact, under, rel) == (0, 0, 0.0) and f.dtype == np.float32 and np.array_equal(ref.widen(f), v)


def test_widening_a_demoted_array_is_idempotent():
    rng = np.random.default_rng(2)
    v = rng.standard_normal(10000) * np.ldexp(1.0, rng.integers(-30, 31, size=10000))
    f, inexact, under, rel = ref.demote(v)
    assert inexact > 9900 and under == 0 and 2.0**-26 < rel <= 2.0**-24  # half an ulp of a 24-bit significand at the most
    g, again, under2, rel2 = ref.demote(ref.widen(f))
    assert np.array_equal(g.view(np.uint32), f.view(np.uint32)) and (again, under2, rel2) == (0, 0, 0.0)


def test_statistics_on_one_value_of_each_class():
    flt_max, flt_min, true_min = float(np.finfo(np.float32).max), ref.FLT_MIN, 2.0**-149
    v = np.array([1.5,                  # exact
                  0.0, -0.0,            # zeros stay, and count as nothing
                  1.0 + 2.0**-30,       # inexact: rounds to 1.0, relative change 2^-30 / (1 + 2^-30)
                  -(1.0 + 3 * 2.0**-24),  # inexact: a tie at half an ulp goes to the even neighbour 1 + 2^-22
                  1e-46,                # underflow to zero (and changed)
                  true_min,             # a subnormal float: underflow, unchanged
                  flt_min * (1 - 2.0**-30),  # just under FLT_MIN: rounds UP to FLT_MIN - a normal float: inexact, no underflow
                  1e-40,                # underflow to a subnormal (and changed)
                  flt_max, -flt_min])   # exact at both ends of the normal range
    f, inexact, under, rel = ref.demote(v)
    assert inexact == 5 and under == 3
    assert f[3] == np.float32(1.0) and f[4] == np.float32(-(1.0 + 2.0**-22)) and f[5] == 0.0 and f[7] == np.float32(flt_min)
    assert np.signbit(f[2]) and not np.signbit(f[1])
    assert rel == max(2.0**-30 / (1.0 + 2.0**-30), 2.0**-24 / (1.0 + 3 * 2.0**-24), (flt_min - v[7]) / v[7])
    # the overflow rule: FLT_MAX + half an ulp is the first double that rounds to inf; just below it rounds to FLT_MAX
    first_inf = flt_max + 2.0**103
    assert ref.demote(np.array([np.nextafter(first_inf, 0.0)]))[0][0] == np.float32(flt_max)
    for bad in (first_inf, -first_inf, 1e39, np.inf, -np.inf, np.nan):
        with pytest.raises(ValueError, match="1 values .* entry 2"):
            ref.demote(np.array([1.0, 2.0, bad, 3.0]))
    with pytest.raises(ValueError, match="2 values .* entry 0"):
        ref.demote(np.array([np.nan, 2.0, 1e39]))


def test_the_entry_word_keeps_column_and_sign_apart():
    cols = np.array([0, 1, 2**31 - 1, 7, 123456789], dtype=np.int32)
    vals = np.array([-0.0, -1.5, -float(np.finfo(np.float32).max), 2.0**-149, 3.25], dtype=np.float32)
    w = ref.pack(cols, vals)
    assert w.dtype == np.uint64 and int(w[1]) == (0xBFC00000 << 32) | 1 and int(w[0]) == 0x80000000 << 32
    c, v = ref.unpack(w)
    assert np.array_equal(c, cols) and np.array_equal(v.view(np.uint32), vals.view(np.uint32))


def test_product_of_the_widened_values_in_long_double():
    rp, col = np.array([0, 2, 2, 3], np.int32), np.array([1, 0, 2], np.int32)
    f = np.array([0.1, -2.0, 3.0], np.float32)
    x, y0 = np.array([1.0, 10.0, 100.0]), np.array([1.0, 2.0, 3.0])
    y = ref.product(rp, col, f, x, y0)
    assert y.dtype == np.longdouble and y[1] == 2.0 and y[2] == 303.0
    assert y[0] == np.longdouble(1.0) + np.longdouble(float(np.float32(0.1))) * 10 - 2  # the FLOAT 0.1, widened
    s, t = ref.abs_product(rp, col, f, x)
    assert list(t) == [2, 0, 1] and s[2] == 300.0


def test_refinement_reaches_fp64_accuracy_where_the_rounded_matrix_alone_stalls():
    n, rp, col, val = ref.scaled_laplacian()
    A = ref.dense(n, n, rp, col, val)
    f, inexact, under, rel = ref.demote(val)
    assert inexact > 0.99 * len(val) and under == 0
    A32 = ref.dense(n, n, rp, col, ref.widen(f))
    assert np.array_equal(A32, A32.T)  # d_i * d_j rounds the same way on both sides
    assert 100 < np.linalg.cond(A) < 5000
    b = np.random.default_rng(11).standard_normal(n)
    nb = np.linalg.norm(b)
    # the rounded matrix alone: its solution misses the true system by about cond * 2^-24
    x = np.zeros(n)
    ref.cg(A32, b, x, 1e-13, 5000)
    alone = np.linalg.norm(b - A @ x) / nb
    assert 1e-9 < alone < 1e-5, alone
    # refinement: fp64 residual, corrections from the rounded matrix
    x = np.zeros(n)
    outer, inner, res = ref.refine(A, A32, b, x, 1e-4, 1e-12, 20, 1000)
    true = np.linalg.norm((b.astype(np.longdouble) - A.astype(np.longdouble) @ x.astype(np.longdouble)).astype(np.float64)) / nb
    assert res <= 1e-12 and true <= 1e-12 and 2 <= outer <= 5, (outer, inner, res, true)
    plain = ref.cg(A, b, np.zeros(n), 1e-12, 5000)
    assert plain < inner < 3 * plain, (plain, inner)
    # the edges of the loop: b = 0, one outer step, A_lo = A
    x1 = np.ones(n)
    assert ref.refine(A, A32, np.zeros(n), x1, 1e-4, 1e-12, 20, 1000) == (0, 0, 0.0) and np.all(x1 == 1.0)
    assert ref.refine(A, A32, b, np.zeros(n), 1e-4, 1e-12, 1, 1000)[0] == 1
    assert ref.refine(A, A, b, np.zeros(n), 1e-12, 1e-11, 20, 5000)[0] == 1


def test_demotion_and_its_statistics_commute_with_block_diagonal_copies():
    """the oracle of tests/tiled.py for csrc/convert_f32.hip: the rounding is entry by entry, so k copies demote and widen to the
    base's bytes tiled; the counts are k times the base's and the largest relative change is the base's; one value of the last
    copy can raise it.  And the coverage conditions of the GPU cases (tests/test_gpu_csr_f32.py) hold for their k."""
    import tiled

    rp, col, val = ref.tiled_rounded()
    nrow0, nnz0 = len(rp) - 1, len(val)
    assert (nrow0, int(rp[-1])) == (ref.TILED_ROWS, nnz0) and col.max() < ref.TILED_NCOL
    once = {n for lpr in ref.LANES for n in (0, 1, lpr + 1, 4 * lpr + 1)} | {300}
    assert once <= set(np.diff(rp).tolist()), "every row length of the 300-row matrix"
    f0, inexact0, under0, rel0 = ref.demote(val)
    assert under0 == 3 and inexact0 == nnz0 - 1 and 0.0 < rel0 < 2.0**-24
    for k in (1, 3, 7):
        trp, tcc, tcv = tiled.tile_csr(k, ref.TILED_NCOL, rp, col, val)
        f, inexact, under, rel = ref.demote(tcv)
        assert (inexact, under, rel) == (k * inexact0, k * under0, rel0)
        assert f.tobytes() == np.tile(f0, k).tobytes() and ref.widen(f).tobytes() == np.tile(ref.widen(f0), k).tobytes()
        assert tiled.tiled_mismatch((trp, tcc, ref.widen(f)), (rp, col, ref.widen(f0)), k, ref.TILED_NCOL) is None
        assert np.array_equal(ref.pack(tcc, f) >> np.uint64(32), np.tile(ref.pack(col, f0) >> np.uint64(32), k))
        # one value of the last copy with a larger change than any of the base
        worse = tcv.copy()
        worse[-1] = ref.WORST_VALUE
        g, inexact_w, under_w, rel_w = ref.demote(worse)
        assert rel_w == ref.WORST_REL > rel0 and (inexact_w, under_w) == (k * inexact0, k * under0) and g[-1] == np.float32(1.0)
    trip = tiled.max_grid() * tiled.block_lanes()
    k, cond = ref.tiled_copies(rp, trip)
    assert all(cond.values()) and not ((k - 1) * nrow0 > trip and (k - 1) * nnz0 > trip), (k, cond)
    print(f"{k} copies: {k * nrow0} rows, {k * nnz0} entries, one trip {trip}")
