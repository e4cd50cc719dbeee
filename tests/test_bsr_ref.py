"""The NumPy twin of the block CSR conversions and product (tests/bsr_ref.py) held to a dense product and to the round-trip
identity, for every block size, on shapes that are no multiple of it.  No GPU."""
import numpy as np
import pytest

import bsr_ref


def _random_csr(rng, nrow, ncol, per_row):
    """ascending columns, no duplicates, no zero values"""
    cols = [np.sort(rng.choice(ncol, size=min(per_row, ncol), replace=False)) for _ in range(nrow)]
    row_ptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    col = np.concatenate(cols).astype(np.int32) if nrow else np.zeros(0, np.int32)
    val = rng.uniform(0.5, 2.0, size=len(col)) * rng.choice([-1.0, 1.0], size=len(col))
    return row_ptr, col, val


def _dense_csr(nrow, ncol, row_ptr, col, val):
    A = np.zeros((nrow, ncol))
    np.add.at(A, (np.repeat(np.arange(nrow), np.diff(row_ptr)), col), val)
    return A


@pytest.mark.parametrize("bs", range(2, 9))
def test_the_twin_against_a_dense_product_and_the_round_trip(bs):
    rng = np.random.default_rng(100 + bs)
    nrow, ncol = 5 * bs - 1, 6 * bs - (bs - 1)  # no multiples of bs
    row_ptr, col, val = _random_csr(rng, nrow, ncol, 4)
    bp, bc, bv = bsr_ref.csr_to_bsr(nrow, ncol, row_ptr, col, val, bs)
    mb, nbc = bsr_ref.dims(nrow, ncol, bs)
    assert len(bp) == mb + 1 and bp[0] == 0 and bp[-1] == len(bc) and len(bv) == len(bc) * bs * bs and bc.max() < nbc
    for r in range(mb):  # block columns ascend inside a block row
        assert np.all(np.diff(bc[bp[r]:bp[r + 1]]) > 0)
    A = _dense_csr(nrow, ncol, row_ptr, col, val)
    assert np.array_equal(bsr_ref.dense(nrow, ncol, bs, bp, bc, bv), A)
    x, y0 = rng.standard_normal(ncol), rng.standard_normal(nrow)
    y = bsr_ref.product(nrow, ncol, bs, bp, bc, bv, x, y0)
    assert np.allclose(np.asarray(y, dtype=np.float64), y0 + A @ x, rtol=0, atol=1e-12 * (np.abs(A) @ np.abs(x) + np.abs(y0)).max())
    # the padding of edge blocks is absent: whatever stands there reaches neither the product nor the CSR form
    keep = bsr_ref.positions(nrow, ncol, bs, bp, bc, bv)[3]
    poisoned = np.full(len(bv), np.nan)
    poisoned[keep] = bv[keep]
    assert len(keep) < len(bv)
    assert np.array_equal(np.asarray(bsr_ref.product(nrow, ncol, bs, bp, bc, poisoned, x, y0)), np.asarray(y))
    for got, want in zip(bsr_ref.bsr_to_csr(nrow, ncol, bs, bp, bc, poisoned, True), (row_ptr, col, val)):
        assert np.array_equal(got, want)  # bsr_to_csr(csr_to_bsr(A), drop_zeros) is A, array for array
    rp0, c0, v0 = bsr_ref.bsr_to_csr(nrow, ncol, bs, bp, bc, bv, False)
    assert len(v0) == len(keep) and np.count_nonzero(v0) == len(val)
    # the transposed arrays are those of A^T
    tp, tc, tv = bsr_ref.transpose(nrow, ncol, bs, bp, bc, bv)
    assert np.array_equal(bsr_ref.dense(ncol, nrow, bs, tp, tc, tv), A.T)


def test_duplicates_are_added_in_stored_order_from_zero():
    # three entries on one position: ((0.0 + a) + b) + c in stored order, which no other order gives here
    a, b, c = 1.0, 2.0**-53, 2.0**-53
    row_ptr, col, val = np.array([0, 3, 4], np.int32), np.array([1, 1, 1, 0], np.int32), np.array([a, b, c, -0.0])
    bp, bc, bv = bsr_ref.csr_to_bsr(2, 2, row_ptr, col, val, 2)
    assert np.array_equal(bp, [0, 1]) and np.array_equal(bc, [0])
    assert bv[1] == ((0.0 + a) + b) + c == 1.0 and (b + c) + a != 1.0
    assert bv[2] == 0.0 and not np.signbit(bv[2])  # 0.0 + -0.0
    assert bv[0] == 0.0 and bv[3] == 0.0


def test_empty_shapes():
    bp, bc, bv = bsr_ref.csr_to_bsr(0, 7, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0), 3)
    assert np.array_equal(bp, [0]) and len(bc) == 0 and len(bv) == 0
    bp, bc, bv = bsr_ref.csr_to_bsr(5, 7, np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0), 3)
    assert np.array_equal(bp, [0, 0, 0]) and len(bc) == 0
    rp, c, v = bsr_ref.bsr_to_csr(5, 7, 3, bp, bc, bv)
    assert np.array_equal(rp, np.zeros(6)) and len(c) == 0 and len(v) == 0
    assert np.array_equal(bsr_ref.product(5, 7, 3, bp, bc, bv, np.ones(7), np.arange(5.0)), np.arange(5.0))


def test_unsorted_block_columns_come_out_ascending():
    bs, nrow, ncol = 2, 4, 6
    bp, bc = np.array([0, 3, 4], np.int32), np.array([2, 0, 1, 1], np.int32)
    bv = np.arange(1.0, 17.0)
    rp, c, v = bsr_ref.bsr_to_csr(nrow, ncol, bs, bp, bc, bv)
    for r in range(nrow):
        assert np.all(np.diff(c[rp[r]:rp[r + 1]]) > 0)
    assert np.array_equal(_dense_csr(nrow, ncol, rp, c, v), bsr_ref.dense(nrow, ncol, bs, bp, bc, bv))


@pytest.mark.parametrize("bs", (2, 3, 8))
def test_the_conversions_commute_with_block_diagonal_copies(bs):
    """the oracle of tests/tiled.py for csrc/convert_bsr.hip: csr_to_bsr, bsr_to_csr (both drop_zeros) and transpose of k copies are
    the base's result tiled, as bytes; and the coverage conditions of the GPU cases (tests/test_gpu_bsr.py) hold for their k"""
    import tiled

    base = bsr_ref.tiled_base(bs)
    nrow0, ncol0, rp, cc, cv = base
    assert (nrow0, ncol0) == (8 * bs, 9 * bs)
    rows = np.repeat(np.arange(nrow0), np.diff(rp))
    assert rp[2] == rp[1] and not np.any(rows // bs == 5), "an empty row and an empty block row"
    assert any(np.any(np.diff(cc[rp[r]:rp[r + 1]]) < 0) for r in range(nrow0)), "unsorted columns"
    assert all(np.count_nonzero(cc[rp[r]:rp[r + 1]] == cc[rp[r]]) == 3 for r in range(nrow0) if rp[r + 1] > rp[r]), "duplicates"
    bp0, bc0, bv0 = bsr_ref.csr_to_bsr(nrow0, ncol0, rp, cc, cv, bs)
    assert np.any(bv0 == 0.0) and np.any(np.diff(bp0) == 0)
    for k in (1, 2, 5):
        trp, tcc, tcv = tiled.tile_csr(k, ncol0, rp, cc, cv)
        got = bsr_ref.csr_to_bsr(k * nrow0, k * ncol0, trp, tcc, tcv, bs)
        want = tiled.tile_bsr(k, 9, bp0, bc0, bv0, bs)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), f"bs {bs} k {k}: csr_to_bsr"
        # from blocks in random order inside the block rows, as an uploaded handle may hold them
        sc0, sv0 = bsr_ref.shuffle_blocks(np.random.default_rng(k), bp0, bc0, bv0, bs)
        assert np.any(np.diff(sc0)[np.diff(np.repeat(np.arange(8), np.diff(bp0))) == 0] < 0)
        sp, sc, sv = tiled.tile_bsr(k, 9, bp0, sc0, sv0, bs)
        for drop in (True, False):
            base_csr = bsr_ref.bsr_to_csr(nrow0, ncol0, bs, bp0, bc0, bv0, drop)
            assert tiled.tiled_mismatch(bsr_ref.bsr_to_csr(k * nrow0, k * ncol0, bs, *want, drop), base_csr, k, ncol0) is None
            assert tiled.tiled_mismatch(bsr_ref.bsr_to_csr(k * nrow0, k * ncol0, bs, sp, sc, sv, drop), base_csr, k, ncol0) is None
        tp0, tc0, tv0 = bsr_ref.transpose(nrow0, ncol0, bs, bp0, sc0, sv0)
        for g, w in zip(bsr_ref.transpose(k * nrow0, k * ncol0, bs, sp, sc, sv), tiled.tile_bsr(k, 8, tp0, tc0, tv0, bs)):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), f"bs {bs} k {k}: transpose"
    # what tile_bsr is: the copy's offset on the block columns, the pointer continued, the same bytes
    p2, c2, v2 = tiled.tile_bsr(2, 9, bp0, bc0, bv0, bs)
    assert np.array_equal(p2, np.concatenate([bp0, bp0[1:] + bp0[-1]])) and np.array_equal(c2, np.concatenate([bc0, bc0 + 9]))
    assert v2.tobytes() == bv0.tobytes() * 2
    trip = tiled.max_grid() * tiled.block_lanes()
    k, cond = bsr_ref.tiled_copies(bs, base, trip)
    assert all(cond.values()), cond
    per = {2: nrow0, 3: int(rp[-1]), 8: int(rp[-1])}[bs]  # what binds k here; one copy fewer misses its condition: k is the least
    assert not ((k - 1) * per + (1 if bs == 2 else 0) > trip), (k, per)
    print(f"bs {bs}: {k} copies, nnz {k * int(rp[-1])}, nnzb {k * len(bc0)}, rows {k * nrow0}, one trip {trip}")
