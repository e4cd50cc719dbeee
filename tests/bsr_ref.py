"""NumPy twin of the block CSR set-up (csrc/convert_bsr.hip) and product (csrc/kernels_bsr.hip) - TEST INFRASTRUCTURE ONLY.

The same definitions as the device code:
  * a BSR matrix is (nrow, ncol, bs, brow_ptr[mb + 1], bcol[nnzb], val[nnzb * bs * bs]) with mb = ceil(nrow / bs) block rows and
    nbc = ceil(ncol / bs) block columns, blocks one after the other, row-major inside a block;
  * positions of a stored block outside nrow x ncol are ABSENT: no product, no entry of the CSR form;
  * csr_to_bsr: the blocks that hold an entry, block columns ascending inside a block row, every stored position the sum of the
    CSR entries that fall on it, added in stored order from 0.0 (a position without an entry is 0.0);
  * bsr_to_csr: the stored positions inside nrow x ncol, the blocks of a block row in stable order by block column, with
    drop_zeros without the values equal to 0.0;
  * transpose: blocks in stable order by block column, each transposed.
"""
from __future__ import annotations

import numpy as np


def dims(nrow: int, ncol: int, bs: int) -> tuple[int, int]:
    return -(-nrow // bs), -(-ncol // bs)


def csr_to_bsr(nrow, ncol, row_ptr, col, val, bs):
    rp = np.asarray(row_ptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    val = np.asarray(val, dtype=np.float64)
    mb, nbc = dims(nrow, ncol, bs)
    row = np.repeat(np.arange(nrow, dtype=np.int64), np.diff(rp))
    key = (row // bs) * max(nbc, 1) + col // bs
    order = np.argsort(key, kind="stable")  # stored order inside a block
    blocks, inverse = np.unique(key, return_inverse=True)
    bval = np.zeros((len(blocks), bs, bs))
    np.add.at(bval, (inverse[order], (row % bs)[order], (col % bs)[order]), val[order])  # unbuffered: one addition after the other
    brow_ptr = np.zeros(mb + 1, dtype=np.int64)
    np.add.at(brow_ptr, blocks // max(nbc, 1) + 1, 1)
    return np.cumsum(brow_ptr).astype(np.int32), (blocks % max(nbc, 1)).astype(np.int32), bval.reshape(-1)


def positions(nrow, ncol, bs, brow_ptr, bcol, val, sort_blocks=False):
    """(row, column, value, offset into val) of every stored position inside nrow x ncol, block after block, row-major inside a
    block; sort_blocks: the blocks of a block row in stable order by block column first"""
    bp = np.asarray(brow_ptr, dtype=np.int64)
    bcol = np.asarray(bcol, dtype=np.int64)
    nnzb = len(bcol)
    brow = np.repeat(np.arange(len(bp) - 1, dtype=np.int64), np.diff(bp))
    ids = np.arange(nnzb, dtype=np.int64)
    if sort_blocks and nnzb:
        ids = ids[np.argsort(bcol, kind="stable")]
        ids = ids[np.argsort(brow[ids], kind="stable")]
    r = np.tile(np.repeat(np.arange(bs, dtype=np.int64), bs), nnzb)
    c = np.tile(np.arange(bs, dtype=np.int64), nnzb * bs)
    b = np.repeat(ids, bs * bs)
    i, j, at = brow[b] * bs + r, bcol[b] * bs + c, b * bs * bs + r * bs + c
    keep = (i < nrow) & (j < ncol)
    return i[keep], j[keep], np.asarray(val, dtype=np.float64)[at[keep]], at[keep]


def bsr_to_csr(nrow, ncol, bs, brow_ptr, bcol, val, drop_zeros=True):
    i, j, v, _ = positions(nrow, ncol, bs, brow_ptr, bcol, val, sort_blocks=True)
    if drop_zeros:
        keep = ~(v == 0.0)
        i, j, v = i[keep], j[keep], v[keep]
    order = np.argsort(i, kind="stable")  # row after row; inside a row the blocks' order, columns of a block ascending
    row_ptr = np.zeros(nrow + 1, dtype=np.int64)
    np.add.at(row_ptr, i + 1, 1)
    return np.cumsum(row_ptr).astype(np.int32), j[order].astype(np.int32), v[order]


def transpose(nrow, ncol, bs, brow_ptr, bcol, val):
    """the BSR arrays of A^T (ncol x nrow)"""
    bp = np.asarray(brow_ptr, dtype=np.int64)
    bcol = np.asarray(bcol, dtype=np.int64)
    mb, nbc = dims(nrow, ncol, bs)
    brow = np.repeat(np.arange(mb, dtype=np.int64), np.diff(bp))
    order = np.argsort(bcol, kind="stable")
    tp = np.zeros(nbc + 1, dtype=np.int64)
    np.add.at(tp, bcol + 1, 1)
    blocks = np.asarray(val, dtype=np.float64).reshape(-1, bs, bs)[order].transpose(0, 2, 1)
    return np.cumsum(tp).astype(np.int32), brow[order].astype(np.int32), np.ascontiguousarray(blocks).reshape(-1)


def product(nrow, ncol, bs, brow_ptr, bcol, val, x, y0=None, dtype=np.longdouble):
    """y0 + A x over the stored positions inside nrow x ncol, in `dtype`"""
    i, j, v, _ = positions(nrow, ncol, bs, brow_ptr, bcol, val)
    y = np.zeros(nrow, dtype=dtype) if y0 is None else np.array(y0, dtype=dtype)
    np.add.at(y, i, v.astype(dtype) * np.asarray(x)[j].astype(dtype))
    return y


def abs_product(nrow, ncol, bs, brow_ptr, bcol, val, x):
    """(|A| |x|)_i and the number of stored positions of every row"""
    i, j, v, _ = positions(nrow, ncol, bs, brow_ptr, bcol, val)
    s = np.zeros(nrow)
    np.add.at(s, i, np.abs(v) * np.abs(np.asarray(x, dtype=np.float64)[j]))
    return s, np.bincount(i, minlength=nrow)[:nrow] if nrow else np.zeros(0, dtype=np.int64)


# ---- block-diagonal copies past one trip of the set-up kernels' grid (tests/tiled.py) ------------------------------------------------
def tiled_base(bs, bits=3, e=2):
    """(nrow0, ncol0, row_ptr, col, val) of a CSR base of 8 x 9 blocks of bs: dyadic values (tests/exact.py: sums of duplicates are
    exact), columns unsorted, every row's first entry stored twice more (three values on one position), row 1 empty, block row 5
    empty; the rows of a block row draw their columns from four of the nine block columns"""
    import exact

    rng = np.random.default_rng(2500 + bs)
    nrow0, ncol0 = 8 * bs, 9 * bs
    cols = []
    for br in range(8):
        pool = (rng.permutation(9)[:4, None] * bs + np.arange(bs)[None, :]).ravel()
        for r in range(bs):
            i = br * bs + r
            if i == 1 or br == 5:
                cols.append(np.zeros(0, np.int64))
                continue
            c = rng.permutation(pool)[:3 + (i % 3)]
            cols.append(np.concatenate([c, c[:1], c[:1]]))
    row_ptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    col = np.concatenate(cols).astype(np.int32)
    return nrow0, ncol0, row_ptr, col, exact.dyadic(rng, len(col), bits, e)


def tiled_copies(bs, base, trip):
    """(k, conditions): the least number of copies of `base` with which every grid-stride kernel of csrc/convert_bsr.hip takes a
    later trip (one trip: `trip` items), and the conditions as {text: holds}.  The kernels run over the entries (owner_of_entry,
    block_keys and the runs' pipeline: nnz), the blocks (block_fill, block_order_check, gather_i32, histogram, the sorts: nnzb), the
    stored values (block_transpose: nnzb * bs^2) and the scalar rows and one (bsr_rows: nrow + 1)."""
    nrow0, ncol0, rp, cc, cv = base
    nnz0 = int(rp[-1])
    nnzb0 = len(csr_to_bsr(nrow0, ncol0, rp, cc, cv, bs)[1])
    more = lambda per: trip // per + 1  # the least k with k * per > trip
    if bs == 2:
        k = max(more(nnz0), more(nnzb0), -(-trip // nrow0))
        cond = {"nnz > one trip": k * nnz0 > trip, "nnzb > one trip": k * nnzb0 > trip, "nrow + 1 > one trip": k * nrow0 + 1 > trip,
                "blocks per copy no divisor of 256": 256 % nnzb0 != 0}
    else:
        k = max(more(nnz0), more(nnzb0 * bs * bs))
        cond = {"nnz > one trip": k * nnz0 > trip, f"nnzb * {bs * bs} > one trip": k * nnzb0 * bs * bs > trip,
                "below 100 MB of values": k * nnzb0 * bs * bs * 8 < 100e6}
    return k, cond


def shuffle_blocks(rng, brow_ptr, bcol, val, bs):
    """the same BSR matrix with the blocks of every block row in random order"""
    bp = np.asarray(brow_ptr, dtype=np.int64)
    ids = np.concatenate([bp[r] + rng.permutation(int(bp[r + 1] - bp[r])) for r in range(len(bp) - 1)]).astype(np.int64)
    return np.asarray(bcol)[ids], np.asarray(val, dtype=np.float64).reshape(-1, bs * bs)[ids].reshape(-1)


def dense(nrow, ncol, bs, brow_ptr, bcol, val):
    i, j, v, _ = positions(nrow, ncol, bs, brow_ptr, bcol, val)
    A = np.zeros((nrow, ncol))
    np.add.at(A, (i, j), v)
    return A
