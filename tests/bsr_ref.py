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


def dense(nrow, ncol, bs, brow_ptr, bcol, val):
    i, j, v, _ = positions(nrow, ncol, bs, brow_ptr, bcol, val)
    A = np.zeros((nrow, ncol))
    np.add.at(A, (i, j), v)
    return A
