"""The NumPy twin of spmv_spgemm and spmv_csr_transpose (csrc/spgemm.hip; include/spmv_abi.h states the definition), and the
inputs that tests/test_spgemm_ref.py and tests/test_gpu_spgemm.py share.

C = A B, A m x k and B k x n as CSR triples (row_ptr, col, val) that may hold unsorted columns, duplicates and stored zeros.
Pattern: one entry (i, j) for every pair that a stored a_ip and a stored b_pj reach - structural - columns ascending.  Value: the
scalar products of row i in the order (position of the A entry in the row, position of the B entry in its row), each t = a * b
rounded once, added from 0.0 left to right in plain additions."""
from fractions import Fraction

import numpy as np

MUTANTS = ("reversed", "fma", "merged_b", "dropped_last", "cancelled_removed")


def _expand(m, A, B):
    """every scalar product in (i, p, q) order: (row, column, a, b, ub)"""
    arp, acc, acv = (np.asarray(x) for x in A)
    brp, bcc, bcv = (np.asarray(x) for x in B)
    arp, brp = arp.astype(np.int64), brp.astype(np.int64)
    arow = np.repeat(np.arange(m, dtype=np.int64), np.diff(arp))
    blen = np.diff(brp)[acc] if len(acc) else np.zeros(0, dtype=np.int64)
    ub = np.zeros(m, dtype=np.int64)
    np.add.at(ub, arow, blen)
    total = int(blen.sum())
    src = np.repeat(np.arange(len(acc), dtype=np.int64), blen)  # the A entry of every product
    start = np.cumsum(blen) - blen
    q = np.arange(total, dtype=np.int64) - np.repeat(start, blen)
    at = brp[acc.astype(np.int64)][src] + q if total else np.zeros(0, dtype=np.int64)
    return arow[src], bcc[at].astype(np.int64), np.asarray(acv, dtype=np.float64)[src], np.asarray(bcv, dtype=np.float64)[at], ub


def _merge_duplicates(nrow, M):
    """the mutation's B: duplicates of a row summed into their first occurrence (stored order otherwise)"""
    rp, cc, cv = (np.asarray(x) for x in M)
    out_rp, out_c, out_v = [0], [], []
    for i in range(nrow):
        seen = {}
        for e in range(rp[i], rp[i + 1]):
            c = int(cc[e])
            if c in seen:
                out_v[seen[c]] += float(cv[e])
            else:
                seen[c] = len(out_c)
                out_c.append(c)
                out_v.append(float(cv[e]))
        out_rp.append(len(out_c))
    return np.array(out_rp, dtype=np.int32), np.array(out_c, dtype=np.int32), np.array(out_v, dtype=np.float64)


def spgemm_twin(m, k, n, A, B, mutate=None):
    """(row_ptr, col, val, ub): ub[i] the scalar products of row i.  `mutate`: one of MUTANTS - a wrong product for the tests"""
    assert mutate is None or mutate in MUTANTS
    if mutate == "merged_b":
        B = _merge_duplicates(k, B)
    ri, cj, a, b, ub = _expand(m, A, B)
    if mutate == "dropped_last" and len(ri):
        keep = np.ones(len(ri), dtype=bool)
        keep[np.cumsum(ub[ub > 0]) - 1] = False  # the last product of every non-empty row
        ri, cj, a, b = ri[keep], cj[keep], a[keep], b[keep]
    t = a * b
    order = np.lexsort((cj, ri))  # stable: (p, q) order inside equal (i, j)
    ri, cj, t, a, b = ri[order], cj[order], t[order], a[order], b[order]
    head = np.ones(len(ri), dtype=bool)
    head[1:] = (ri[1:] != ri[:-1]) | (cj[1:] != cj[:-1])
    start = np.flatnonzero(head)
    length = np.diff(np.append(start, len(ri)))
    val = np.zeros(len(start))
    if mutate == "fma":  # acc = fma(a, b, acc): one rounding per product, through exact rationals
        for s, (at, ln) in enumerate(zip(start, length)):
            acc = 0.0
            for e in range(at, at + ln):
                acc = float(Fraction(float(a[e])) * Fraction(float(b[e])) + Fraction(acc))
            val[s] = acc
    else:
        for pos in range(int(length.max(initial=0))):  # position by position: 0.0 + t_1 + t_2 + ... in every run at once
            live = length > pos
            at = start[live] + (length[live] - 1 - pos if mutate == "reversed" else pos)
            val[live] = val[live] + t[at]
    rows_c, cols_c = ri[head], cj[head]
    if mutate == "cancelled_removed":
        keep = val != 0.0
        rows_c, cols_c, val = rows_c[keep], cols_c[keep], val[keep]
    rp = np.zeros(m + 1, dtype=np.int64)
    np.add.at(rp, rows_c + 1, 1)
    return np.cumsum(rp).astype(np.int32), cols_c.astype(np.int32), val, ub


def transpose_twin(m, n, A):
    """(row_ptr, col, val) of A^T (n x m): row j holds column j of A in ascending i, equal (j, i) in A's stored order"""
    rp, cc, cv = (np.asarray(x) for x in A)
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(rp.astype(np.int64)))
    order = np.argsort(cc, kind="stable")  # entry ids ascend inside a column: ascending i, then stored order
    out = np.zeros(n + 1, dtype=np.int64)
    np.add.at(out, cc.astype(np.int64) + 1, 1)
    return np.cumsum(out).astype(np.int32), rows[order].astype(np.int32), np.asarray(cv, dtype=np.float64)[order]


def sorted_columns(m, A):
    """A with every row's entries ordered stably by column (duplicates kept)"""
    rp, cc, cv = (np.asarray(x) for x in A)
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(rp.astype(np.int64)))
    order = np.lexsort((cc, rows))
    return rp.astype(np.int32), cc[order].astype(np.int32), np.asarray(cv, dtype=np.float64)[order]


def triple_loop(m, k, n, A, B):
    """the definition as scalar loops: {(i, j): value} with Python floats"""
    arp, acc, acv = A
    brp, bcc, bcv = B
    out = [dict() for _ in range(m)]
    for i in range(m):
        for e in range(arp[i], arp[i + 1]):
            p = int(acc[e])
            for f in range(brp[p], brp[p + 1]):
                t = float(acv[e]) * float(bcv[f])
                out[i][int(bcc[f])] = out[i].get(int(bcc[f]), 0.0) + t
    return out


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def csr_of(nrow, row, col, val):
    """entries grouped by row, their order inside a row kept"""
    row, col, val = np.asarray(row, dtype=np.int64), np.asarray(col), np.asarray(val, dtype=np.float64)
    order = np.argsort(row, kind="stable")
    rp = np.zeros(nrow + 1, dtype=np.int64)
    np.add.at(rp, row + 1, 1)
    return np.cumsum(rp).astype(np.int32), col[order].astype(np.int32), val[order]


def identity(n):
    return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n)


def laplacian_2d(mgrid):
    import solver_ref

    n, r, c, v = solver_ref.laplacian_2d(mgrid)
    return n, csr_of(n, r, c, v)


def tridiagonal(n):
    i = np.arange(n, dtype=np.int64)
    row = np.concatenate([i, i[1:], i[:-1]])
    col = np.concatenate([i, i[:-1], i[1:]])
    val = np.concatenate([np.full(n, 2.0), np.full(n - 1, -1.0), np.full(n - 1, -1.0)])
    order = np.lexsort((col, row))
    return csr_of(n, row[order], col[order], val[order])


def arrow(n):
    """row and column 0 full, a diagonal; small integer values"""
    i = np.arange(1, n, dtype=np.int64)
    row = np.concatenate([np.zeros(n, dtype=np.int64), i, i])
    col = np.concatenate([np.arange(n, dtype=np.int64), np.zeros(n - 1, dtype=np.int64), i])
    val = np.concatenate([np.arange(n) % 5 + 1.0, i % 3 + 1.0, i % 7 + 2.0])
    order = np.lexsort((col, row))
    return csr_of(n, row[order], col[order], val[order])


def random_rows(nrow, ncol, per_row, seed, values="uniform", bits=6, e=4):
    """per_row entries a row at random columns (duplicates happen), unsorted.  values: "uniform" in (-1, 1) or "dyadic" (exact.py)"""
    import exact

    rng = np.random.default_rng(seed)
    row = np.repeat(np.arange(nrow, dtype=np.int64), per_row)
    col = rng.integers(0, ncol, nrow * per_row)
    val = rng.uniform(-1, 1, nrow * per_row) if values == "uniform" else exact.dyadic(rng, nrow * per_row, bits, e)
    return csr_of(nrow, row, col, val)


def random_unique_rows(nrow, ncol, per_row, seed):
    """per_row distinct columns a row, unsorted, values uniform in (-1, 1)"""
    rng = np.random.default_rng(seed)
    row = np.repeat(np.arange(nrow, dtype=np.int64), per_row)
    col = np.concatenate([rng.permutation(ncol)[:per_row] for _ in range(nrow)])
    return csr_of(nrow, row, col, rng.uniform(-1, 1, nrow * per_row))


def order_sensitive_pair():
    """40 x 30 by 30 x 35, 12 random entries a row: duplicates, unsorted columns, runs of three and more addends"""
    return 40, 30, 35, random_rows(40, 30, 12, 101), random_rows(30, 35, 12, 102)


def cancelling_pair():
    """stored zeros, and an entry whose two products cancel exactly: c_00 = 1 * 3 + (-1) * 3 = 0 stays in the pattern"""
    A = csr_of(3, [0, 0, 0, 1, 2, 2], [0, 1, 2, 1, 2, 0], [1.0, -1.0, 0.5, 0.0, 2.0, 0.25])
    B = csr_of(3, [0, 1, 1, 2, 2], [0, 0, 2, 1, 2], [3.0, 3.0, 0.0, 0.75, 0.1])
    return 3, 3, 3, A, B


def one_row_case(c, one_column):
    """a one-row A of c entries against a B of one entry a row: exactly c scalar products, in c runs or (one_column) in one"""
    rng = np.random.default_rng(7000 + c + (1 if one_column else 0))
    A = (np.array([0, c], dtype=np.int32), rng.permutation(c).astype(np.int32), rng.uniform(-1, 1, c))
    bcol = np.zeros(c, dtype=np.int32) if one_column else rng.permutation(c).astype(np.int32)
    B = (np.arange(c + 1, dtype=np.int32), bcol, rng.uniform(-1, 1, c))
    return 1, c, (1 if one_column else c), A, B


def hub_case(hub_len=5000, hub_rows=200, short_rows=300, n=6000, seed=31):
    """hub_rows rows of A that all reach row 0 of B, which holds hub_len entries, mixed with short rows: (m, k, n, A, B)"""
    rng = np.random.default_rng(seed)
    m, k = hub_rows + short_rows, 64
    is_hub = np.zeros(m, dtype=bool)
    is_hub[rng.permutation(m)[:hub_rows]] = True
    row, col = [], []
    for i in range(m):
        cols = rng.integers(1, k, 3)
        if is_hub[i]:
            cols = np.concatenate([cols[:1], [0], cols[1:]])
        elif i % 7 == 0:
            cols = cols[:0]  # an empty row among them
        row.append(np.full(len(cols), i))
        col.append(cols)
    row, col = np.concatenate(row), np.concatenate(col)
    A = csr_of(m, row, col, rng.uniform(-1, 1, len(row)))
    brow = np.concatenate([np.zeros(hub_len, dtype=np.int64), np.repeat(np.arange(1, k, dtype=np.int64), 4)])
    bcol = np.concatenate([rng.permutation(n)[:hub_len], rng.integers(0, n, 4 * (k - 1))])
    B = csr_of(k, brow, bcol, rng.uniform(-1, 1, len(brow)))
    return m, k, n, A, B


# ---- rows that take a later trip over the grid (tests/tiled.py) ---------------------------------------------------------------------
# the scalar products of the rows of class_edge_pair: both edges of the wavefront class (129 .. 512) and of the workgroup class
# (513 .. 2048), either side of a power of two in each - the sorting network exactly full and one over - a 16-lane row, an empty one
CLASS_EDGE_UB = (129, 513, 40, 200, 700, 0, 256, 1024, 257, 1025, 512, 2048)


def class_edge_pair(ubs=CLASS_EDGE_UB, ncol=400, seed=61):
    """(m, k, n, A, B): row i of A has exactly ubs[i] scalar products.  B has 40 rows of lengths 1 .. 40 with random columns
    (unsorted, repeats) and values in (-1, 1); a row of A names random rows of B, repeats among them, until their lengths add up:
    runs of several addends whose order matters"""
    rng = np.random.default_rng(seed)
    brow = np.repeat(np.arange(40, dtype=np.int64), np.arange(1, 41))
    B = csr_of(40, brow, rng.integers(0, ncol, len(brow)), rng.uniform(-1, 1, len(brow)))
    row, col = [], []
    for i, ub in enumerate(ubs):
        left = int(ub)
        while left > 0:
            length = int(rng.integers(1, min(40, left) + 1))
            row.append(i)
            col.append(length - 1)  # (row p of B holds p + 1 entries)
            left -= length
    A = csr_of(len(ubs), row, col, rng.uniform(-1, 1, len(row)))
    return len(ubs), 40, ncol, A, B


def grid_loop_case():
    """class_edge_pair in as many block-diagonal copies as take the wavefront class and the workgroup class of spgemm_rows_kernel
    past kMaxGrid workgroups: a dict of the base pair, its twin, the copies k, per looping class (name, rows a copy, rows a
    workgroup), and where(copy, row) for tiled.tiled_mismatch.  Every threshold comes from the settings headers."""
    import tiled

    grid = tiled.max_grid()
    classes = tiled.spgemm_classes()  # ascending: 16 lanes, the wavefront, the workgroup
    caps = [cap for _, cap, _ in classes]
    m, k0, n, A, B = class_edge_pair()
    twin = spgemm_twin(m, k0, n, A, B)
    ub = twin[3]
    cls = np.where(ub > 0, np.searchsorted(caps, ub, side="left") + 1, 0)  # spgemm_class_of: 0 none, 1 .. 3 the LDS classes
    names = {0: "none", 1: "lane16", 2: "wave", 3: "block", 4: "sort"}
    looping = {c: (names[c], int(np.sum(cls == c)), classes[c - 1][2]) for c in (2, 3)}
    # one copy beyond the smallest count that loops: the second trip of the wavefront class then holds two whole row groups
    copies = max(per_group * grid // rows for _, rows, per_group in looping.values()) + 2
    where = tiled.describe_trips(cls, {c + 1: per_group for c, (_, _, per_group) in enumerate(classes)}, grid, names)
    return dict(m=m, k=k0, n=n, A=A, B=B, twin=twin, cls=cls, caps=caps, grid=grid, copies=copies, looping=looping, where=where)
