"""Block CSR on the GPU: the product and its transposed form bit for bit on dyadic inputs (tests/exact.py) for every block size and
every number of lanes per block row, the conversions against the NumPy twin (tests/bsr_ref.py) array for array, the rounding gate
for ordinary values, the plumbing (validate, download, plans, memory) and the solvers on a BSR handle.  The exact cases stand at every
block-row length where the kernel's loop changes shape, at every remainder of nrow and ncol, over more than two workgroups, through
spmv_apply_dot and spmv_apply_host as well; the set-up runs past one trip of its grid on block-diagonal copies (tests/tiled.py); a
closing test asserts that every instance of the kernel ran.

The rounding gate is derived, not measured: a row of t stored positions is a sum of t + 1 terms (y0 and t products); any order of
them, with or without fma, stays within (t + 1) * 2^-52 * (|A||x| + |y0|)_i of the exact sum to first order, and the reference
is the twin's product in np.longdouble.
"""
import collections

import numpy as np
import pytest

import bsr_ref
import exact
import tiled
from conftest import perf_expect

pytestmark = pytest.mark.gpu
AUTO, VECTOR, PANEL = 0, 1, 4
GUARD = 12345.0
INSTANCES = set()  # (bs, G, EDGE) of the bsr_vector_kernel instances that an exact test launched
RUNS = collections.Counter()


def _lanes(bs):
    """every number of lanes a block row may get (csrc/bsr_settings.hpp): bs^2 times a divisor of 64 // bs^2"""
    slots = 64 // (bs * bs)
    return [g * bs * bs for g in range(1, slots + 1) if slots % g == 0]


def _guarded(ctx, host):
    """(a Vector over the first len(host) entries of device memory that holds one guard element more, a reader of all of it).  Here
    the memory is an engine vector; tests/child_bsr_torch.py passes a torch tensor instead (torch has to initialise its HIP runtime
    before the engine's library is loaded, so that runs in a process of its own)"""
    big = ctx.vector_from(np.concatenate([host, [GUARD]]))
    v = ctx.wrap_vector(big.device_ptr, len(host))
    v._keep = big
    return v, big.download


def _structure(rng, mb, nbc, counts):
    """block row pointer and block columns: counts[i] distinct block columns per block row, in random order; every second
    non-empty block row holds the last block column"""
    cols = []
    for i, n in enumerate(counts):
        c = rng.permutation(nbc)[:n]
        if n and i % 2 == 0 and nbc - 1 not in c:
            c[rng.integers(n)] = nbc - 1
        cols.append(c)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), np.concatenate(cols).astype(np.int32) if mb else np.zeros(0, np.int32)


def _exact_matrices(bs):
    """(name, mb, nbc, counts): one block row of 0, 1, S, S + 1 and 1000 blocks each, and 37 block rows that hold all of them (the
    1000 behind others, so that its values cross offset 2^16 at bs = 8; the last workgroup is part-filled)"""
    S = tiled.bsr_slots(bs)
    out = [(f"mb1-{n}", 1, 1003, [n]) for n in (0, 1, S, S + 1, 1000)]
    pattern = [1, S, 0, S + 1, 1]
    counts = [pattern[i % 5] for i in range(37)]
    counts[20] = 1000
    out.append(("mb37", 37, 1003, counts))
    return out


def _loop_lengths(bs):
    """the block-row lengths at which the loop of bsr_vector_kernel<bs, G, .> changes shape (four steps of G blocks in flight, then
    single steps), for every G that bs takes: none, one, one short of / exactly / one more than a step, the same around the four
    steps in flight, a fifth step, and a long row whose steps are no multiple of four at any G but 1, 2, 5 (at those, 4 G + 1 is)"""
    groups = [lanes // (bs * bs) for lanes in _lanes(bs)]
    return sorted({n for G in groups for n in (0, 1, G - 1, G, G + 1, 4 * G - 1, 4 * G, 4 * G + 1, 5 * G, 1000)})


MIXED_ROWS = 131


def _mixed_counts(bs):
    """131 block rows that hold every length of _loop_lengths, the 1000 once and behind others; every round through the lengths
    starts one further, so that a length stands on even and on odd block rows (_structure: with and without the last block column)"""
    short = [n for n in _loop_lengths(bs) if n != 1000]
    counts = [short[(i + i // len(short)) % len(short)] for i in range(MIXED_ROWS)]
    counts[70] = 1000
    return counts


def _edge_matrices(bs):
    """(name, mb, nbc, counts, nrow % bs, ncol % bs): every length of _loop_lengths as a matrix of one block row, and the 131 mixed
    block rows once for every column remainder 0 .. bs - 1 (remainder 0: the kernel without the column edge), the row remainder one
    less (so 0 .. bs - 1 occur as well, and the instance without the column edge meets absent rows).  131 block rows are more than
    two workgroups at every number of lanes: a third, part-filled one runs"""
    out = [(f"row-{n}", 1, 1003, [n], (t + 1) % bs, t % bs) for t, n in enumerate(_loop_lengths(bs))]
    for crem in range(bs):
        out.append((f"mixed-c{crem}", MIXED_ROWS, 1003, _mixed_counts(bs), (crem - 1) % bs, crem))
    return out


def _shape(bs, matrix):
    """(name, mb, nbc, counts, nrow, ncol); a matrix without remainders has nrow % bs = bs - 1 and ncol % bs = 1"""
    name, mb, nbc, counts = matrix[:4]
    rrem, crem = matrix[4:] if len(matrix) > 4 else (bs - 1, 1)
    return name, mb, nbc, counts, bs * (mb - 1) + (rrem or bs), bs * (nbc - 1) + (crem or bs)


def _poisoned_handle(ctx, rng, bs, matrix, bits, e):
    """the BSR handle of a matrix with dyadic values and NaN at every stored position outside nrow x ncol, and its entry list"""
    name, mb, nbc, counts, nrow, ncol = _shape(bs, matrix)
    bp, bc = _structure(rng, mb, nbc, counts)
    val = exact.dyadic(rng, len(bc) * bs * bs, bits, e)
    i, j, v, at = bsr_ref.positions(nrow, ncol, bs, bp, bc, val)
    stored = np.full(len(val), np.nan)  # NaN at every position outside nrow x ncol
    stored[at] = val[at]
    outside = bool((ncol % bs and np.any(bc == nbc - 1)) or (nrow % bs and counts[-1] > 0))
    assert (len(at) < len(val)) == outside, name
    A = ctx.bsr(nrow, ncol, bs, bp, bc, stored)
    info = A.info
    assert (info.format, info.nrow, info.ncol, info.ell_k, info.nnz, info.kernel) == (5, nrow, ncol, bs, len(bc) * bs * bs, VECTOR)
    assert info.max_row_nnz == max(counts) * bs and info.lanes_per_row in _lanes(bs)
    return A, (i, j, v)


def _ran(A, bs):
    """the instance of bsr_vector_kernel that a product of A launches (bsr_apply: none where there is nothing to add)"""
    info = A.info
    if info.nrow and info.nnz:
        INSTANCES.add((bs, info.lanes_per_row // (bs * bs), info.ncol % bs != 0))


def check_exact(ctx, bs, matrices, guarded):
    """the forward product under every number of lanes per block row and the transposed product, bit for bit, y with a guard"""
    rng = np.random.default_rng(500 + bs)
    for matrix in matrices:
        name, mb, nbc, counts, nrow, ncol = _shape(bs, matrix)
        bits, e = exact.choose_bits(max(1000 * bs, mb * bs))
        A, (i, j, v) = _poisoned_handle(ctx, rng, bs, matrix, bits, e)
        info = A.info
        x = exact.poison(exact.dyadic(rng, ncol, bits, e), j)  # NaN / inf at every column no stored in-range position uses
        y0 = exact.dyadic(rng, nrow, bits, e)
        want = exact.exact_product(nrow, i, j, v, x, e, y0=y0)
        dx = ctx.vector_from(x)
        for lanes in _lanes(bs):
            A.set_kernel(VECTOR, lanes)
            assert A.info.lanes_per_row == lanes and A.info.kernel == VECTOR
            dy, read = guarded(ctx, y0)
            ctx.apply(A, dx, dy)
            ctx.sync()
            got = read()
            assert got[nrow] == GUARD, f"bs {bs} {name} lanes {lanes}: y written at nrow"
            assert np.array_equal(got[:nrow], want), f"bs {bs} {name} lanes {lanes}: forward"
            _ran(A, bs)
        A.set_kernel(AUTO, 0)
        assert A.info.lanes_per_row == info.lanes_per_row
        # transposed: x has nrow entries (poisoned where no stored position reads a row), y ncol and its guard
        xt = exact.poison(exact.dyadic(rng, nrow, bits, e), i)
        yt0 = exact.dyadic(rng, ncol, bits, e)
        want_t = exact.exact_product(ncol, j, i, v, xt, e, y0=yt0)
        dyt, read = guarded(ctx, yt0)
        ctx.apply_transpose(A, ctx.vector_from(xt), dyt)
        ctx.sync()
        got = read()
        assert got[ncol] == GUARD, f"bs {bs} {name}: transposed y written at ncol"
        assert np.array_equal(got[:ncol], want_t), f"bs {bs} {name}: transposed"
        assert A.get_param("transpose_ready") == 1 and A.get_param("transpose_kernel") == VECTOR


@pytest.mark.parametrize("bs", range(2, 9))
def test_product_and_transposed_product_are_exact_on_dyadic_inputs(ctx, bs):
    check_exact(ctx, bs, _exact_matrices(bs), _guarded)
    RUNS["exact"] += 1


@pytest.mark.parametrize("bs", range(2, 9))
def test_every_loop_edge_and_every_remainder_is_exact(ctx, bs):
    """every length at which the kernel's loop changes shape, alone and mixed over three workgroups, every nrow % bs and ncol % bs,
    under every number of lanes per block row"""
    matrices = _edge_matrices(bs)
    lengths = _loop_lengths(bs)
    for lanes in _lanes(bs):
        G = lanes // (bs * bs)
        assert {0, 1, G - 1, G, G + 1, 4 * G - 1, 4 * G, 4 * G + 1, 5 * G, 1000} <= set(lengths), (bs, G)
        assert MIXED_ROWS >= 2 * tiled.bsr_rows_per_workgroup(bs, lanes) + 1, (bs, lanes)
    assert {m[3][0] for m in matrices if m[1] == 1} == set(lengths) == set(_mixed_counts(bs))
    assert {m[5] for m in matrices} == set(range(bs)) == {m[4] for m in matrices}
    assert {m[5] for m in matrices if m[1] == MIXED_ROWS} == set(range(bs)) == {m[4] for m in matrices if m[1] == MIXED_ROWS}
    check_exact(ctx, bs, matrices, _guarded)
    RUNS["edges"] += 1


@pytest.mark.parametrize("bs", range(2, 9))
def test_the_other_entry_points_are_exact_on_the_mixed_matrix(ctx, bs):
    """spmv_apply_transpose, spmv_apply_dot (y = A x over NaN, y += A x, and the dot w . y held to integer arithmetic) and
    spmv_apply_host on the 131 mixed block rows, at the lanes AUTO picks and at the widest"""
    rng = np.random.default_rng(900 + bs)
    for crem in sorted({0, 1, bs - 1}):  # without the column edge, the remainder of the earlier tests, the widest remainder
        matrix = (f"mixed-c{crem}", MIXED_ROWS, 1003, _mixed_counts(bs), (crem - 1) % bs, crem)
        name, mb, nbc, counts, nrow, ncol = _shape(bs, matrix)
        bits, e = exact.choose_bits_dot(sum(counts) * bs * bs, max(nrow, ncol))
        A, (i, j, v) = _poisoned_handle(ctx, rng, bs, matrix, bits, e)
        x = exact.poison(exact.dyadic(rng, ncol, bits, e), j)
        y0, w = exact.dyadic(rng, nrow, bits, e), exact.dyadic(rng, nrow, bits, e)
        xt = exact.poison(exact.dyadic(rng, nrow, bits, e), i)
        yt0 = exact.dyadic(rng, ncol, bits, e)
        over, onto = exact.exact_product(nrow, i, j, v, x, e), exact.exact_product(nrow, i, j, v, x, e, y0=y0)
        want_t = exact.exact_product(ncol, j, i, v, xt, e, y0=yt0)
        dx, dw, dxt = ctx.vector_from(x), ctx.vector_from(w), ctx.vector_from(xt)
        auto = A.info.lanes_per_row
        for lanes in sorted({auto, _lanes(bs)[-1]}):
            A.set_kernel(VECTOR, lanes)
            what = f"bs {bs} {name} lanes {lanes}"
            dy, read = _guarded(ctx, np.full(nrow, np.nan))
            dot = ctx.apply_dot(A, dx, dy, dw, overwrite=True)
            got = read()
            assert got[nrow] == GUARD and np.array_equal(got[:nrow], over), f"{what}: overwrite"
            assert dot == exact.exact_dot(w, over, e, 2 * e), f"{what}: the dot of y = A x"
            dy, read = _guarded(ctx, y0)
            dot = ctx.apply_dot(A, dx, dy, dw, overwrite=False)
            got = read()
            assert got[nrow] == GUARD and np.array_equal(got[:nrow], onto), f"{what}: y += A x with the dot"
            assert dot == exact.exact_dot(w, onto, e, 2 * e), f"{what}: the dot of y += A x"
            _ran(A, bs)
            y, dy = y0.copy(), ctx.vector_from(y0)
            ctx.apply_host(A, x, y)
            ctx.apply(A, dx, dy)
            ctx.sync()
            assert np.array_equal(y.view(np.uint64), dy.download().view(np.uint64)), f"{what}: apply_host against apply on device vectors"
            assert np.array_equal(y, onto), f"{what}: apply_host"
            dyt, read = _guarded(ctx, yt0)
            ctx.apply_transpose(A, dxt, dyt)
            ctx.sync()
            got = read()
            assert got[ncol] == GUARD and np.array_equal(got[:ncol], want_t), f"{what}: transposed"
    RUNS["entry points"] += 1


def _torch_child(case):
    """tests/child_bsr_torch.py in a fresh process: torch initialises its HIP runtime before the engine's library is loaded"""
    import subprocess
    import sys
    from pathlib import Path

    child = Path(__file__).with_name("child_bsr_torch.py")
    r = subprocess.run([sys.executable, str(child), case], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"BSR_TORCH_OK {case}" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])


def test_exact_products_with_the_guard_in_a_longer_torch_tensor():
    """every block size, the 37 block rows, every number of lanes, forward and transposed: y is spmv_vec_wrap_device over the first
    nrow entries of a torch tensor of nrow + 1"""
    _torch_child("exact")


def test_validate_on_wrapped_device_arrays_changed_under_the_handle():
    _torch_child("validate")


def test_multiples_of_the_block_size_take_the_kernel_without_the_column_edge(ctx):
    # nrow and ncol multiples of bs: the instance of the kernel that knows nothing of edges; poison everywhere it must not read
    rng = np.random.default_rng(77)
    for bs in (2, 3, 4, 8):
        mb, nbc = 9, 40
        nrow, ncol = bs * mb, bs * nbc
        counts = [0, 1, 5, 17, 2, 40, 3, 1, 7]
        bp, bc = _structure(rng, mb, nbc, counts)
        bits, e = exact.choose_bits(40 * bs)
        val = exact.dyadic(rng, len(bc) * bs * bs, bits, e)
        i, j, v, _ = bsr_ref.positions(nrow, ncol, bs, bp, bc, val)
        x = exact.poison(exact.dyadic(rng, ncol, bits, e), j)
        y0 = exact.dyadic(rng, nrow, bits, e)
        A = ctx.bsr(nrow, ncol, bs, bp, bc, val)
        for lanes in _lanes(bs):
            A.set_kernel(VECTOR, lanes)
            dy, read = _guarded(ctx, y0)
            ctx.apply(A, ctx.vector_from(x), dy)
            ctx.sync()
            got = read()
            assert got[nrow] == GUARD and np.array_equal(got[:nrow], exact.exact_product(nrow, i, j, v, x, e, y0=y0)), (bs, lanes)


def test_zero_size_shapes_leave_y_as_it_was(ctx):
    A = ctx.bsr(0, 5, 3, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    assert (A.info.format, A.info.nrow, A.info.nnz) == (5, 0, 0)
    ctx.apply(A, ctx.vector_from(np.ones(5)), ctx.vector(0))
    ctx.apply_transpose(A, ctx.vector(0), ctx.vector_from(np.ones(5)))
    y0 = np.arange(1.0, 11.0)
    B = ctx.bsr(10, 7, 4, np.zeros(4, np.int32), np.zeros(0, np.int32), np.zeros(0))
    assert B.info.nnz == 0 and B.info.max_row_nnz == 0
    dy = ctx.vector_from(y0)
    ctx.apply(B, ctx.vector_from(np.full(7, np.nan)), dy)
    dyt = ctx.vector_from(np.arange(7.0))
    ctx.apply_transpose(B, ctx.vector_from(np.full(10, np.nan)), dyt)
    ctx.sync()
    assert np.array_equal(dy.download(), y0) and np.array_equal(dyt.download(), np.arange(7.0))
    C = ctx.bsr_to_csr(B)
    assert (C.info.format, C.info.nrow, C.info.ncol, C.info.nnz) == (1, 10, 7, 0)
    D = ctx.csr_to_bsr(C, 4)
    a, b, v = D.download()
    assert np.array_equal(a, np.zeros(4)) and len(b) == 0 and len(v) == 0


# ---- conversions ---------------------------------------------------------------------------------------------------------------------
def _csr_inputs():
    rng = np.random.default_rng(9)
    nrow, ncol = 300, 290
    cols = np.sort(np.stack([rng.choice(ncol, size=5, replace=False) for _ in range(nrow)]), axis=1)
    rp = (5 * np.arange(nrow + 1)).astype(np.int32)
    val = rng.uniform(0.5, 2.0, size=5 * nrow) * rng.choice([-1.0, 1.0], size=5 * nrow)
    plain = (nrow, ncol, rp, cols.reshape(-1).astype(np.int32), val)
    # duplicates: every row's second entry repeated twice more behind the row's others (unsorted, three values on one position)
    dcols = np.concatenate([cols, cols[:, 1:2], cols[:, 1:2]], axis=1)
    dval = rng.uniform(0.5, 2.0, size=7 * nrow) * rng.choice([-1.0, 1.0], size=7 * nrow)
    dup = (nrow, ncol, (7 * np.arange(nrow + 1)).astype(np.int32), dcols.reshape(-1).astype(np.int32), dval)
    # rows 40 .. 79 empty: whole block rows without a block for every bs
    keep = np.ones(nrow, dtype=bool)
    keep[40:80] = False
    counts = np.where(keep, 5, 0)
    erp = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    empty = (nrow, ncol, erp, cols[keep].reshape(-1).astype(np.int32), val[np.repeat(keep, 5)])
    return {"plain": plain, "duplicates": dup, "empty block row": empty}


CSR_INPUTS = _csr_inputs()


def _gate(nrow, ncol, bs, bp, bc, bv, x, y0, got, what):
    ref = bsr_ref.product(nrow, ncol, bs, bp, bc, bv, x, y0)
    scale, t = bsr_ref.abs_product(nrow, ncol, bs, bp, bc, bv, x)
    bound = (t + 1) * 2.0**-52 * (scale + np.abs(y0))
    err = np.abs((got.astype(np.longdouble) - ref).astype(np.float64))
    worst = float(np.max(err / np.maximum(bound, 1e-300), initial=0.0))
    print(f"{what}: worst error / bound = {worst:.3f}")
    assert np.all(err <= bound), f"{what}: {worst:.3f} of the bound"


@pytest.mark.parametrize("bs", range(2, 9))
@pytest.mark.parametrize("which", list(CSR_INPUTS))
def test_conversions_equal_the_twin_and_the_products_agree(ctx, which, bs):
    nrow, ncol, rp, col, val = CSR_INPUTS[which]
    A = ctx.csr(nrow, ncol, rp, col, val)
    B = ctx.csr_to_bsr(A, bs)
    bp, bc, bv = bsr_ref.csr_to_bsr(nrow, ncol, rp, col, val, bs)
    a, b, v = B.download()
    assert np.array_equal(a, bp) and np.array_equal(b, bc) and np.array_equal(v, bv), f"{which} bs {bs}: csr_to_bsr"
    B.validate()
    mb = -(-nrow // bs)
    assert (B.info.format, B.info.ell_k, B.info.nnz, B.info.max_row_nnz) == (5, bs, len(bc) * bs * bs, int(np.max(np.diff(bp))) * bs)
    if which == "empty block row":
        assert np.any(np.diff(bp) == 0) and len(bp) == mb + 1
    for drop in (True, False):
        C = ctx.bsr_to_csr(B, drop_zeros=drop)
        for got, want in zip(C.download(), bsr_ref.bsr_to_csr(nrow, ncol, bs, bp, bc, bv, drop)):
            assert np.array_equal(got, want), f"{which} bs {bs}: bsr_to_csr(drop_zeros={drop})"
        C.validate()
        if drop and which != "duplicates":  # the round-trip identity
            for got, want in zip(C.download(), (rp, col, val)):
                assert np.array_equal(got, want), f"{which} bs {bs}: round trip"
    # the BSR product against the twin in long double, and against the product of the CSR handle it came from, both in the gate
    rng = np.random.default_rng(3)
    x, y0 = rng.uniform(-1.0, 1.0, size=ncol), rng.uniform(-1.0, 1.0, size=nrow)
    dx, dyb, dya = ctx.vector_from(x), ctx.vector_from(y0), ctx.vector_from(y0)
    ctx.apply(B, dx, dyb)
    ctx.apply(A, dx, dya)
    ctx.sync()
    yb, ya = dyb.download(), dya.download()
    _gate(nrow, ncol, bs, bp, bc, bv, x, y0, yb, f"{which} bs {bs}: BSR product")
    # (each product within its own gate of its own exact sum; the two sums differ by the rounding of the duplicates' sums, at
    # most two additions per stored position: 2 * 2^-52 of the CSR entries' |a||x|)
    scale, t = bsr_ref.abs_product(nrow, ncol, bs, bp, bc, bv, x)
    rows = np.repeat(np.arange(nrow), np.diff(rp))
    scale_c = np.zeros(nrow)
    np.add.at(scale_c, rows, np.abs(val) * np.abs(x[col]))
    bound = 2.0**-52 * ((t + 1) * (scale + np.abs(y0)) + (np.diff(rp) + 1 + 2) * (scale_c + np.abs(y0)))
    assert np.all(np.abs(yb - ya) <= bound), f"{which} bs {bs}: BSR against CSR"
    xt, yt0 = rng.uniform(-1.0, 1.0, size=nrow), rng.uniform(-1.0, 1.0, size=ncol)
    dyt = ctx.vector_from(yt0)
    ctx.apply_transpose(B, ctx.vector_from(xt), dyt)
    ctx.sync()
    tp, tc, tv = bsr_ref.transpose(nrow, ncol, bs, bp, bc, bv)
    _gate(ncol, nrow, bs, tp, tc, tv, xt, yt0, dyt.download(), f"{which} bs {bs}: transposed BSR product")


def test_unsorted_block_columns_convert_in_stable_column_order(ctx):
    rng = np.random.default_rng(21)
    bs, mb, nbc = 3, 11, 30
    nrow, ncol = bs * mb - 1, bs * nbc - 2
    bp, bc = _structure(rng, mb, nbc, [0, 4, 1, 9, 30, 2, 0, 3, 5, 1, 7])
    bv = rng.uniform(0.5, 2.0, size=len(bc) * bs * bs)
    B = ctx.bsr(nrow, ncol, bs, bp, bc, bv)
    for got, want in zip(ctx.bsr_to_csr(B).download(), bsr_ref.bsr_to_csr(nrow, ncol, bs, bp, bc, bv)):
        assert np.array_equal(got, want)


def test_rounding_gate_on_non_dyadic_values(ctx):
    rng = np.random.default_rng(31)
    for bs in range(2, 9):
        mb, nbc = 37, 300
        nrow, ncol = bs * mb - 1, bs * nbc - (bs - 1)
        S = 64 // (bs * bs)
        counts = [[1, S, 0, S + 1, 1][i % 5] for i in range(mb)]
        counts[20] = 300
        bp, bc = _structure(rng, mb, nbc, counts)
        bv = rng.standard_normal(len(bc) * bs * bs)
        x, y0 = rng.standard_normal(ncol), rng.standard_normal(nrow)
        A = ctx.bsr(nrow, ncol, bs, bp, bc, bv)
        for lanes in _lanes(bs):
            A.set_kernel(VECTOR, lanes)
            dy = ctx.vector_from(y0)
            ctx.apply(A, ctx.vector_from(x), dy)
            ctx.sync()
            _gate(nrow, ncol, bs, bp, bc, bv, x, y0, dy.download(), f"bs {bs} lanes {lanes}")


# ---- set-up kernels past one trip of their grid (tests/tiled.py) ---------------------------------------------------------------------------
TRIP = tiled.max_grid() * tiled.block_lanes()  # items of one trip of a grid-stride kernel of csrc/convert_bsr.hip


def _tiled_case(bs):
    base = bsr_ref.tiled_base(bs)
    k, cond = bsr_ref.tiled_copies(bs, base, TRIP)
    assert all(cond.values()), (bs, k, cond)
    return base, k


def _where(nrow0):
    return lambda copy, row: f"scalar row {copy * nrow0 + row}, trip {(copy * nrow0 + row) // TRIP} of the row kernels"


@pytest.mark.parametrize("bs", (2, 3, 8))
def test_conversions_and_products_of_block_diagonal_copies_past_one_trip(ctx, bs):
    """k copies of an 8 x 9-block base: every grid-stride kernel of the set-up takes a later trip (the conditions are those of
    bsr_ref.tiled_copies, asserted here and in tests/test_bsr_ref.py), and the results are the base twin's tiled, as bytes"""
    (nrow0, ncol0, rp, cc, cv), k = _tiled_case(bs)
    nrow, ncol = k * nrow0, k * ncol0
    bp0, bc0, bv0 = bsr_ref.csr_to_bsr(nrow0, ncol0, rp, cc, cv, bs)
    print(f"bs {bs}: {k} copies, nnz {k * int(rp[-1])}, nnzb {k * len(bc0)}, stored values {k * len(bv0)}, rows {nrow}, one trip {TRIP}")
    C = ctx.csr(nrow, ncol, *tiled.tile_csr(k, ncol0, rp, cc, cv))
    B = ctx.csr_to_bsr(C, bs)
    del C
    for part, got, want in zip(("brow_ptr", "bcol", "val"), B.download(), tiled.tile_bsr(k, 9, bp0, bc0, bv0, bs)):
        assert got.dtype == want.dtype and got.shape == want.shape, f"bs {bs}: csr_to_bsr {part}"
        if got.tobytes() != want.tobytes():
            at = int(np.flatnonzero(got.view(np.uint64 if part == "val" else np.int32) != want.view(np.uint64 if part == "val" else np.int32))[0])
            raise AssertionError(f"bs {bs}: csr_to_bsr {part}[{at}] is {got[at]!r} against {want[at]!r} (copy {at // max(len(want) // k, 1)})")
    assert B.info.max_row_nnz == int(np.max(np.diff(bp0))) * bs
    for drop in (True, False):
        miss = tiled.tiled_mismatch(ctx.bsr_to_csr(B, drop_zeros=drop).download(), bsr_ref.bsr_to_csr(nrow0, ncol0, bs, bp0, bc0, bv0, drop), k, ncol0, _where(nrow0))
        assert miss is None, f"bs {bs}: bsr_to_csr(drop_zeros={drop}): {miss}"
    # the products: the base's exact y tiled (a stored 0.0 multiplies its x: every column of a stored block is read)
    rng = np.random.default_rng(2600 + bs)
    i, j, v, _ = bsr_ref.positions(nrow0, ncol0, bs, bp0, bc0, bv0)
    bits, e = exact.choose_bits(4 * 9 * bs)  # (a row holds at most 4 blocks of bs positions, each the sum of at most three values)
    x0, y00 = exact.poison(exact.dyadic(rng, ncol0, bits, e), j), exact.dyadic(rng, nrow0, bits, e)
    xt0, yt00 = exact.poison(exact.dyadic(rng, nrow0, bits, e), i), exact.dyadic(rng, ncol0, bits, e)
    dy, dyt = ctx.vector_from(np.tile(y00, k)), ctx.vector_from(np.tile(yt00, k))
    ctx.apply(B, ctx.vector_from(np.tile(x0, k)), dy)
    ctx.apply_transpose(B, ctx.vector_from(np.tile(xt0, k)), dyt)
    ctx.sync()
    for what, got, want0 in (("forward", dy.download(), exact.exact_product(nrow0, i, j, v, x0, e, y0=y00)),
                             ("transposed", dyt.download(), exact.exact_product(ncol0, j, i, v, xt0, e, y0=yt00))):
        bad = np.flatnonzero(got.view(np.uint64) != np.tile(want0, k).view(np.uint64))
        assert len(bad) == 0, f"bs {bs}: {what} product: {len(bad)} outputs differ, the first is {bad[0]} (copy {bad[0] // len(want0)}, output {bad[0] % len(want0)})"
    RUNS["tiled"] += 1


def test_unsorted_blocks_past_one_trip_and_a_block_column_out_of_range_in_the_last_block(ctx, pkg):
    """the sort path of bsr_to_csr (block_order_check, sort_ids_by_key twice, gather_i32) at nnzb > one trip: an uploaded handle whose
    blocks stand in random order inside the block rows gives the base twin - which sorts them stably - tiled"""
    bs = 2
    (nrow0, ncol0, rp, cc, cv), k = _tiled_case(bs)
    bp0, bc0, bv0 = bsr_ref.csr_to_bsr(nrow0, ncol0, rp, cc, cv, bs)
    sc0, sv0 = bsr_ref.shuffle_blocks(np.random.default_rng(7), bp0, bc0, bv0, bs)
    assert k * len(bc0) > TRIP and not np.array_equal(sc0, bc0)
    bp, bc, bv = tiled.tile_bsr(k, 9, bp0, sc0, sv0, bs)
    B = ctx.bsr(k * nrow0, k * ncol0, bs, bp, bc, bv)
    for drop in (True, False):
        want0 = bsr_ref.bsr_to_csr(nrow0, ncol0, bs, bp0, sc0, sv0, drop)
        for a, b in zip(want0, bsr_ref.bsr_to_csr(nrow0, ncol0, bs, bp0, bc0, bv0, drop)):
            assert a.tobytes() == b.tobytes()  # (distinct block columns: the stable order is the ascending one)
        miss = tiled.tiled_mismatch(ctx.bsr_to_csr(B, drop_zeros=drop).download(), want0, k, ncol0, _where(nrow0))
        assert miss is None, f"bsr_to_csr(drop_zeros={drop}) of unsorted blocks: {miss}"
    del B
    bad = bc.copy()
    bad[-1] = 9 * k  # = nbc, in the last block: the validation's later trip
    with pytest.raises(pkg.capi.SpmvError, match="index out of range"):
        ctx.bsr(k * nrow0, k * ncol0, bs, bp, bad, bv)
    RUNS["tiled unsorted"] += 1


def test_the_longest_block_row_is_found_on_a_later_trip(ctx):
    """bsr_row_max_kernel: one trip and 5 block rows of one block each, the last of three"""
    bs, mb = 2, TRIP + 5
    bp = np.concatenate([np.arange(mb), [mb + 2]]).astype(np.int32)
    bc = np.concatenate([np.arange(mb - 1) % 3, [0, 1, 2]]).astype(np.int32)
    A = ctx.bsr(bs * mb, bs * 3, bs, bp, bc, np.ones(len(bc) * bs * bs))
    assert (A.info.nnz, A.info.max_row_nnz) == (len(bc) * bs * bs, 3 * bs)
    RUNS["row max"] += 1


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------
def _small(rng, bs=3, mb=12, nbc=15):
    nrow, ncol = bs * mb - 1, bs * nbc - 1
    bp, bc = _structure(rng, mb, nbc, [rng.integers(0, 6) for _ in range(mb)])
    return nrow, ncol, bs, bp, bc, rng.uniform(0.5, 2.0, size=len(bc) * bs * bs)


def test_validate_catches_a_block_column_out_of_range_and_a_decreasing_pointer(ctx, pkg):
    rng = np.random.default_rng(41)
    nrow, ncol, bs, bp, bc, bv = _small(rng)
    nbc = -(-ncol // bs)
    bad = bc.copy()
    bad[len(bad) // 2] = nbc
    with pytest.raises(pkg.capi.SpmvError, match="index out of range"):
        ctx.bsr(nrow, ncol, bs, bp, bad, bv)
    down = bp.copy()
    k = int(np.flatnonzero(np.diff(bp) > 0)[0]) + 1
    down[k] = down[k - 1] - 1 if down[k - 1] > 0 else down[k + 1] + 1
    with pytest.raises(pkg.capi.SpmvError, match="offsets decrease"):
        ctx.bsr(nrow, ncol, bs, down, bc, bv)


def test_download_plans_and_memory(ctx, pkg):
    rng = np.random.default_rng(43)
    nrow, ncol, bs, bp, bc, bv = _small(rng)

    def round_trip():
        A = ctx.bsr(nrow, ncol, bs, bp, bc, bv)
        a, b, v = A.download()
        assert np.array_equal(a, bp) and np.array_equal(b, bc) and np.array_equal(v, bv)
        own = 4 * (len(bp) + len(bc)) + 8 * len(bv)
        assert A.info.device_bytes == own
        # a plan: one node of format 5; on a second handle it gives the same lanes per block row without a timing launch
        assert A.info.lanes_per_row == _lanes(bs)[0]  # (a mean of 2.5 blocks per block row: one slot)
        A.set_kernel(VECTOR, _lanes(bs)[-1])
        plan = A.get_plan()
        assert pkg.capi.plan_check(plan)[0] == 5 and pkg.capi.plan_check(plan)[2] == 1
        B = ctx.bsr(nrow, ncol, bs, bp, bc, bv)
        assert B.info.lanes_per_row != A.info.lanes_per_row
        B.set_plan(plan)
        assert B.info.lanes_per_row == A.info.lanes_per_row and B.get_param("select_candidates") == 0
        assert B.get_plan() == plan
        with pytest.raises(pkg.capi.SpmvError, match="spmv_mat_set_kernel"):
            A.set_kernel(PANEL, 0)
        with pytest.raises(pkg.capi.SpmvError, match="spmv_mat_set_kernel"):
            A.set_kernel(VECTOR, 16)  # no multiple of bs * bs = 9
        # the transposed handle's memory is the handle's: counted at transpose_setup, gone with the handle
        assert A.get_param("transpose_ready") == 0
        A.transpose_setup()
        comp = 4 * (-(-ncol // bs) + 1 + len(bc)) + 8 * len(bv)
        assert A.info.device_bytes == own + comp and A.get_param("transpose_bytes") == comp
        A.transpose_setup()
        assert A.info.device_bytes == own + comp
        C = ctx.bsr_to_csr(A)
        D = ctx.csr_to_bsr(C, bs)
        del A, B, C, D
        ctx.sync()

    round_trip()  # (what the context itself keeps grows on first use)
    before = ctx.mem_info()[0]
    round_trip()
    assert ctx.mem_info()[0] == before, "handles, companions and set-up memory go back"


# ---- solvers ----------------------------------------------------------------------------------------------------------------------------
def _kron_system():
    n, bs = 200, 3
    S = np.array([[4.0, 1.0, 0.0], [1.0, 3.0, 1.0], [0.0, 1.0, 2.0]])
    bp, bc, blocks = [0], [], []
    for i in range(n):
        for j, t in ((i - 1, -1.0), (i, 2.0), (i + 1, -1.0)):
            if 0 <= j < n:
                bc.append(j)
                blocks.append(t * S)
        bp.append(len(bc))
    return n * bs, bs, np.array(bp, np.int32), np.array(bc, np.int32), np.concatenate([b.reshape(-1) for b in blocks])


def test_solvers_run_on_a_bsr_handle(ctx):
    n, bs, bp, bc, bv = _kron_system()
    A = ctx.bsr(n, n, bs, bp, bc, bv)
    C = ctx.bsr_to_csr(A)
    assert C.info.nnz == np.count_nonzero(bv)
    rng = np.random.default_rng(51)
    b = rng.standard_normal(n)
    db = ctx.vector_from(b)
    dense = bsr_ref.dense(n, n, bs, bp, bc, bv)

    def solve(run):
        out = []
        for M in (A, C):
            dx = ctx.vector_from(np.zeros(n))
            res = run(M, dx)
            ctx.sync()
            out.append((dx.download(), res))
        return out

    # (solved to 1e-12 so that the two handles' solutions, each within cond(A) * its residual of the true one, can agree to 1e-8)
    for name, run in (("cg", lambda M, dx: ctx.cg(M, db, dx, max_iter=20000, rel_tol=1e-12)),
                      ("gmres", lambda M, dx: ctx.gmres(M, db, dx, restart=64, max_iter=60000, rel_tol=1e-12))):
        (xb, rb), (xc, rc) = solve(run)
        assert rb[1] <= 1e-10 and rc[1] <= 1e-10, (name, rb, rc)
        assert np.linalg.norm(b - dense @ xb) <= 1e-9 * np.linalg.norm(b), name
        assert np.linalg.norm(xb - xc) <= 1e-8 * np.linalg.norm(xc), (name, np.linalg.norm(xb - xc) / np.linalg.norm(xc))
    # least squares: the same number of steps over A and A^T on both handles
    (xb, rb), (xc, rc) = solve(lambda M, dx: ctx.cgls(M, db, dx, max_iter=40, rel_tol=1e-30))
    assert rb[0] == rc[0] == 40 and A.get_param("transpose_ready") == 1
    assert np.linalg.norm(xb - xc) <= 1e-8 * np.linalg.norm(xc)
    assert np.linalg.norm(b - dense @ xb) < np.linalg.norm(b)


# ---- one statement about the clock -------------------------------------------------------------------------------------------------------------
def test_band_product_against_its_csr_handle(ctx):
    """bs = 4, 250k block rows of 8 blocks (1M scalar rows of 32) in a band of 16384 blocks: the BSR product within the gate of its
    CSR handle's, and - recorded under -m gpu, asserted under gpu_perf - no slower than it"""
    rng = np.random.default_rng(61)
    bs, mb, per, band = 4, 250_000, 8, 16384
    n = bs * mb
    bc = np.sort(np.clip(np.arange(mb)[:, None] + rng.integers(-band // 2, band // 2, size=(mb, per)), 0, mb - 1), axis=1).astype(np.int32).reshape(-1)
    bp = (per * np.arange(mb + 1)).astype(np.int32)
    bv = rng.uniform(0.5, 1.5, size=len(bc) * bs * bs)
    A = ctx.bsr(n, n, bs, bp, bc, bv)
    C = ctx.bsr_to_csr(A)
    assert C.info.nnz == len(bv) and A.info.lanes_per_row == 16  # (8 blocks per block row: one slot)
    x = rng.uniform(-1.0, 1.0, size=n)
    dx, dya, dyc = ctx.vector_from(x), ctx.vector_from(np.zeros(n)), ctx.vector_from(np.zeros(n))
    ctx.apply(A, dx, dya)
    ctx.apply(C, dx, dyc)
    ctx.sync()
    ya, yc = dya.download(), dyc.download()
    rows = np.repeat(np.arange(mb), per)
    absx = np.abs(x).reshape(mb, bs)
    scale = np.zeros((mb, bs))
    np.add.at(scale, rows, np.einsum("brc,bc->br", np.abs(bv).reshape(-1, bs, bs), absx[bc]))
    assert np.all(np.abs(ya - yc) <= 2 * (per * bs + 1) * 2.0**-52 * scale.reshape(-1))
    t_bsr, t_csr = [], []
    for _ in range(3):  # interleaved
        t_bsr.append(ctx.apply_timed(A, dx, dya, 20))
        t_csr.append(ctx.apply_timed(C, dx, dyc, 20))
    m_bsr, m_csr = float(np.median(t_bsr)), float(np.median(t_csr))
    print(f"bs 4 band, 1M rows: BSR {m_bsr:.4f} ms, CSR kernel {C.info.kernel} {m_csr:.4f} ms, ratio {m_csr / m_bsr:.3f}")
    perf_expect(m_bsr <= m_csr, f"the bs = 4 band product takes {m_bsr:.4f} ms, its CSR AUTO handle (kernel {C.info.kernel}) {m_csr:.4f} ms")


# ---- coverage -------------------------------------------------------------------------------------------------------------------------
def test_every_instance_of_the_kernel_ran():
    """every bsr_vector_kernel<BS, G, EDGE> that bsr_apply's switch can launch ran under exact values: the 15 cases of the switch
    (read from csrc/kernels_bsr.hip), with and without the column edge"""
    expect = {"exact": 7, "edges": 7, "entry points": 7, "tiled": 3, "tiled unsorted": 1, "row max": 1}
    if any(RUNS[f] != c for f, c in expect.items()):
        pytest.skip(f"the coverage check needs every test of this module (ran {dict(RUNS)}, expected {expect})")
    cases = tiled.bsr_kernel_cases()
    assert len(cases) == 15 and set(cases) == {(bs, lanes // (bs * bs)) for bs in range(2, 9) for lanes in _lanes(bs)}
    need = {(bs, g, edge) for bs, g in cases for edge in (True, False)}
    print(f"{len(INSTANCES)} instances of bsr_vector_kernel ran: {sorted(INSTANCES)}")
    assert len(need) == 30 and INSTANCES == need, f"never ran: {sorted(need - INSTANCES)}; not in the switch: {sorted(INSTANCES - need)}"
