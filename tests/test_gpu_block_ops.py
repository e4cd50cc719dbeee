"""spmv_block_gram (G = U^T V) and spmv_block_combine (Out = S C) on the GPU (csrc/block_ops.hip).

Written against the kernels' tiles: the Gram kernel stages row tiles of 32 rows and its COLUMN TILE is 16 (register tiles for up to 16,
32, 48 and 96 columns, chosen for p and q separately: the edges are 16 | 17, 32 | 33, 48 | 49 and the limit 96); at most 512
workgroups, so from n = 32 * 512 rows on a workgroup takes more than one tile (n = 20001, 70001 and the block beyond every grid).  The
combine kernel takes row tiles of 64 and output
columns in four groups of 2, 4, 8, 12 or 24 (edges 8 | 9, 16 | 17, 32 | 33, 48 | 49, limit 96).

Exact cases: every entry is dyadic (tests/exact.py: a small integer over a power of two, sized so that every sum of the call is exact in
any order), so the GPU's result must equal the integer reference BIT FOR BIT: a dropped, doubled or misplaced term, a padding row or a
zero-filled tile slot that leaks in, all change the bits.  With ld = n + 37 the padding rows hold NaN: every result must be finite, and
behind block_combine the padding must still hold those NaN bits.  On random input: two calls agree bit for bit, the Gram matrix is
within the bound of a sum of n products of the long double one, it is exactly symmetric for U = V, and block_combine equals the
fma-ordered ascending sum bit for bit (fma emulated exactly in rationals).
"""
import collections
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import exact

pytestmark = pytest.mark.gpu
RUNS = collections.Counter()
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 4099)
# p from {1, 2, 3, 7, 8, 9, 16, 17, 47, 48}, q from those and 95, 96: every value on both sides, every tile edge on both sides
PAIRS = ((1, 1), (2, 3), (3, 2), (7, 9), (8, 8), (9, 7), (16, 16), (16, 17), (17, 16), (17, 17), (47, 95), (48, 96), (48, 48), (47, 47), (1, 96), (48, 1),
         (3, 95), (9, 48), (2, 47), (7, 2), (8, 3), (16, 9), (17, 8), (1, 7))
BIG_PAIRS = ((1, 1), (2, 3), (3, 2), (3, 3))
PAD = 37
_NAN = np.float64(np.nan)


def _big_n():
    """2 * kMaxGrid * kBlock + 2051 with the constants as csrc/common.hpp defines them: beyond 512 row tiles of either kernel by far, odd"""
    text = (Path(__file__).resolve().parent.parent / "arm-spmv_amd" / "csrc" / "common.hpp").read_text()
    vals = {}
    for name, expr in re.findall(r"constexpr int (k\w+)\s*=\s*([^;]+);", text):
        try:
            vals[name] = int(eval(expr, {"__builtins__": {}}, dict(vals)))
        except Exception:
            pass
    return 2 * vals["kMaxGrid"] * vals["kBlock"] + 2051


def _pack(M, ld, cols=None):
    """the block of M (n, p) as a flat array with leading dimension ld, padding rows NaN; cols: columns the array has room for"""
    n, p = M.shape
    cols = p if cols is None else cols
    buf = np.full((cols - 1) * ld + n, _NAN)
    for c in range(p):
        buf[c * ld:c * ld + n] = M[:, c]
    return buf


def _unpack(buf, n, ld, cols):
    return np.column_stack([buf[c * ld:c * ld + n] for c in range(cols)])


def _padding(buf, n, ld, cols):
    return np.concatenate([buf[c * ld + n:(c + 1) * ld] for c in range(cols - 1)]) if cols > 1 else np.zeros(0)


def _device(ctx, host, offset8=False):
    """host on the device: a vector of its own, or a wrapped pointer 8 bytes past a 16-byte boundary into a vector of one more entry"""
    if not offset8:
        v = ctx.vector_from(host)
        assert v.device_ptr % 16 == 0
        return v, None
    base = ctx.vector(len(host) + 1)
    base.fill(0.0)
    assert (base.device_ptr + 8) % 16 == 8
    v = ctx.wrap_vector(base.device_ptr + 8, len(host))
    v.upload(host)
    return v, base


def _exact_case(ctx, rng, n, p, q, ld, offset8):
    """Gram (U, V and U = V) and combine (out of place and in place) of one shape on dyadic inputs; returns what went wrong"""
    bad = []
    tag = f"n={n} p={p} q={q} ld={ld}{' offset8' if offset8 else ''}"
    # ---- Gram: sums of n products
    bits, e = exact.choose_bits(n)
    U, iU = exact.draw(rng, (n, p), bits, e)
    V, iV = exact.draw(rng, (n, q), bits, e)
    dU, keepU = _device(ctx, _pack(U, ld), offset8)
    dV, keepV = _device(ctx, _pack(V, ld), offset8)
    G = ctx.block_gram(n, p, dU, ld, q, dV, ld)
    ref = np.ldexp((iU.T @ iV).astype(np.float64), -2 * e)
    if not np.array_equal(G, ref):
        bad.append(f"{tag}: U^T V differs from the integer reference in {np.count_nonzero(G != ref)} of {p * q} entries")
    GU = ctx.block_gram(n, p, dU, ld, p, dU, ld)
    refU = np.ldexp((iU.T @ iU).astype(np.float64), -2 * e)
    if not (np.array_equal(GU, refU) and np.array_equal(GU, GU.T)):
        bad.append(f"{tag}: U^T U differs from the integer reference, or is not symmetric")
    del dU, dV, keepU, keepV
    # ---- combine: sums of p products
    bits, e = exact.choose_bits(p)
    S, iS = exact.draw(rng, (n, p), bits, e)
    Cm, iC = exact.draw(rng, (p, q), bits, e)
    refO = np.ldexp((iS @ iC).astype(np.float64), -2 * e)
    cols = max(p, q)
    hostS = _pack(S, ld, cols)
    for in_place in (False, True):
        dS, keepS = _device(ctx, hostS, offset8)
        if in_place:
            dO, keepO, before = dS, None, hostS
        else:
            before = np.full((q - 1) * ld + n, _NAN)
            dO, keepO = _device(ctx, before, offset8)
        ctx.block_combine(n, p, dS, ld, q, Cm, dO, ld)
        ctx.sync()
        got = dO.download()
        out = _unpack(got, n, ld, q)
        what = "in place" if in_place else "out of place"
        if not np.array_equal(out, refO):
            bad.append(f"{tag}: S C {what} differs from the integer reference in {np.count_nonzero(out != refO)} of {n * q} entries")
        if not np.array_equal(_padding(got, n, ld, q).view(np.uint64), _padding(before, n, ld, q).view(np.uint64)):
            bad.append(f"{tag}: S C {what} wrote into the padding rows")
        if not in_place and not np.array_equal(dS.download().view(np.uint64), hostS.view(np.uint64)):
            bad.append(f"{tag}: S C out of place changed S")
        del dS, dO, keepS, keepO
    return bad


@pytest.mark.parametrize("n", SIZES)
def test_dyadic_blocks_give_the_integer_reference_bit_for_bit(ctx, n):
    rng = np.random.default_rng(1000 + n)
    bad = []
    for i, (p, q) in enumerate(PAIRS):
        for ld in (n, n + PAD):
            bad += _exact_case(ctx, rng, n, p, q, ld, offset8=(i + (ld != n)) % 3 == 0)
    assert not bad, "\n".join(bad[:20])
    RUNS["exact"] += 1


def test_a_block_beyond_every_grid_gives_the_integer_reference(ctx):
    n = _big_n()
    assert n > 64 * 2048 * 2 and n % 2 == 1
    rng = np.random.default_rng(7)
    bad = []
    for i, (p, q) in enumerate(BIG_PAIRS):
        bad += _exact_case(ctx, rng, n, p, q, n + PAD if i % 2 else n, offset8=i == 1)
    assert not bad, "\n".join(bad)
    RUNS["big"] += 1


def _fma(a, b, c):
    """fma(a, b, c) of three doubles, exactly: the rational a b + c rounded once (to nearest, ties to even)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


@pytest.mark.parametrize("n,p,q", [(130, 17, 9), (65, 48, 33), (257, 9, 96)])
def test_combine_on_random_input_is_the_ascending_fma_chain_bit_for_bit(ctx, n, p, q):
    rng = np.random.default_rng(n + p + q)
    S, Cm = rng.standard_normal((n, p)), rng.standard_normal((p, q))
    ld = n + PAD
    dS, _ = _device(ctx, _pack(S, ld))
    dO, _ = _device(ctx, np.full((q - 1) * ld + n, _NAN))
    out = []
    for _ in range(2):
        ctx.block_combine(n, p, dS, ld, q, Cm, dO, ld)
        ctx.sync()
        out.append(_unpack(dO.download(), n, ld, q))
    assert out[0].tobytes() == out[1].tobytes(), "two calls on the same data differ"
    rows = (0, 1, 63, 64, n - 1)  # (every row is the same function of its own entries: a few of them, every column)
    for i in rows:
        for j in range(q):
            acc = 0.0
            for k in range(p):
                acc = _fma(S[i, k], Cm[k, j], acc)
            assert out[0][i, j] == acc, (i, j, out[0][i, j], acc)
    ref = (S.astype(np.longdouble) @ Cm.astype(np.longdouble))
    bound = (p + 2) * np.finfo(np.float64).eps * (np.abs(S) @ np.abs(Cm))
    assert np.all(np.abs(out[0] - ref) <= bound)
    RUNS["combine random"] += 1


@pytest.mark.parametrize("n,p,q", [(4099, 48, 96), (4099, 17, 7), (65, 96, 96), (20001, 9, 33), (70001, 48, 48)])
def test_gram_on_random_input_is_reproducible_and_within_the_bound_of_a_sum(ctx, n, p, q):
    rng = np.random.default_rng(n + p + q)
    U, V = rng.standard_normal((n, p)), rng.standard_normal((n, q))
    ld = n + PAD
    dU, _ = _device(ctx, _pack(U, ld))
    dV, _ = _device(ctx, _pack(V, ld), offset8=True)
    G1, G2 = ctx.block_gram(n, p, dU, ld, q, dV, ld), ctx.block_gram(n, p, dU, ld, q, dV, ld)
    assert G1.tobytes() == G2.tobytes(), "two calls on the same data differ"
    ref = U.astype(np.longdouble).T @ V.astype(np.longdouble)
    bound = (n + 2) * np.finfo(np.float64).eps * (np.abs(U).T @ np.abs(V))
    err = np.abs(G1 - ref)
    print(f"n={n} p={p} q={q}: max |G - G_longdouble| / bound = {float(np.max(err / bound)):.3e}")
    assert np.all(np.isfinite(G1)) and np.all(err <= bound)
    GU = ctx.block_gram(n, p, dU, ld, p, dU, ld)
    assert np.array_equal(GU, GU.T), "U^T U is not exactly symmetric"
    assert np.all(np.abs(GU - U.astype(np.longdouble).T @ U.astype(np.longdouble)) <= (n + 2) * np.finfo(np.float64).eps * (np.abs(U).T @ np.abs(U)))
    RUNS["gram random"] += 1


def test_refusals_on_live_vectors_and_an_empty_block(ctx, pkg):
    capi = pkg.capi
    U, V = ctx.vector(400), ctx.vector(500)
    U.fill(1.0)
    V.fill(1.0)

    def refused(f, needle):
        with pytest.raises(capi.SpmvError) as e:
            f()
        assert e.value.code == -1 and needle in str(e.value), str(e.value)

    refused(lambda: ctx.block_gram(100, 5, U, 100, 5, V, 100), "too short")
    refused(lambda: ctx.block_gram(100, 4, U, 99, 5, V, 100), "at least n")
    refused(lambda: ctx.block_gram(100, 97, U, 100, 5, V, 100), "columns")
    refused(lambda: ctx.block_gram(-1, 4, U, 100, 5, V, 100), "rows")
    refused(lambda: ctx.block_combine(100, 4, U, 100, 6, np.zeros((4, 6)), V, 100), "too short")
    refused(lambda: ctx.block_combine(100, 4, V, 100, 4, np.zeros((4, 4)), ctx.wrap_vector(V.device_ptr + 8 * 100, 400), 100), "overlap")
    refused(lambda: ctx.block_combine(100, 4, V, 100, 0, np.zeros((4, 0)), U, 100), "columns")
    assert np.array_equal(ctx.block_gram(100, 4, U, 100, 5, V, 100), np.full((4, 5), 100.0))
    assert not ctx.block_gram(0, 4, U, 0, 5, V, 0).any()
    ctx.block_combine(0, 4, U, 0, 5, np.ones((4, 5)), V, 0)
    ctx.sync()
    assert np.array_equal(V.download(), np.ones(500))
    RUNS["refusals"] += 1


def test_every_case_ran():
    expect = {"exact": len(SIZES), "big": 1, "combine random": 3, "gram random": 5, "refusals": 1}
    if any(RUNS[f] != c for f, c in expect.items()):
        pytest.skip(f"the coverage check needs every test of this module (ran {dict(RUNS)}, expected {expect})")
    seen_p, seen_q = {p for p, _ in PAIRS}, {q for _, q in PAIRS}
    assert seen_p == {1, 2, 3, 7, 8, 9, 16, 17, 47, 48} and seen_q == seen_p | {95, 96}
