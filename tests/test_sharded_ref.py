"""The CPU references of the sharded solver step (tests/sharded_ref.py) against Python-integer arithmetic - no GPU.

tests/child_sharded_ops.py and tests/child_sharded_ranks.py compare dist.HipShardOps with these references bit for bit.  That
is only a test if (a) every sum the engine may form, in whatever order, is exact on these inputs, and (b) the references are
right.  Both are settled here, in Python integers, for every (n, world) the GPU tests run and every rank."""
import numpy as np
import pytest

import exact as ex
import sharded_ref as sr


@pytest.fixture(scope="module", params=sr.OPS_CASES, ids=lambda c: f"n{c[0]}-world{c[1]}")
def problem(request):
    return sr.OpsProblem(*request.param)


def _ints(a, e):
    return [int(v) for v in ex.scaled(a, e)]


def _int_product(nout, out_idx, in_idx, iv, ix, acc=None):
    acc = [0] * nout if acc is None else list(acc)
    for o, i, v in zip(out_idx, in_idx, iv):
        acc[int(o)] += v * ix[int(i)]
    return acc


def _floats(acc, e):
    return np.array([float(np.ldexp(float(a), -e)) for a in acc], dtype=np.float64)


def _split_by_hand(srp, scol, sval, c0, c1):
    """row by row, entry by entry: what spmv_csr_split_columns documents"""
    parts = {True: ([0], [], []), False: ([0], [], [])}
    for i in range(len(srp) - 1):
        for j in range(srp[i], srp[i + 1]):
            inside = c0 <= scol[j] < c1
            parts[inside][1].append(int(scol[j]) - (c0 if inside else 0))
            parts[inside][2].append(float(sval[j]))
        for rp, cols, _ in parts.values():
            rp.append(len(cols))
    return parts[True], parts[False]


def test_the_bound_is_a_bound():
    """fits_53 at its edge, in integers: the last shape it admits stays below 2^53 in the worst case, the next does not"""
    assert sr.fits_53(5, 3, 300, 1003) and not sr.fits_53(6, 3, 300, 1003) and not sr.fits_53(5, 4, 300, 1003)
    for bits, e, longest, length in ((5, 3, 300, 1003), (9, 3, 40, 5), (3, 3, 10_000, 40_000)):
        worst_term = ((2**bits - 1) * 2 ** (2 * e)) ** 3  # three factors of (2^bits - 1) 2^e each, on the grid 2^-3e
        total = (length * longest + length) * worst_term
        assert (total < 2**53) or not sr.fits_53(bits, e, longest, length), (bits, e, longest, length)
    with pytest.raises(ValueError):
        sr.choose_bits(10**6, 10**6)


def test_every_sum_of_every_case_fits_53_bits(problem):
    """the condition, not a tolerance: w . (A p) over the whole matrix (any rank's share is a part of it), with a starting
    vector's worth of terms on top, and every column of |y0| + |A|^T |x|, as Python integers on the grids the sums live on"""
    P, e = problem, problem.e
    assert sr.fits_53(P.bits, e, P.longest, P.n) and P.bits >= 3
    assert P.longest == max(int(np.max(np.diff(P.rp))), int(np.bincount(P.cc, minlength=P.n).max()))
    iv, ip, iw, ix, iy0 = (_ints(a, e) for a in (P.cv, P.p, P.w, P.x, P.y0))
    row_abs = _int_product(P.n, P.rows, P.cc, [abs(v) for v in iv], [abs(v) for v in ip])
    dot_abs = sum(abs(w) * q for w, q in zip(iw, row_abs))  # grid 2^-3e; the q the inside part leaves behind is part of the same terms
    assert dot_abs < 2**53 and max(row_abs) < 2**53, dot_abs
    col_abs = _int_product(P.n, P.cc, P.rows, [abs(v) for v in iv], [abs(v) for v in ix], acc=[abs(v) * 2**e for v in iy0])
    assert max(col_abs) < 2**53  # grid 2^-2e
    assert max(abs(v) for v in iv + ip + iw + ix + iy0) < 2 ** (P.bits + 2 * e)  # every factor is what fits_53 assumes


def test_rows_tile_and_the_shape_crosses_every_edge(problem):
    P = problem
    assert P.bounds[0][0] == 0 and P.bounds[-1][1] == P.n and all(P.bounds[r][1] == P.bounds[r + 1][0] for r in range(P.world - 1))
    lens = np.diff(P.rp)
    lo, hi = P.bounds[-1]
    long_row = int(np.argmax(lens))
    assert lo <= long_row < hi and lens[long_row] >= 5 * np.median(lens[lens > 0]) and np.any(lens == 0)
    if P.n == sr.N_OPS:
        assert P.world == 1 or P.n % P.world != 0
        for r in range(P.world):  # every rank's rows reach into every other rank's column range, and into its own
            _, scol, _ = P.shard(r)
            for b, e_ in P.bounds:
                assert np.any((scol >= b) & (scol < e_)), (r, b, e_)
    else:
        assert sum(1 for b, e_ in P.bounds if b == e_) == P.world - 1 and P.bounds[-1] == (0, P.n)


def test_split_twin_and_products_in_integers(problem):
    """for every rank: the twin equals the entry-by-entry split; inside * x[c0:c1] + outside * x equals the shard's rows of A x;
    the float references (want_product, its dot) are those integers"""
    P, e = problem, problem.e
    iv, ip, iw = (_ints(a, e) for a in (P.cv, P.p, P.w))
    whole = _int_product(P.n, P.rows, P.cc, iv, ip)
    for r, (lo, hi) in enumerate(P.bounds):
        srp, scol, sval = P.shard(r)
        assert srp[0] == 0 and len(srp) == hi - lo + 1 and np.array_equal(scol, P.cc[P.rp[lo]:P.rp[hi]])
        rows_l = np.repeat(np.arange(hi - lo), np.diff(srp))
        for c0, c1 in ((lo, hi), (min(lo + 1, hi), hi), (lo, lo), (0, P.n)):
            m_in, m_out = sr.split_columns(srp, scol, sval, c0, c1)
            h_in, h_out = _split_by_hand(srp, scol, sval, c0, c1)
            for got, want in ((m_in, h_in), (m_out, h_out)):
                assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.float64
                assert got[0].tolist() == want[0] and got[1].tolist() == want[1] and got[2].tolist() == want[2], (r, c0, c1)
            assert len(m_in[1]) + len(m_out[1]) == len(scol)
            assert not len(m_in[1]) or (m_in[1].min() >= 0 and m_in[1].max() < c1 - c0)
            assert not np.any((m_out[1] >= c0) & (m_out[1] < c1))
            q = _int_product(hi - lo, np.repeat(np.arange(hi - lo), np.diff(m_in[0])), m_in[1], _ints(m_in[2], e), ip[c0:c1])
            q = _int_product(hi - lo, np.repeat(np.arange(hi - lo), np.diff(m_out[0])), m_out[1], _ints(m_out[2], e), ip, acc=q)
            assert q == whole[lo:hi], (r, c0, c1)
        want_q, want_dot = P.want_product(r)
        assert np.array_equal(want_q, _floats(whole[lo:hi], 2 * e))
        assert want_dot == float(np.ldexp(float(sum(w * q for w, q in zip(iw[lo:hi], whole[lo:hi]))), -3 * e))
        assert np.array_equal(want_q, _floats(_int_product(hi - lo, rows_l, scol, _ints(sval, e), ip), 2 * e))


def test_transposed_partials_add_up_in_rank_order(problem):
    """the rank-order sum of A_p^T x_p equals A^T x: in integers, and as the float64 sum reduce_transposed forms onto y0"""
    P, e = problem, problem.e
    iv, ix = _ints(P.cv, e), _ints(P.x, e)
    whole = _int_product(P.n, P.cc, P.rows, iv, ix)
    acc, y = [0] * P.n, P.y0.copy()
    for r, (lo, hi) in enumerate(P.bounds):
        srp, scol, sval = P.shard(r)
        part = _int_product(P.n, scol, np.repeat(np.arange(hi - lo), np.diff(srp)), _ints(sval, e), ix[lo:hi])
        assert np.array_equal(P.want_transpose(r), _floats(part, 2 * e)), r
        acc = [a + b for a, b in zip(acc, part)]
        y += P.want_transpose(r)
    assert acc == whole
    assert np.array_equal(P.want_transpose_whole(), _floats(whole, 2 * e))
    assert np.array_equal(y, P.want_transpose_whole(P.y0))
    assert np.array_equal(y, _floats([a + b * 2**e for a, b in zip(whole, _ints(P.y0, e))], 2 * e))
    if P.n == sr.N_OPS:
        b = sr.RAGGED_COLUMNS
        assert b[0][0] == 0 and b[-1][1] == P.n and all(b[i][1] == b[i + 1][0] for i in range(len(b) - 1)) and len(b) == 3
        assert [c[1] - c[0] for c in b] != [hi - lo for lo, hi in sr.row_bounds(P.n, 3)]


def test_blas1_references_in_integers(problem):
    P, e = problem, problem.e
    iu, iv = _ints(P.u, e), _ints(P.v, e)
    for lo, hi in P.bounds:
        want = [-6 * a + b for a, b in zip(iu[lo:hi], iv[lo:hi])]  # (-1.5 u + 0.25 v) * 2^(e + 2)
        assert np.array_equal(P.want_axpby(lo, hi), _floats(want, e + 2))
        assert np.array_equal(P.want_axpby(lo, hi), P.ALPHA * P.u[lo:hi] + P.BETA * P.v[lo:hi])  # exact in float64 as well
        assert P.want_dot(lo, hi) == float(np.ldexp(float(sum(a * b for a, b in zip(iu[lo:hi], iv[lo:hi]))), -2 * e))


@pytest.mark.parametrize("world", [w for n, w in sr.OPS_CASES if n == sr.N_OPS and w > 1])
def test_a_broken_result_differs_from_the_reference(world, orc):
    """every exact check of the GPU children can fail: the wrong-but-plausible results differ from the references in their bits"""
    P = sr.OpsProblem(sr.N_OPS, world)
    e = P.e
    whole_t = P.want_transpose_whole()
    for r, (lo, hi) in enumerate(P.bounds):
        srp, scol, sval = P.shard(r)
        want_q, want_dot = P.want_product(r)
        (rp_i, cc_i, cv_i), (rp_o, cc_o, cv_o) = sr.split_columns(srp, scol, sval, lo, hi)
        q_in = ex.exact_product(hi - lo, *ex.csr_entries(rp_i, cc_i, cv_i), P.p[lo:hi], e)
        q_out = ex.exact_product(hi - lo, *ex.csr_entries(rp_o, cc_o, cv_o), P.p, e)
        assert np.array_equal(q_in + q_out, want_q)
        assert not np.array_equal(q_out, want_q) and not np.array_equal(q_in, want_q)  # finish_remote_dot overwrote / added nothing
        assert ex.exact_dot(P.w[lo:hi], q_out, e, 2 * e) != want_dot
        if lo > 0:  # the rebase left out: the inside part reads the wrong slice of the direction (lo swapped for 0)
            unrebased = ex.exact_product(hi - lo, *ex.csr_entries(rp_i, cc_i, cv_i), P.p[:hi - lo], e)
            assert not np.array_equal(unrebased, q_in) and not np.array_equal(cc_i + lo, cc_i)
        assert np.isnan(ex.poison(P.p, cc_o)[lo:hi]).any()  # the outside part must not read the rank's own columns
        assert not np.array_equal(whole_t - P.want_transpose(r), whole_t)  # one rank's partial left out
        other = (r + 1) % P.world
        assert not np.array_equal(P.want_transpose(other)[:10], P.want_transpose(r)[:10])
    # the sweep: in another sequence, or on a block cut at the wrong place, it is further off than the gate allows
    import oracle_lib as ol
    from test_gpu_solver import _spd_random

    _, rp, cc, cv = _spd_random(P.n, 6, 9)
    lo, hi = P.bounds[-1]
    b_in, _ = sr.split_columns(*sr.shard_arrays(rp, cc, cv, lo, hi), lo, hi)
    seq = ol.greedy_colour_order(orc, b_in[0], b_in[1])[2]
    r_host = np.random.default_rng(500).uniform(-1, 1, hi - lo)
    z = {}
    for name, order in (("colours", seq), ("rows", None)):
        z[name] = np.zeros(hi - lo)
        assert ol.symgs(orc, *b_in, r_host, z[name], 1, order=order) == 0
    assert np.max(np.abs(z["colours"] - z["rows"])) / np.max(np.abs(z["rows"])) > 1e4 * ol.REL_TOL
    shifted, _ = sr.split_columns(*sr.shard_arrays(rp, cc, cv, lo - 1, hi - 1), lo - 1, hi - 1)  # the block one row off
    z_off = np.zeros(hi - lo)
    assert ol.symgs(orc, *shifted, r_host, z_off, 1) == 0
    assert np.max(np.abs(z_off - z["rows"])) / np.max(np.abs(z["rows"])) > 1e4 * ol.REL_TOL
