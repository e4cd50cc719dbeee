"""The references of tests/gmres_ref.py, checked on the CPU (no GPU): the extended-precision recurrence ends at the solution numpy
finds, every float64 twin lies inside the gate built from the other five, the drop rule at the noise floor takes nothing on these
problems, and each wrong recurrence is outside the gate within five iterations.

Observed here (x86, np.longdouble; b then x0 from default_rng(seed).uniform(-1, 1); the tests print them):
  (a) leave-one-out (one twin against the envelope of the other five), worst over n1, n2, n3, r33, r4097, band4099, m = 4 and
      m = 30, plain and Jacobi, k in (1, 2, 3, 4, 5, 8, 9, 13): from the random starts 1.35 for x (band4099, m = 4, plain) and 2.32
      for the residual (r4097, m = 4, Jacobi); from x0 = 0 0.76 (band4099, m = 4, plain) and 2.60 (r4097, m = 30, plain).  The
      wide basis (tri4099): m = 64, k in (16, 17, 33, 64, 65, 66) 1.33 and 2.00; m = 8, k in (8, 9, 16, 17) 1.49 and 1.17; m = 1, k in
      (1, 2, 3) 1.03 and 1.00.  F = 8
      holds for this file's own arithmetic with a factor of three to spare.
      Nothing is dropped, from either start: the lowest ||r|| / ||b|| of the reference before k = 13 is 2.8e-8 from the random
      starts (r33, m = 30, Jacobi) and 2.5e-9 from x0 = 0 (the same case); the wide basis stays at or above 0.116 through k = 66.
      Twin envelopes: x 8.9e-16 (the floor) .. 3.3e-15; residual 8.9e-16 .. 6.6e-15 without a restart, up to 3.6e-9 behind one
      (m = 4: |g| restarts from the recomputed ||r||, and what rounding did to x is in it); the wide basis 1.0e-14 and 6.7e-15.
  (b) mutations on r33, deviation of x_k over the gate at the first asked k that sees it (plain / Jacobi):
      rot       k = 2   2.6e13 / 1.4e13      (m = 4 and m = 30)
      g         k = 1   1.6e13 / 9.3e12
      last_col  k = 1   3.8e14 / 3.6e14
      keep_vm   k = 5   2.0e12 / 6.1e11      (m = 4: the first iterate behind a restart; m = 30 has none to see it by)
      left      k = 1   - / 5.6e12
      no_minv   k = 1   - / 2.2e15
      tail      k = 1   2.7e14 / 2.7e14
"""
import numpy as np
import pytest

import gmres_ref as gr
import precond_ops as po

SMALL = ("n1", "n2", "n3")
MID = ("r33", "r4097", "band4099")
PRECONDS = (None, "jacobi")


def _skip_unless_available(n):
    why = gr.available(n)
    if why:
        pytest.skip(why)


@pytest.fixture(scope="module")
def envelopes():
    cache = {}

    def get(name, m, precond, zero_start=False):
        key = (name, m, precond, zero_start)
        if key not in cache:
            n, ent, b, x0, ks = gr.problem(name)
            cache[key] = gr.Envelope(ent, n, b, np.zeros_like(x0) if zero_start else x0, gr.WIDE_KS[m] if name == gr.WIDE else ks, m, precond)
        return cache[key]

    return get


@pytest.mark.parametrize("precond", PRECONDS)
@pytest.mark.parametrize("m", gr.RESTARTS)
def test_the_reference_ends_at_the_solution(m, precond):
    n, ent, b, x0, ks = gr.problem("n3")
    dense = np.zeros((n, n))
    np.add.at(dense, (ent[0], ent[1]), ent[2])
    assert not np.array_equal(dense, dense.T) and ks == (1, 2, 3)
    want = np.linalg.solve(dense, b)
    x, res = gr.gmres_reference(ent, n, b, x0, (3,), m, precond)[3]
    assert np.max(np.abs(np.asarray(x, dtype=np.float64) - want)) <= 1e-12 * np.max(np.abs(want))
    assert res <= 1e-12


def test_a_restarted_run_converges_to_the_solution():
    """GMRES(4) through a dozen restarts: the iterates behind a restart are those of the recurrence, not of one long cycle"""
    n, ent, b, x0, _ = gr.problem("r33")
    dense = np.zeros((n, n))
    np.add.at(dense, (ent[0], ent[1]), ent[2])
    want = np.linalg.solve(dense, b)
    x, iters = gr.run_to_tolerance(ent, n, b, x0, 4, None, 1e-12, 400)
    assert 4 < iters < 400 and np.max(np.abs(x - want)) <= 1e-10 * np.max(np.abs(want)), iters
    long_x, long_iters = gr.run_to_tolerance(ent, n, b, x0, 30, None, 1e-12, 400)
    assert long_iters < iters and np.max(np.abs(long_x - want)) <= 1e-10 * np.max(np.abs(want)), (long_iters, iters)


def _leave_one_out(env, label):
    worst = [max(env.leave_one_out(k, what) for k in env.ks) for what in (0, 1)]
    spread = [(min(env.envelope(k, what) for k in env.ks), max(env.envelope(k, what) for k in env.ks)) for what in (0, 1)]
    print(f"{label}: kept {env.ks}, dropped {env.dropped}, lowest ||r|| / ||b|| before the last k {min(env.resid_hist[:env.ks[-1]]):.2e}; twin "
          f"envelope x {spread[0][0]:.1e} .. {spread[0][1]:.1e}, residual {spread[1][0]:.1e} .. {spread[1][1]:.1e}; leave-one-out x {worst[0]:.2f}, "
          f"residual {worst[1]:.2f}")
    return worst


@pytest.mark.parametrize("name", SMALL + MID)
@pytest.mark.parametrize("m", gr.RESTARTS)
@pytest.mark.parametrize("precond", PRECONDS)
@pytest.mark.parametrize("zero_start", (False, True))
def test_every_twin_lies_inside_the_gate_of_the_other_five(envelopes, name, m, precond, zero_start):
    n, ent, b, x0, ks = gr.problem(name)
    _skip_unless_available(n)
    assert np.all(x0 != 0) and (ks == gr.KS or n <= 3)
    env = envelopes(name, m, precond, zero_start)
    # the drop rule: nothing goes on these problems, from either start (the cap of two is asserted by Envelope besides)
    assert env.dropped == () and env.ks == ks, (name, m, precond, zero_start, env.dropped)
    assert all(env.resid_hist[j] > gr.DROP_BELOW for j in range(env.ks[-1])) or n <= 3
    for k in env.ks:
        assert len(env.twin_dev[k]) == len(gr.DOT_ORDERS) * len(gr.ROW_ORDERS)
    worst = _leave_one_out(env, f"{name} m={m} {precond} {'x0=0' if zero_start else 'random start'}")
    assert worst[0] <= gr.F and worst[1] <= gr.F, (name, m, precond, worst)
    assert worst[0] <= gr.OBSERVED_LEAVE_ONE_OUT["x"] * 2 and worst[1] <= gr.OBSERVED_LEAVE_ONE_OUT["residual"] * 2, "the recorded figures moved"


@pytest.mark.parametrize("m", sorted(gr.WIDE_KS))
def test_the_wide_basis_twins_lie_inside_the_gate_of_the_other_five(envelopes, m):
    n = gr.problem(gr.WIDE)[0]
    _skip_unless_available(n)
    env = envelopes(gr.WIDE, m, None)
    assert env.dropped == () and env.ks == gr.WIDE_KS[m]
    assert min(env.resid_hist) >= 0.11, "the wide basis converged: a full basis of 64 vectors no longer fills far from the floor"
    worst = _leave_one_out(env, f"{gr.WIDE} m={m}")
    assert worst[0] <= gr.F and worst[1] <= gr.F, (m, worst)


FIRST_SEEN_BY = 5


@pytest.mark.parametrize("mutate", gr.MUTATIONS)
def test_the_gate_is_below_what_a_wrong_recurrence_does(envelopes, mutate):
    """the mutation check, on r33: each mutation leaves the gate at some asked k <= 5 (a restart that keeps v_m: under m = 4, where
    k = 5 is the first iterate behind a restart)"""
    name = "r33"
    n, ent, b, x0, ks = gr.problem(name)
    _skip_unless_available(n)
    Op = gr.Operator(ent, (n, n), "f64")
    for m in gr.RESTARTS:
        if mutate == "keep_vm" and m > FIRST_SEEN_BY:
            continue  # (no restart within the k asked for)
        for precond in PRECONDS:
            if mutate in ("left", "no_minv") and precond is None:
                continue  # (no M to misplace)
            env = envelopes(name, m, precond)
            out, _ = gr.run_gmres(Op, b, x0, env.ks, m, precond, mutate=mutate)
            ratio = {k: env.x_dev(k, out[k][0]) / env.gate(k) for k in env.ks}
            seen = [k for k in env.ks if ratio[k] > 1]
            print(f"mutation {mutate:8s} on {name} m={m} {precond}: first seen at k = {seen[0] if seen else None}, deviation / gate there "
                  f"{ratio[seen[0]] if seen else 0:.1e}")
            assert seen and seen[0] <= FIRST_SEEN_BY, (mutate, m, precond, ratio)
            assert ratio[seen[0]] > 1000, (mutate, m, precond, ratio)


def test_the_special_cases_of_the_contract():
    """the identity from x0 = 0 lands in one iteration (h_1 is rounding noise or 0: nothing is divided by it); the quarter-turn
    rotation, on which BiCGSTAB breaks down, is solved by GMRES in two iterations and stagnates under GMRES(1) without an error"""
    n = 5
    ent = (np.arange(n), np.arange(n), np.ones(n))
    b = np.array([0.5, -1.25, 2.0, 0.75, -3.0])
    for kind in ("f64", gr._hp_kind(n)):
        out, hist = gr.run_gmres(gr.Operator(ent, (n, n), kind), b, np.zeros(n), (1,), 30)
        assert np.max(np.abs(np.asarray(out[1][0], dtype=np.float64) - b)) <= 4e-16 * 3.0 and out[1][1] <= 1e-15 and hist[0] == 1.0
    rot = (np.array([0, 1]), np.array([1, 0]), np.array([1.0, -1.0]))
    rb = np.array([1.0, 2.0])
    out, hist = gr.run_gmres(gr.Operator(rot, (2, 2), "f64"), rb, np.zeros(2), (1, 2), 30)
    assert np.allclose(out[2][0], [-2.0, 1.0], rtol=0, atol=1e-15) and hist[1] == 1.0 and hist[2] <= 1e-15
    out, hist = gr.run_gmres(gr.Operator(rot, (2, 2), "f64"), rb, np.zeros(2), (6,), 1)
    assert np.array_equal(out[6][0], np.zeros(2)) and hist == [1.0] * 7


def test_the_mpmath_fallback_is_the_same_reference():
    pytest.importorskip("mpmath")
    n, ent, b, x0, ks = gr.problem("n3")
    for precond in PRECONDS:
        mp = gr.gmres_reference(ent, n, b, x0, ks, 4, precond, force_mp=True)
        if gr._hp_kind(3) == "ld":
            ld = gr.gmres_reference(ent, n, b, x0, ks, 4, precond)
            for k in ks:
                assert max(abs(float(p) - float(l)) for p, l in zip(mp[k][0], ld[k][0])) <= 1e-15
                assert abs(mp[k][1] - ld[k][1]) <= 1e-15


# ---- the preconditioners applied by launches (tests/precond_ops.py): FSAI, ILU(0), Chebyshev as operators in every arithmetic -------
# Observed here (the tests print them): leave-one-out worst over precond_ops.GMRES_CASES but big, m = 4 and m = 30, both starts: see
# gmres_ref.OBSERVED_LEAVE_ONE_OUT_LAUNCHED.  Dropped: band4099 under ILU(0) loses k = 13 (3.5e-11 at k = 12 from the random start)
# and nothing else; n2 and n3 under ILU(0), an exact factorisation of a dense matrix, end at k = 1 and keep that k alone.
LAUNCHED = [(name, spec) for name, spec in po.GMRES_CASES if name != "big"]  # (big: a million rows in np.longdouble, the GPU file's)


@pytest.fixture(scope="module")
def launched():
    cache = {}

    def get(name, spec, m, zero_start=False):
        key = (name, spec, m, zero_start)
        if key not in cache:
            n, ent, b, x0, ks = po.nonsym_problem(name)
            op = cache.setdefault((name, spec), po.build(spec, n, ent))
            cache[key] = gr.Envelope(ent, n, b, np.zeros_like(x0) if zero_start else x0, ks, m, op)
        return cache[key], cache[name, spec]

    return get


@pytest.mark.parametrize("name,spec", LAUNCHED, ids=lambda v: v if isinstance(v, str) else v.kind)
@pytest.mark.parametrize("m", gr.RESTARTS)
@pytest.mark.parametrize("zero_start", (False, True))
def test_every_twin_lies_inside_the_gate_of_the_other_five_under_a_launched_preconditioner(launched, name, spec, m, zero_start):
    n, ent, b, x0, ks = po.nonsym_problem(name)
    _skip_unless_available(n)
    env, op = launched(name, spec, m, zero_start)
    assert len(env.dropped) <= (gr.MAX_DROPPED if n > 3 else n - 1) and env.ks == ks[: len(env.ks)] and env.ks, (name, spec, m, env.dropped)
    for k in env.ks:
        assert len(env.twin_dev[k]) == len(gr.DOT_ORDERS) * len(gr.ROW_ORDERS)
    worst = _leave_one_out(env, f"{po.label(name, spec)} m={m} {'x0=0' if zero_start else 'random start'}")
    # the reference's x at the largest kept k has the residual its recurrence reports
    k = env.ks[-1]
    kind = gr._hp_kind(n)
    bb = gr._conv(b, kind)
    r = bb - gr.Operator(ent, (n, n), kind).mv(env.ref_x[k])
    true = float(gr._sqrt(gr._dot(r, r) / gr._dot(bb, bb), kind))
    print(f"    true residual at k = {k} {true:.3e}, reported {env.ref_resid[k]:.3e}")
    assert worst[0] <= gr.F and worst[1] <= gr.F, (name, spec, m, worst)
    assert worst[0] <= gr.OBSERVED_LEAVE_ONE_OUT_LAUNCHED["x"] * 2 and worst[1] <= gr.OBSERVED_LEAVE_ONE_OUT_LAUNCHED["residual"] * 2, "the recorded figures moved"
    assert abs(true - env.ref_resid[k]) <= 1e-12 * max(env.resid_hist[0], 1.0), (name, spec, m, k, true, env.ref_resid[k])


LAUNCHED_MUTATION_CASES = [(po.LAP, po.FSAI2), (po.LAP, po.CHEB4), (po.CONV, po.ILU0)]


@pytest.mark.parametrize("name,spec", LAUNCHED_MUTATION_CASES, ids=lambda v: v if isinstance(v, str) else v.kind)
@pytest.mark.parametrize("mutate", gr.LAUNCHED_MUTATIONS)
def test_the_gate_is_below_what_a_wrong_launch_sequence_does(launched, name, spec, mutate):
    """z = M^-1 v_j not refreshed, x += V y without M^-1, an element of x left out, under each operator: outside the gate at some kept
    k <= 5, by a factor above 1000, with and without restarts inside the run"""
    n, ent, b, x0, ks = po.nonsym_problem(name)
    _skip_unless_available(n)
    for m in gr.RESTARTS:
        env, op = launched(name, spec, m)
        out, _ = gr.run_gmres(gr.Operator(ent, (n, n), "f64"), b, x0, env.ks, m, op, mutate=mutate)
        ratio = {k: env.x_dev(k, out[k][0]) / env.gate(k) for k in env.ks}
        seen = [k for k in env.ks if ratio[k] > 1]
        print(f"mutation {mutate:8s} on {po.label(name, spec)} m={m}: first seen at k = {seen[0] if seen else None}, deviation / gate there "
              f"{ratio[seen[0]] if seen else 0:.1e}")
        assert seen and seen[0] <= FIRST_SEEN_BY, (mutate, m, ratio)
        assert ratio[seen[0]] > 1000, (mutate, m, ratio)
