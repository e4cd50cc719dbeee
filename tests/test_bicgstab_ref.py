"""The references of tests/bicgstab_ref.py, checked on the CPU (no GPU): the extended-precision recurrence ends at the solution
numpy finds, every float64 twin lies inside the gate built from the other five, the drop rule at the noise floor takes no more than
its cap, and each wrong recurrence - beta without alpha / omega, omega over s.s, a stale p, an element of x left out, the
preconditioner on the other side - is outside the gate within five iterations.
"""
import numpy as np
import pytest

import bicgstab_ref as br
import precond_ops as po

SMALL = ("n1", "n2", "n3")
MID = ("r33", "r4097", "band4099")
PRECONDS = (None, "jacobi")


def _skip_unless_available(n):
    why = br.available(n)
    if why:
        pytest.skip(why)


@pytest.fixture(scope="module")
def envelopes():
    cache = {}

    def get(name, precond, zero_start=False):
        key = (name, precond, zero_start)
        if key not in cache:
            n, ent, b, x0, ks = br.problem(name)
            cache[key] = br.Envelope(ent, n, b, np.zeros_like(x0) if zero_start else x0, ks, precond)
        return cache[key]

    return get


@pytest.mark.parametrize("precond", PRECONDS)
def test_the_reference_ends_at_the_solution(precond):
    n, ent, b, x0, ks = br.problem("n3")
    dense = np.zeros((n, n))
    np.add.at(dense, (ent[0], ent[1]), ent[2])
    assert not np.array_equal(dense, dense.T) and ks == (1, 2, 3)
    want = np.linalg.solve(dense, b)
    x, res = br.bicgstab_reference(ent, n, b, x0, (3,), precond)[3]
    assert np.max(np.abs(np.asarray(x, dtype=np.float64) - want)) <= 1e-12 * np.max(np.abs(want))
    assert res <= 1e-12


@pytest.mark.parametrize("name", SMALL + MID)
@pytest.mark.parametrize("precond", PRECONDS)
@pytest.mark.parametrize("zero_start", (False, True))
def test_every_twin_lies_inside_the_gate_of_the_other_five(envelopes, name, precond, zero_start):
    n, ent, b, x0, ks = br.problem(name)
    _skip_unless_available(n)
    assert np.all(x0 != 0) and (ks == br.KS or n <= 3)
    env = envelopes(name, precond, zero_start)
    # the drop rule's cap (Envelope asserts it too): at most two of the eight k go to the noise floor, and only from the end
    assert len(env.dropped) <= (br.MAX_DROPPED if n > 3 else 0) and env.ks == ks[: len(env.ks)], (name, precond, env.dropped)
    assert all(env.resid_hist[k - 1] > br.DROP_BELOW for k in env.ks)
    for k in env.ks:
        assert len(env.twin_dev[k]) == len(br.DOT_ORDERS) * len(br.ROW_ORDERS)
    worst = [max(env.leave_one_out(k, what) for k in env.ks) for what in (0, 1)]
    spread = [(min(env.envelope(k, what) for k in env.ks), max(env.envelope(k, what) for k in env.ks)) for what in (0, 1)]
    print(f"{name} {precond} {'x0=0' if zero_start else 'random start'}: kept {env.ks}, dropped {env.dropped}, ||r|| / ||b|| before the last "
          f"k {env.resid_hist[env.ks[-1] - 1]:.2e}; twin envelope x {spread[0][0]:.1e} .. {spread[0][1]:.1e}, residual {spread[1][0]:.1e} .. "
          f"{spread[1][1]:.1e}; leave-one-out x {worst[0]:.2f}, residual {worst[1]:.2f}")
    assert worst[0] <= br.F and worst[1] <= br.F, (name, precond, worst)


def test_the_drop_rule_is_the_one_the_module_states():
    """what was observed when the problems were chosen: plain nothing goes; under Jacobi r33 and r4097 lose k = 13 alone"""
    for name in MID:
        n, ent, b, x0, ks = br.problem(name)
        _skip_unless_available(n)
        for precond in PRECONDS:
            _, hist = br.run_bicgstab(br.Operator(ent, (n, n), br._hp_kind(n)), b, x0, ks, precond)
            left = br.kept(ks, hist)
            assert left == (ks[:-1] if precond and name != "band4099" else ks), (name, precond, left, hist[12])
    assert br.kept((1, 2, 3), [1.0, 1e-14, 1.0, 1.0]) == (1,), "a k behind a quiet iteration goes too"


FIRST_SEEN_BY = 5


@pytest.mark.parametrize("mutate", br.MUTATIONS)
def test_the_gate_is_below_what_a_wrong_recurrence_does(envelopes, mutate):
    """the mutation check, on r33: each mutation leaves the gate at some k <= 5"""
    name = "r33"
    n, ent, b, x0, ks = br.problem(name)
    _skip_unless_available(n)
    Op = br.Operator(ent, (n, n), "f64")
    for precond in PRECONDS:
        if mutate == "left" and precond is None:
            continue  # (no side to change)
        env = envelopes(name, precond)
        out, _ = br.run_bicgstab(Op, b, x0, env.ks, precond, mutate=mutate)
        ratio = {k: env.x_dev(k, out[k][0]) / env.gate(k) for k in env.ks}
        seen = [k for k in env.ks if ratio[k] > 1]
        print(f"mutation {mutate:8s} on {name} {precond}: first seen at k = {seen[0] if seen else None}, deviation / gate there "
              f"{ratio[seen[0]] if seen else 0:.1e}")
        assert seen and seen[0] <= FIRST_SEEN_BY, (mutate, precond, ratio)
        assert ratio[seen[0]] > 1000, (mutate, precond, ratio)


def test_the_half_step_that_lands_is_taken_whole():
    """t.t = 0: the identity from x0 = 0 ends in one iteration with omega = 0, x = b and r = 0 exactly, in every arithmetic"""
    n = 5
    ent = (np.arange(n), np.arange(n), np.ones(n))
    b = np.array([0.5, -1.25, 2.0, 0.75, -3.0])
    for kind in ("f64", br._hp_kind(n)):
        out, hist = br.run_bicgstab(br.Operator(ent, (n, n), kind), b, np.zeros(n), (1,))
        assert np.array_equal(np.asarray(out[1][0], dtype=np.float64), b) and out[1][1] == 0.0 and hist == [1.0, 0.0]


def test_the_mpmath_fallback_is_the_same_reference():
    pytest.importorskip("mpmath")
    n, ent, b, x0, ks = br.problem("n3")
    for precond in PRECONDS:
        mp = br.bicgstab_reference(ent, n, b, x0, ks, precond, force_mp=True)
        if br._hp_kind(3) == "ld":
            ld = br.bicgstab_reference(ent, n, b, x0, ks, precond)
            for k in ks:
                assert max(abs(float(p) - float(l)) for p, l in zip(mp[k][0], ld[k][0])) <= 1e-15
                assert abs(mp[k][1] - ld[k][1]) <= 1e-15


# ---- the preconditioners applied by launches (tests/precond_ops.py): FSAI, ILU(0), Chebyshev as operators in every arithmetic -------
LAUNCHED = [(name, spec) for name, spec in po.BICGSTAB_CASES if name != "big"]  # (big: a million rows in np.longdouble, the GPU file's)


@pytest.fixture(scope="module")
def launched():
    cache = {}

    def get(name, spec, zero_start=False):
        key = (name, spec, zero_start)
        if key not in cache:
            n, ent, b, x0, ks = po.nonsym_problem(name)
            op = cache.setdefault((name, spec), po.build(spec, n, ent))
            cache[key] = br.Envelope(ent, n, b, np.zeros_like(x0) if zero_start else x0, ks, op)
        return cache[key], cache[name, spec]

    return get


@pytest.mark.parametrize("name,spec", LAUNCHED, ids=lambda v: v if isinstance(v, str) else v.kind)
@pytest.mark.parametrize("zero_start", (False, True))
def test_every_twin_lies_inside_the_gate_of_the_other_five_under_a_launched_preconditioner(launched, name, spec, zero_start):
    n, ent, b, x0, ks = po.nonsym_problem(name)
    _skip_unless_available(n)
    env, op = launched(name, spec, zero_start)
    assert len(env.dropped) <= (br.MAX_DROPPED if n > 3 else n - 1) and env.ks == ks[: len(env.ks)] and env.ks, (name, spec, env.dropped)
    for k in env.ks:
        assert len(env.twin_dev[k]) == len(br.DOT_ORDERS) * len(br.ROW_ORDERS)
    worst = [max(env.leave_one_out(k, what) for k in env.ks) for what in (0, 1)]
    spread = [(min(env.envelope(k, what) for k in env.ks), max(env.envelope(k, what) for k in env.ks)) for what in (0, 1)]
    # the reference's x at the largest kept k has the residual its recurrence reports
    k = env.ks[-1]
    kind = br._hp_kind(n)
    Op = br.Operator(ent, (n, n), kind)
    r = br._conv(b, kind) - Op.mv(env.ref_x[k])
    true = float(br._sqrt(br._dot(r, r) / br._dot(br._conv(b, kind), br._conv(b, kind)), kind))
    print(f"{po.label(name, spec)} {'x0=0' if zero_start else 'random start'}: kept {env.ks}, dropped {env.dropped}, ||r|| / ||b|| before the last "
          f"k {env.resid_hist[k - 1]:.2e}; twin envelope x {spread[0][0]:.1e} .. {spread[0][1]:.1e}, residual {spread[1][0]:.1e} .. "
          f"{spread[1][1]:.1e}; leave-one-out x {worst[0]:.2f}, residual {worst[1]:.2f}; true residual at k = {k} {true:.3e}, reported {env.ref_resid[k]:.3e}")
    assert worst[0] <= br.F and worst[1] <= br.F, (name, spec, worst)
    assert worst[0] <= br.OBSERVED_LEAVE_ONE_OUT_LAUNCHED["x"] * 2 and worst[1] <= br.OBSERVED_LEAVE_ONE_OUT_LAUNCHED["residual"] * 2, "the recorded figures moved"
    assert abs(true - env.ref_resid[k]) <= 1e-12 * max(env.resid_hist[0], 1.0), (name, spec, k, true, env.ref_resid[k])


LAUNCHED_MUTATION_CASES = [(po.LAP, po.FSAI2), (po.LAP, po.CHEB4), (po.CONV, po.ILU0)]


@pytest.mark.parametrize("name,spec", LAUNCHED_MUTATION_CASES, ids=lambda v: v if isinstance(v, str) else v.kind)
@pytest.mark.parametrize("mutate", br.LAUNCHED_MUTATIONS)
def test_the_gate_is_below_what_a_wrong_launch_sequence_does(launched, name, spec, mutate):
    """the mutations that need a phat and shat of their own: each leaves the gate at some kept k <= 5, by a factor above 1000"""
    n, ent, b, x0, ks = po.nonsym_problem(name)
    _skip_unless_available(n)
    env, op = launched(name, spec)
    out, _ = br.run_bicgstab(br.Operator(ent, (n, n), "f64"), b, x0, env.ks, op, mutate=mutate)
    ratio = {k: env.x_dev(k, out[k][0]) / env.gate(k) for k in env.ks}
    seen = [k for k in env.ks if ratio[k] > 1]
    print(f"mutation {mutate:10s} on {po.label(name, spec)}: first seen at k = {seen[0] if seen else None}, deviation / gate there "
          f"{ratio[seen[0]] if seen else 0:.1e}")
    assert seen and seen[0] <= FIRST_SEEN_BY, (mutate, ratio)
    assert ratio[seen[0]] > 1000, (mutate, ratio)
