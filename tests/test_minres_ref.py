"""The references of tests/minres_ref.py, checked on the CPU (no GPU): the extended-precision recurrence ends at the solution numpy
finds on the small problems, phibar is the M^-1 norm of the true residual and never grows, every float64 twin lies inside the gate
built from the other five, the drop rule at the noise floor takes no more than its cap, and each wrong recurrence - the r1 term
dropped, a stale w1, dbar with the wrong sign, the shift ignored, beta from r2.r2 under a preconditioner, an element of x left out -
is outside the gate at some kept k of some problem.
"""
import numpy as np
import pytest

import minres_ref as mr
import precond_ops as po

SMALL = ("n1", "n2", "n3")
MID = ("r33", "r4097", "band4099", "saddle", "shifted")


def _preconds(name):
    """the preconditioners the twins can state: Jacobi where the diagonal of the preconditioner's matrix is positive"""
    return (None, "jacobi") if name in ("band4099", "saddle", "shifted") else (None,)


CASES = [(name, precond) for name in SMALL + MID for precond in _preconds(name)]


def _skip_unless_available(n):
    why = mr.available(n)
    if why:
        pytest.skip(why)


@pytest.fixture(scope="module")
def envelopes():
    cache = {}

    def get(name, precond, zero_start=False):
        key = (name, precond, zero_start)
        if key not in cache:
            p = mr.problem(name)
            cache[key] = mr.Envelope(p.entries, p.n, p.b, np.zeros_like(p.x0) if zero_start else p.x0, p.ks, p.shift, precond, p.p_entries)
        return cache[key]

    return get


def _dense(p):
    dense = np.zeros((p.n, p.n), dtype=np.longdouble)
    np.add.at(dense, (p.entries[0], p.entries[1]), p.entries[2].astype(np.longdouble))
    return dense


def test_every_problem_is_exactly_symmetric_and_indefinite():
    for name in SMALL + MID:
        p = mr.problem(name)
        row, col, val = p.entries
        fwd, bwd = {}, {}
        for i, j, v in zip(row.tolist(), col.tolist(), val.tolist()):
            fwd[i, j] = fwd.get((i, j), 0.0) + v
            bwd[j, i] = bwd.get((j, i), 0.0) + v
        assert fwd == bwd, name
        assert np.all(p.x0 != 0) and (p.ks == mr.KS or p.n <= 3)
    for name in ("n2", "n3", "r33"):
        p = mr.problem(name)
        lam = np.linalg.eigvalsh(_dense(p).astype(np.float64))
        assert lam[0] < 0 < lam[-1], (name, lam)
    assert mr.DENSE[1][0][0] < 0
    # shifted: the shift lies strictly inside the Laplacian's spectrum, between two of its eigenvalues
    lam, shift = mr.laplacian_eigenvalues(mr.SHIFTED_GRID), mr.problem("shifted").shift
    below = int(np.sum(lam < shift))
    assert 10 <= below <= 40 and np.min(np.abs(lam - shift)) > 1e-4, (below, np.min(np.abs(lam - shift)))


@pytest.mark.parametrize("name", SMALL + ("r33",))
def test_the_reference_ends_at_the_solution(name):
    """in longdouble: n iterations solve the small systems; r33 (rounding costs the Lanczos vectors their orthogonality, so n
    iterations do not end it) is there after 100"""
    p = mr.problem(name)
    _skip_unless_available(p.n)
    dense = _dense(p) - np.longdouble(p.shift) * np.eye(p.n, dtype=np.longdouble)
    want = np.linalg.solve(dense.astype(np.float64), p.b)
    k = p.n if p.n <= 3 else 100
    out, hist = mr.run_minres(mr.Operator(p.entries, (p.n, p.n), mr._hp_kind(p.n)), p.b, p.x0, (k,), p.shift)
    x = np.asarray(out[k][0], dtype=np.float64)
    assert np.max(np.abs(x - want)) <= 1e-12 * np.max(np.abs(want)), (name, np.max(np.abs(x - want)))
    assert hist[k] <= 1e-12


@pytest.mark.parametrize("name,precond", CASES, ids=lambda v: str(v))
def test_phibar_is_the_true_residual_and_never_grows(name, precond):
    p = mr.problem(name)
    _skip_unless_available(p.n)
    kind = mr._hp_kind(p.n)
    Op = mr.Operator(p.entries, (p.n, p.n), kind)
    Pop = mr.Operator(p.p_entries, (p.n, p.n), kind) if p.p_entries is not None else None
    out, hist = mr.run_minres(Op, p.b, p.x0, p.ks, p.shift, precond, Pop)
    assert all(hist[k + 1] <= hist[k] * (1 + 1e-15) for k in range(len(hist) - 1)), (name, precond, hist)
    dinv = mr.inverse_diagonal(Pop if Pop is not None else Op) if precond else 1
    b = mr._conv(p.b, kind)
    beta_b = np.sqrt(mr._dot(b, dinv * b))
    for k in p.ks:
        x = out[k][0]
        r = b - (Op.mv(x) - mr._conv(np.array([p.shift]), kind)[0] * x)
        true = float(np.sqrt(mr._dot(r, dinv * r)) / beta_b)
        assert abs(true - out[k][1]) <= 1e-12 * max(hist[0], 1.0), (name, precond, k, true, out[k][1])


@pytest.mark.parametrize("name,precond", CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("zero_start", (False, True))
def test_every_twin_lies_inside_the_gate_of_the_other_five(envelopes, name, precond, zero_start):
    p = mr.problem(name)
    _skip_unless_available(p.n)
    env = envelopes(name, precond, zero_start)
    # the drop rule's cap (Envelope asserts it too): at most two of the eight k go to the noise floor, and only from the end
    assert len(env.dropped) <= (mr.MAX_DROPPED if p.n > 3 else 0) and env.ks == p.ks[: len(env.ks)], (name, precond, env.dropped)
    assert all(env.resid_hist[k - 1] > mr.DROP_BELOW for k in env.ks)
    for k in env.ks:
        assert len(env.twin_dev[k]) == len(mr.DOT_ORDERS) * len(mr.ROW_ORDERS)
    worst = [max(env.leave_one_out(k, what) for k in env.ks) for what in (0, 1)]
    spread = [(min(env.envelope(k, what) for k in env.ks), max(env.envelope(k, what) for k in env.ks)) for what in (0, 1)]
    print(f"{name} {precond} {'x0=0' if zero_start else 'random start'}: kept {env.ks}, dropped {env.dropped}, phibar / beta_b before the last "
          f"k {env.resid_hist[env.ks[-1] - 1]:.2e}; twin envelope x {spread[0][0]:.1e} .. {spread[0][1]:.1e}, residual {spread[1][0]:.1e} .. "
          f"{spread[1][1]:.1e}; leave-one-out x {worst[0]:.2f}, residual {worst[1]:.2f}")
    assert worst[0] <= mr.F and worst[1] <= mr.F, (name, precond, worst)
    assert worst[0] <= mr.OBSERVED_LEAVE_ONE_OUT["x"] + 0.005 and worst[1] <= mr.OBSERVED_LEAVE_ONE_OUT["residual"] + 0.005, "the module's record is out of date"


def test_the_drop_rule_is_the_one_the_module_states():
    assert mr.kept((1, 2, 3), [1.0, 1e-14, 1.0, 1.0]) == (1,), "a k behind a quiet iteration goes too"
    assert mr.kept((1, 2, 3), [1.0, 1.0, 1e-14, 1.0]) == (1, 2)
    assert mr.DROP_BELOW == 1e-13 and mr.MAX_DROPPED == 2 and mr.KS == (1, 2, 3, 4, 5, 8, 9, 13)


# where each mutation must show: a problem with the ingredient it spoils
MUTATION_CASES = {"r1_term": ("r33", None), "stale_w1": ("r33", None), "dbar_sign": ("r33", None), "no_shift": ("shifted", None),
                  "beta_rr": ("saddle", "jacobi"), "tail": ("r33", None)}


@pytest.mark.parametrize("mutate", mr.MUTATIONS)
def test_the_gate_is_below_what_a_wrong_recurrence_does(envelopes, mutate):
    """the mutation check: each mutation leaves the gate at some kept k, by a factor above 1000"""
    name, precond = MUTATION_CASES[mutate]
    p = mr.problem(name)
    _skip_unless_available(p.n)
    env = envelopes(name, precond)
    Pop = mr.Operator(p.p_entries, (p.n, p.n), "f64") if p.p_entries is not None else None
    out, _ = mr.run_minres(mr.Operator(p.entries, (p.n, p.n), "f64"), p.b, p.x0, env.ks, p.shift, precond, Pop, mutate=mutate)
    ratio = {k: env.x_dev(k, out[k][0]) / env.gate(k) for k in env.ks}
    seen = [k for k in env.ks if ratio[k] > 1]
    print(f"mutation {mutate:9s} on {name} {precond}: first seen at k = {seen[0] if seen else None}, deviation / gate there "
          f"{ratio[seen[0]] if seen else 0:.1e}")
    assert seen and ratio[seen[0]] > 1000, (mutate, ratio)


def test_an_exhausted_krylov_space_ends_the_run_with_the_exact_iterate():
    """diag(2, 2, -1, -1) has two eigenvalues, so the second iteration lands: beta is what rounding leaves of 0 and phibar falls
    below the engine's floor.  The swap from x0 = 0 with b = (2, 0) lands exactly - v_1 = e_1, v_2 = e_2, beta = 0 - in every
    arithmetic, and the iterates behind it are the one that stands"""
    n = 4
    ent = (np.arange(n), np.arange(n), np.array([2.0, 2.0, -1.0, -1.0]))
    b = np.array([0.5, -1.25, 2.0, 0.75])
    p = mr.problem("n2")
    for kind in ("f64", mr._hp_kind(n)):
        out, hist = mr.run_minres(mr.Operator(ent, (n, n), kind), b, np.zeros(n), (2,))
        x = np.asarray(out[2][0], dtype=np.float64)
        assert np.max(np.abs(x - b / ent[2])) <= 2e-15 and hist[2] <= 1e-15 and hist[1] > 0.1, (kind, x, hist)
        out, hist = mr.run_minres(mr.Operator(p.entries, (2, 2), kind), np.array([2.0, 0.0]), np.zeros(2), (1, 2, 5))
        assert hist == [1.0, 1.0, 0.0, 0.0, 0.0, 0.0], hist
        assert all(np.array_equal(np.asarray(out[k][0], dtype=np.float64), np.array([0.0, 2.0])) for k in (2, 5)), out
        assert not np.asarray(out[1][0], dtype=np.float64).any()


def test_the_mpmath_fallback_is_the_same_reference():
    pytest.importorskip("mpmath")
    p = mr.problem("n3")
    kinds = ["mp"] + (["ld"] if mr._hp_kind(3) == "ld" else [])
    runs = {kind: mr.run_minres(mr.Operator(p.entries, (3, 3), kind), p.b, p.x0, p.ks, p.shift)[0] for kind in kinds}
    if len(kinds) == 2:
        for k in p.ks:
            assert max(abs(float(a) - float(c)) for a, c in zip(runs["mp"][k][0], runs["ld"][k][0])) <= 1e-15 * max(1.0, float(np.max(np.abs(runs["ld"][k][0]))))
            assert abs(runs["mp"][k][1] - runs["ld"][k][1]) <= 1e-15


# ---- the preconditioners applied by launches (tests/precond_ops.py): FSAI and Chebyshev of a separate positive definite P ----------
LAUNCHED = [(name, spec) for name, spec in po.SYM_CASES if name != "big"]  # (big: a million rows in np.longdouble, the GPU file's)


@pytest.fixture(scope="module")
def launched():
    cache = {}

    def get(name, spec, zero_start=False):
        key = (name, spec, zero_start)
        if key not in cache:
            p = po.sym_problem(name)
            op = cache.setdefault((name, spec), po.build(spec, p.n, p.p_entries))
            cache[key] = mr.Envelope(p.entries, p.n, p.b, np.zeros_like(p.x0) if zero_start else p.x0, p.ks, p.shift, op)
        return cache[key], cache[name, spec]

    return get


@pytest.mark.parametrize("name,spec", LAUNCHED, ids=lambda v: v if isinstance(v, str) else v.kind)
@pytest.mark.parametrize("zero_start", (False, True))
def test_every_twin_lies_inside_the_gate_of_the_other_five_under_a_launched_preconditioner(launched, name, spec, zero_start):
    p = po.sym_problem(name)
    _skip_unless_available(p.n)
    env, op = launched(name, spec, zero_start)
    assert len(env.dropped) <= (mr.MAX_DROPPED if p.n > 3 else 0) and env.ks == p.ks[: len(env.ks)] and env.ks, (name, spec, env.dropped)
    for k in env.ks:
        assert len(env.twin_dev[k]) == len(mr.DOT_ORDERS) * len(mr.ROW_ORDERS)
    worst = [max(env.leave_one_out(k, what) for k in env.ks) for what in (0, 1)]
    spread = [(min(env.envelope(k, what) for k in env.ks), max(env.envelope(k, what) for k in env.ks)) for what in (0, 1)]
    # the reference's x at the largest kept k has the residual its recurrence reports: phibar is the M^-1 norm of the true residual
    k = env.ks[-1]
    kind = mr._hp_kind(p.n)
    b = mr._conv(p.b, kind)
    r = b - (mr.Operator(p.entries, (p.n, p.n), kind).mv(env.ref_x[k]) - mr._conv(np.array([p.shift]), kind)[0] * env.ref_x[k])
    true = float(mr._sqrt(mr._dot(r, op.apply(r, kind)) / mr._dot(b, op.apply(b, kind)), kind))
    print(f"{po.label(name, spec)} {'x0=0' if zero_start else 'random start'}: kept {env.ks}, dropped {env.dropped}, phibar / beta_b before the last "
          f"k {env.resid_hist[k - 1]:.2e}; twin envelope x {spread[0][0]:.1e} .. {spread[0][1]:.1e}, residual {spread[1][0]:.1e} .. "
          f"{spread[1][1]:.1e}; leave-one-out x {worst[0]:.2f}, residual {worst[1]:.2f}; true residual at k = {k} {true:.3e}, reported {env.ref_resid[k]:.3e}")
    assert worst[0] <= mr.F and worst[1] <= mr.F, (name, spec, worst)
    assert worst[0] <= mr.OBSERVED_LEAVE_ONE_OUT_LAUNCHED["x"] * 2 and worst[1] <= mr.OBSERVED_LEAVE_ONE_OUT_LAUNCHED["residual"] * 2, "the recorded figures moved"
    assert abs(true - env.ref_resid[k]) <= 1e-12 * max(env.resid_hist[0], 1.0), (name, spec, k, true, env.ref_resid[k])


LAUNCHED_MUTATION_CASES = [("shifted", po.FSAI2), ("saddle", po.CHEB4)]


@pytest.mark.parametrize("name,spec", LAUNCHED_MUTATION_CASES, ids=lambda v: v if isinstance(v, str) else v.kind)
@pytest.mark.parametrize("mutate", mr.LAUNCHED_MUTATIONS)
def test_the_gate_is_below_what_a_wrong_launch_sequence_does(launched, name, spec, mutate):
    """the mutations that need a y of its own: each leaves a gate at some kept k by a factor above 1000 - x's, but for beta_b from b.b,
    which moves the returned residual alone"""
    p = po.sym_problem(name)
    _skip_unless_available(p.n)
    env, op = launched(name, spec)
    with np.errstate(invalid="ignore"):  # (a stale y makes r2.y negative in the end: the iterates behind it are NaN and count as unseen)
        out, _ = mr.run_minres(mr.Operator(p.entries, (p.n, p.n), "f64"), p.b, p.x0, env.ks, p.shift, op, mutate=mutate)
    if mutate == "beta_b_bb":
        assert all(env.x_dev(k, out[k][0]) <= env.gate(k) for k in env.ks), "beta_b does not enter x"
        ratio = {k: env.resid_dev(k, out[k][1]) / env.gate_resid(k) for k in env.ks}
    else:
        ratio = {k: env.x_dev(k, out[k][0]) / env.gate(k) for k in env.ks}
    seen = [k for k in env.ks if ratio[k] > 1]
    print(f"mutation {mutate:9s} on {po.label(name, spec)}: first seen at k = {seen[0] if seen else None}, deviation / gate there "
          f"{ratio[seen[0]] if seen else 0:.1e}")
    assert seen and ratio[seen[0]] > 1000, (mutate, ratio)
