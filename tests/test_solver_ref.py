"""The references of tests/solver_ref.py, checked on the CPU (no GPU): the two arrangements of the recurrence agree in extended
precision, the reference solves systems whose solution is known, the gate is ten decades below what a wrong beta, a stale ring
slot or an element of x left out does to an iterate, and the problems of tests/test_gpu_solver_steps.py are still far from the
noise floor at the last iterate checked.
"""
import numpy as np
import pytest

import solver_ref as sr

MID = ("lap33", "rand4097")


def _red_black(m):
    colour = (np.add.outer(np.arange(m), np.arange(m)) % 2).ravel()
    return np.argsort(colour, kind="stable"), colour


def _preconds(name, n):
    out = [("plain", None), ("jacobi", "jacobi"), ("symgs rows", ("symgs", np.arange(n)))]
    if name == "lap33":
        order, colour = _red_black(33)
        out.append(("symgs colours", ("symgs", order, colour)))
    return out


@pytest.fixture(scope="module")
def envelopes():
    cache = {}

    def get(name, label, precond):
        if (name, label) not in cache:
            n, ent, b, x0, ks = sr.problem(name)
            cache[name, label] = sr.Envelope(ent, b, x0, ks, precond)
        return cache[name, label]

    return get


def test_the_reference_arithmetic_is_extended_or_says_why_not():
    if sr.EXTENDED:
        assert np.finfo(np.longdouble).eps <= 2.0**-63 and sr.available(10**7) is None
    else:
        assert sr.available(sr.MP_MAX_N) is None and "mpmath" in sr.available(sr.MP_MAX_N + 1)
    assert sr.available(100, force_mp=True) is None and "n = 5001" in sr.available(5001, force_mp=True)


@pytest.mark.parametrize("name", ("n2", "n3") + MID)
def test_the_two_arrangements_agree_in_extended_precision(name):
    n, ent, b, x0, ks = sr.problem(name)
    if sr.available(n):
        pytest.skip(sr.available(n))
    for label, precond in _preconds(name, n):
        a = sr.cg_reference(ent, b, x0, (0,) + ks, precond)
        c = sr.cg_reference(ent, b, x0, (0,) + ks, precond, arrangement="chronopoulos-gear")
        worst = max(float(np.max(np.abs(a[k][0] - c[k][0])) / np.max(np.abs(a[k][0]))) for k in ks)
        print(f"{name} {label}: textbook vs Chronopoulos-Gear in extended precision, largest deviation {worst:.2e}")
        assert worst <= 1e-17, (name, label, worst)
        # the recurrence residual: its rounding error is absolute, on the scale of the largest residual so far
        assert all(abs(a[k][1] - c[k][1]) <= 1e-17 * max(a[j][1] for j in (0,) + ks if j <= k) for k in ks), (name, label)


def test_the_vectorised_colour_sweep_is_the_sequential_sweep_in_that_order():
    n, ent, b, x0, ks = sr.problem("lap33")
    order, colour = _red_black(33)
    a = sr.cg_reference(ent, b, x0, ks, ("symgs", order))
    c = sr.cg_reference(ent, b, x0, ks, ("symgs", order, colour))
    assert max(float(np.max(np.abs(a[k][0] - c[k][0]))) for k in ks) <= 1e-17
    with pytest.raises(ValueError, match="proper colouring"):
        sr.System(ent, n, "f64", ("symgs", np.arange(n), np.zeros(n, int)))  # one class holding coupled rows
    with pytest.raises(ValueError, match="permutation"):
        sr.System(ent, n, "f64", ("symgs", np.zeros(n, int)))


def test_the_reference_solves_systems_with_a_known_solution():
    # n = 3: conjugate gradients ends at iteration 3, whatever the start
    n, ent, b, x0, ks = sr.problem("n3")
    dense = np.zeros((3, 3))
    np.add.at(dense, (ent[0], ent[1]), ent[2])
    want = np.linalg.solve(dense.astype(np.float64), b)
    got = sr.cg_reference(ent, b, x0, (3,))[3]
    assert np.max(np.abs(np.asarray(got[0], dtype=np.float64) - want)) <= 4e-16 and got[1] <= 1e-17
    # the 4097-row system (its diagonal stored twice, columns unsorted): b := A x* in extended precision, then every
    # preconditioner finds x* again
    n, ent, _, x0, _ = sr.problem("rand4097")
    if sr.available(n):
        pytest.skip(sr.available(n))
    S = sr.System(ent, n, "ld" if sr.EXTENDED else "mp")
    xs = np.random.default_rng(3).uniform(-1, 1, n)
    bs = S.mv(sr._conv(xs, S.kind))
    for label, precond, k in (("plain", None, 400), ("jacobi", "jacobi", 300)):
        x, res = sr.cg_reference(ent, bs, x0, (k,), precond)[k]
        err = float(np.max(np.abs(x - sr._conv(xs, S.kind))))
        assert err <= 1e-16 and res <= 1e-16, (label, err, res)
    # duplicates are summed: the diagonal arrives as 3/4 + 1/4 of itself
    row, col, val = ent
    d = np.zeros(n)
    np.add.at(d, row[row == col], val[row == col])
    assert np.array_equal(S.diag.astype(np.float64), d) and np.all(np.bincount(row[row == col]) == 2)
    rp = np.searchsorted(row, np.arange(n + 1))
    assert any(np.any(np.diff(col[rp[i]:rp[i + 1]]) < 0) for i in range(50)), "columns are meant to be unsorted"


@pytest.mark.parametrize("name", MID)
def test_the_gate_is_far_below_what_a_wrong_recurrence_does(envelopes, name):
    """the mutation check: beta = 0 at every fourth iteration (the captured graph that restarted), beta from a slot four
    iterations old, the last element of x never updated - each at least 100 gates away at some k of the list"""
    n, ent, b, x0, ks = sr.problem(name)
    if sr.available(n):
        pytest.skip(sr.available(n))
    for label, precond in _preconds(name, n):
        env = envelopes(name, label, precond)
        S = sr.System(ent, n, "f64", precond)
        for mutate in ("restart", "stale", "tail"):
            out, _ = sr.run_textbook(S, b, x0, ks, mutate=mutate)
            ratio = {k: env.x_dev(k, out[k][0]) / env.gate(k) for k in ks}
            first = min(k for k in ks if ratio[k] > 1)
            print(f"mutation {mutate:8s} on {name} {label}: first seen at k = {first}, largest deviation / gate = {max(ratio.values()):.1e}")
            assert max(ratio.values()) >= 100, (name, label, mutate, ratio)
            if mutate == "tail":
                assert first == 1, ratio
            else:
                assert all(ratio[k] <= 1 for k in ks if k <= 4) and first in (5, 8), ratio  # the first wrong beta is beta_3 / beta_4


@pytest.mark.parametrize("name", sr.PROBLEMS[:5] + ("lap725",))
def test_the_twins_stay_close_and_the_last_iterate_is_above_the_noise_floor(envelopes, name):
    n, ent, b, x0, ks = sr.problem(name)
    if sr.available(n):
        pytest.skip(sr.available(n))
    assert np.all(x0 != 0) and ks == tuple(k for k in sr.KS if k <= n or n > 3)
    for label, precond in _preconds(name, n) if n < 10_000 else [("plain", None)]:
        env = envelopes(name, label, precond)
        worst = max(env.envelope(k) for k in ks)
        worst_r = max(env.envelope(k, 1) for k in ks)
        print(f"twins on {name} {label}: largest deviation of x_k {worst:.2e}, of ||r_k||/||b|| {worst_r:.2e}; residual at k = {ks[-1]}: {env.ref_resid[ks[-1]]:.2e}")
        # float64 over a dozen iterations of a well-conditioned recurrence: the sequential dot products of n terms lose ~sqrt(n) eps
        assert sr.FLOOR <= worst <= 64 * max(np.sqrt(n), 16) * 2.0**-52, (name, label, worst)
        if n > 3:
            assert env.ref_resid[ks[-1]] >= 1e-12, (name, label, env.ref_resid)  # four decades above eps: nothing is noise yet
            # the recurrence residual's rounding error is absolute, on the scale of the largest residual so far
            worst_abs = max(env.envelope(k, 1) * max(env.ref_resid[k], env.resid_hist[k - 1] / 4) / max(env.resid_hist[: k + 1]) for k in ks)
            assert worst_abs <= 64 * max(np.sqrt(n), 16) * 2.0**-52, (name, label, worst_abs)


def test_the_mpmath_fallback_is_the_same_reference():
    pytest.importorskip("mpmath")
    for name in ("n3", "lap7"):
        if name == "lap7":
            n, row, col, val = sr.laplacian_2d(7)
            rng = np.random.default_rng(5)
            ent, b, x0, ks = (row, col, val), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), (1, 4, 9)
        else:
            n, ent, b, x0, ks = sr.problem(name)
        for precond in (None, "jacobi", ("symgs", np.arange(n))):
            mp = sr.cg_reference(ent, b, x0, ks, precond, force_mp=True)
            env = sr.Envelope(ent, b, x0, ks, precond, force_mp=True)
            assert all(sr.FLOOR <= env.gate(k) / sr.F <= 1e-13 for k in ks)
            if sr.EXTENDED:
                ld = sr.cg_reference(ent, b, x0, ks, precond)
                import mpmath

                for k in ks:
                    hi = ld[k][0].astype(np.float64)  # an 80-bit number is the sum of two doubles
                    lo = (ld[k][0] - hi).astype(np.float64)
                    d = max(abs(float(p - (mpmath.mpf(float(h)) + mpmath.mpf(float(l))))) for p, h, l in zip(mp[k][0], hi, lo))
                    assert d <= 1e-17 and abs(mp[k][1] - ld[k][1]) <= 1e-17 * max(1.0, ld[k][1]), (name, precond, k, d)
