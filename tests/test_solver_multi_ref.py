"""The k-column twin of tests/solver_multi_ref.py, checked on the CPU (no GPU): without a freeze it is
solver_ref.run_chronopoulos_gear column by column, bit for bit; a power-of-two multiple of a column is that column's iterates scaled,
bit for bit (which is why two Envelopes serve any k); the freeze rule and the b = 0 rule do what spmv_cg_multi's contract says; the
gate of tests/test_gpu_cg_multi.py (solver_ref.F twin envelopes per column) is exceeded by a column that uses its neighbour's alpha
or gamma_old, by a frozen column that is still updated and by a last row of X that is never updated; and MARGIN_REL_TOL leaves the
twin a factor 2 from the limit on both sides of the look that stops an ordinary column of the zero-and-solved-column test.
"""
import numpy as np
import pytest

import solver_multi_ref as mr
import solver_ref as sr

MID = ("lap33", "rand4097")


@pytest.mark.parametrize("precond", (None, "jacobi"))
def test_the_twin_is_the_single_column_recurrence_column_by_column(precond):
    n, ent, B, X0, ks = mr.columns("lap33", 3)
    S = sr.System(ent, n, "f64", precond)
    for order in sr.DOT_ORDERS:
        X, iters, res, kept = mr.run_multi(S, B, X0, max(ks), dot_order=order, keep=ks)
        assert np.all(iters == max(ks))
        for c in range(3):
            out, _ = sr.run_chronopoulos_gear(S, B[:, c].copy(), X0[:, c].copy(), ks, dot_order=order)
            for j in ks:
                assert np.array_equal(kept[j][:, c], out[j][0]), (precond, order, c, j)
            assert res[c] == out[max(ks)][1]


def test_a_power_of_two_multiple_of_a_column_is_that_column_scaled():
    n, ent, B, X0, ks = mr.columns("rand4097", 5)
    assert np.array_equal(B[:, 4], 4.0 * B[:, 0]) and np.array_equal(X0[:, 3], 2.0 * X0[:, 1])
    S = sr.System(ent, n, "f64", "jacobi")
    X, iters, res, _ = mr.run_multi(S, B, X0, 9)
    assert np.array_equal(X[:, 2], 2.0 * X[:, 0]) and np.array_equal(X[:, 4], 4.0 * X[:, 0]) and np.array_equal(X[:, 3], 2.0 * X[:, 1])
    assert res[2] == res[0] and res[3] == res[1]
    env = mr.envelopes("rand4097", "jacobi")
    assert mr.column_dev(env, 4, 9, X[:, 4]) == mr.column_dev(env, 0, 9, X[:, 0])
    assert mr.column_dev(env, 0, 9, X[:, 0], res[0])[0] <= env[0].gate(9) / sr.F  # the twin is one of the envelope's twins


@pytest.mark.parametrize("check_every,rel_tol", ((1, 1e-10), (5, 1e-10), (5, mr.MARGIN_REL_TOL)))
def test_the_freeze_rule_and_the_zero_column(check_every, rel_tol):
    n, ent, B, X0, kinds, _ = mr.special_columns()
    S = sr.System(ent, n, "f64")
    assert np.all(B[:, 1] == 0) and np.all(X0[:, 1] == 0)
    assert np.all(B[:, 2] - S.mv(X0[:, 2]) == 0), "r_0 of the solved column is exactly 0"
    X, iters, res, kept = mr.run_multi(S, B, X0, 1000, rel_tol, check_every)
    assert iters[1] == 0 and iters[2] == 0 and res[1] == 0 and res[2] == 0
    assert np.array_equal(X[:, 1], X0[:, 1]) and np.array_equal(X[:, 2], X0[:, 2]) and np.all(np.isfinite(X))
    bb = np.einsum("ic,ic->c", B, B)
    for c in (0, 3):
        assert 0 < iters[c] < 1000 and iters[c] % check_every == 0 and res[c] <= rel_tol
        true = np.linalg.norm(B[:, c] - S.mv(X[:, c])) / np.linalg.norm(B[:, c])
        assert true <= 4 * rel_tol, (c, true)
        # a frozen column keeps the iterate of the look that froze it
        Xs, its, _, _ = mr.run_multi(S, B, X0, int(iters[c]), 0.0, check_every)
        assert np.array_equal(Xs[:, c], X[:, c])
        under, over = mr.stopping_margin(kept, bb, c, rel_tol, check_every, int(iters[c]))
        print(f"lap33 special columns, check_every {check_every}, column {c}: stops at {iters[c]}; limit / resid there {under:.2f}, resid at the look before / limit {over:.2f}")
        if rel_tol == mr.MARGIN_REL_TOL:
            assert under >= 2 and over >= 2, "MARGIN_REL_TOL leaves no factor 2 to the limit: the GPU's look may differ from the twin's"


def test_the_eigenvector_column_freezes_after_one_iteration():
    n, ent, B, X0 = mr.freeze_columns()
    S = sr.System(ent, n, "f64")
    X, iters, res, _ = mr.run_multi(S, B, X0, 1000, 1e-8, 1)
    assert iters[0] == 1 and res[0] <= 1e-13 and iters[1] > 20
    X1, _, _, _ = mr.run_multi(S, B, X0, 1, 1e-8, 1)
    assert np.array_equal(X1[:, 0], X[:, 0])


def test_a_breakdown_names_its_column():
    n = 5
    ent = (np.arange(n), np.arange(n), -np.ones(n))
    S = sr.System(ent, n, "f64", "jacobi")
    B = np.ones((n, 3))
    B[:, 1] = 0.0
    with pytest.raises(mr.Breakdown) as e:
        mr.run_multi(S, B, np.zeros((n, 3)), 3)
    assert e.value.column == 0


@pytest.mark.parametrize("name", MID)
def test_the_gate_is_below_what_a_wrong_column_loop_does(name):
    """the mutation check, at k = 3: every mutation takes some column beyond F twin envelopes of its own reference at some j"""
    n, ent, B, X0, ks = mr.columns(name, 3)
    if sr.available(n):
        pytest.skip(sr.available(n))
    for label, precond in (("plain", None), ("jacobi", "jacobi")):
        env = mr.envelopes(name, precond)
        S = sr.System(ent, n, "f64", precond)
        # a rel_tol that freezes column 0 at an iterate of the list, well before the last one: halfway (on a log scale) between the
        # residual there and the smallest one before it, 5 % or more from either - the twins differ from the reference by ~1e-13
        hist = env[0].resid_hist
        jf = next(j for j in ks[2:-1] if hist[j] < 0.9 * min(hist[:j]))
        tol = float(np.sqrt(hist[jf] * min(hist[:jf])))
        for mutate in (None,) + mr.MUTATIONS:
            freeze = mutate == "frozen_updated"
            X, iters, res, kept = mr.run_multi(S, B, X0, max(ks), tol if freeze else 0.0, 1, mutate=mutate, keep=ks)
            if freeze:
                # column 0 is held to the iterate of the look that froze it, at every later j
                assert iters[0] == jf
                Xc, itc, _, _ = mr.run_multi(S, B, X0, max(ks), tol, 1)
                assert itc[0] == jf and mr.column_dev(env, 0, jf, Xc[:, 0])[0] <= env[0].gate(jf)
                ratio = {j: mr.column_dev(env, 0, jf, kept[j][:, 0])[0] / env[0].gate(jf) for j in ks if j >= jf and j in kept}
            else:
                ratio = {j: max(mr.column_dev(env, c, j, kept[j][:, c])[0] / env[c % 2].gate(j) for c in range(3)) for j in ks if j in kept}
            worst = max(ratio.values())
            print(f"mutation {str(mutate):15s} on {name} {label} k = 3: largest deviation / gate = {worst:.1e}")
            if mutate is None:
                assert worst <= 1.0 / sr.F + 1e-12, (name, label, ratio)  # the twin is inside its own envelope
            else:
                assert worst > 1.0, (name, label, mutate, ratio)
                if mutate == "tail":
                    assert ratio[1] > 1.0  # seen at the first iterate
