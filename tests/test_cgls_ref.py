"""The references of tests/cgls_ref.py, checked on the CPU (no GPU): the extended-precision recurrence finds the least-squares
solution numpy finds, the problems of tests/test_gpu_cgls.py are still far from the noise floor at the last iterate checked, and
the gate is decades below what a wrong beta, a delta without its damping term, an s that was not reset or an element of x left
out does to an iterate.
"""
import numpy as np
import pytest

import cgls_ref as cr

SMALL = ("s1x1", "s2x1", "s3x2")
MID = ("r33x17", "r4097x4097", "r6001x4097", "r4097x6001", "band4099")
DAMPS = (0.0, 0.5)


def _skip_unless_available(shape):
    why = cr.available(max(shape))
    if why:
        pytest.skip(why)


@pytest.fixture(scope="module")
def envelopes():
    cache = {}

    def get(name, damp):
        if (name, damp) not in cache:
            shape, ent, b, x0, ks = cr.problem(name)
            cache[name, damp] = cr.Envelope(ent, shape, b, x0, ks, damp)
        return cache[name, damp]

    return get


@pytest.mark.parametrize("name", SMALL)
@pytest.mark.parametrize("damp", DAMPS)
def test_the_reference_ends_at_the_least_squares_solution(name, damp):
    """after min(m, n) iterations CGLS has the minimiser; damped: that of the augmented system [A; damp I] x = [b; 0]"""
    (m, n), ent, b, x0, ks = cr.problem(name)
    dense = np.zeros((m, n))
    np.add.at(dense, (ent[0], ent[1]), ent[2])
    want = np.linalg.lstsq(np.vstack([dense, damp * np.eye(n)]), np.concatenate([b, np.zeros(n)]), rcond=None)[0]
    k = min(m, n)
    assert ks[-1] == k
    x, nres, res = cr.cgls_reference(ent, (m, n), b, x0, (k,), damp)[k]
    assert np.max(np.abs(np.asarray(x, dtype=np.float64) - want)) <= 1e-12 * max(1.0, np.max(np.abs(want))), (name, damp)
    assert nres <= 1e-12
    assert abs(res - np.linalg.norm(b - dense @ want) / np.linalg.norm(b)) <= 1e-12


@pytest.mark.parametrize("name", MID)
@pytest.mark.parametrize("damp", DAMPS)
def test_the_twins_stay_close_and_the_last_iterate_is_above_the_noise_floor(envelopes, name, damp):
    shape, ent, b, x0, ks = cr.problem(name)
    _skip_unless_available(shape)
    assert np.all(x0 != 0) and ks == cr.KS
    env = envelopes(name, damp)
    worst = [max(env.envelope(k, what) for k in ks) for what in range(3)]
    print(f"twins on {name} damp {damp}: largest deviation of x_k {worst[0]:.2e}, of the normal residual {worst[1]:.2e}, of the residual "
          f"{worst[2]:.2e}; sqrt(gamma_13 / gamma_0) = {env.ref_nres[13] / env.nres_hist[0]:.2e}")
    # no gate is taken at the noise floor: gamma_13 > 1e-20 gamma_0
    assert (env.ref_nres[13] / env.nres_hist[0]) ** 2 > 1e-20, (name, damp, env.ref_nres)
    assert len(env.twin_dev[13]) == len(cr.DOT_ORDERS) * len(cr.ROW_ORDERS)
    # float64 over a dozen iterations: the sequential dot products of n terms lose ~sqrt(n) eps
    assert cr.FLOOR <= worst[0] <= 64 * max(np.sqrt(max(shape)), 16) * 2.0**-52, (name, damp, worst)


FIRST_SEEN = {"beta": (2,), "nodamp": (1,), "stale_s": (1, 2), "tail": (1,)}


@pytest.mark.parametrize("name", MID)
def test_the_gate_is_far_below_what_a_wrong_recurrence_does(envelopes, name):
    """the mutation check: each mutation moves x_k by more than 1000 gates at the first k it touches"""
    shape, ent, b, x0, ks = cr.problem(name)
    _skip_unless_available(shape)
    Op = cr.Operator(ent, shape, "f64")
    for damp in DAMPS:
        env = envelopes(name, damp)
        for mutate in cr.MUTATIONS:
            if mutate == "nodamp" and damp == 0.0:
                continue  # (nothing to leave out)
            out, _, _ = cr.run_cgls(Op, b, x0, ks, damp, mutate=mutate)
            ratio = {k: env.x_dev(k, out[k][0]) / env.gate(k) for k in ks}
            first = min(k for k in ks if ratio[k] > 1)
            print(f"mutation {mutate:8s} on {name} damp {damp}: first seen at k = {first}, deviation / gate there {ratio[first]:.1e}")
            assert first in FIRST_SEEN[mutate], (name, damp, mutate, ratio)
            assert ratio[first] > 1000, (name, damp, mutate, ratio)


def test_the_row_orders_are_different_sums_of_the_same_products():
    shape, ent, b, x0, ks = cr.problem("r4097x6001")
    a, c = cr.Operator(ent, shape, "f64", "stored"), cr.Operator(ent, shape, "f64", "reversed")
    ya, yc = a.mv(x0), c.mv(x0)
    assert not np.array_equal(ya, yc) and np.max(np.abs(ya - yc)) <= 64 * 2.0**-52 * np.max(np.abs(ya))
    za, zc = a.rmv(b), c.rmv(b)
    assert not np.array_equal(za, zc) and np.max(np.abs(za - zc)) <= 64 * 2.0**-52 * np.max(np.abs(za))
    assert np.any(np.diff(a.t_ptr) == 0), "4097 x 6001 is meant to have columns without an entry"


def test_the_mpmath_fallback_is_the_same_reference():
    pytest.importorskip("mpmath")
    shape, ent, b, x0, ks = cr.problem("s3x2")
    for damp in DAMPS:
        mp = cr.cgls_reference(ent, shape, b, x0, ks, damp, force_mp=True)
        if cr._hp_kind(3) == "ld":
            ld = cr.cgls_reference(ent, shape, b, x0, ks, damp)
            for k in ks:
                assert max(abs(float(p) - float(l)) for p, l in zip(mp[k][0], ld[k][0])) <= 1e-15
                assert abs(mp[k][1] - ld[k][1]) <= 1e-15 and abs(mp[k][2] - ld[k][2]) <= 1e-15
