"""spmv_cg iterate by iterate against an extended-precision reference (`pytest -m gpu`).

spmv_cg(max_iter = k, rel_tol = 0) runs exactly k iterations from the x passed in.  For k in (1, 2, 3, 4, 5, 8, 9, 13) - around
the period of the scalar ring, and far enough for an error to grow - x_k and the returned ||r_k|| / ||b|| are held to the
textbook recurrence in np.longdouble (tests/solver_ref.py).  The gate at step k is F = 8 times the largest deviation from that
reference of any float64 twin of the recurrence (two arrangements x three dot orders), measured on the reference's own
arithmetic and floored at 2^-50: about 1e-14 .. 1e-12.  A wrong beta, a stale ring slot, a wrong alpha[(k + 3) & 3] or one
element left out moves x_k by 1e-1 .. 1e-4 (tests/test_solver_ref.py), and none of them shows in the residual of the solution
that tests/test_gpu_solver.py asserts.

Every arrangement of the recurrence runs: two launches per iteration (Chronopoulos-Gear) and three, each plain and with Jacobi;
symmetric Gauss-Seidel in row order and in the multicolour order; the captured-graph replay; with the host looking at the
residual after every iteration and only at the end; each on an x that is 256-byte aligned (the 16-byte kernels) and on one that
sits 8 bytes off a 16-byte boundary (the one-element kernels).  The systems: n = 1, 2, 3; a 33 x 33 Laplacian; a 4097-row
dominant random system whose diagonal is stored twice in unsorted columns; Laplacians of n = 525,625 and n = 1,050,625 (odd,
and beyond one sweep of the one-element and the two-element kernels' grids).  The products behind the iteration run under every
CSR kernel that the solver fuses its dot product into or trails it behind.  test_every_arrangement_ran asserts at the end that
all of it ran; with SPMV_SOLVER_RATIOS=<file> it also writes the largest GPU deviation over twin envelope per arrangement.
"""
import collections
import os

import numpy as np
import pytest

import oracle_lib as ol
import solver_ref as sr

pytestmark = pytest.mark.gpu
AUTO, VECTOR, SCALAR, PANEL, TWOPHASE, SPLIT = 0, 1, 3, 4, 5, 7
ARRANGEMENTS = ("fused", "fused+jacobi", "three", "three+jacobi", "symgs rows", "symgs colours")
SEEN = set()  # (arrangement | "graph", "wide" | "scalar")
RUNS = collections.Counter()
RATIO = {}  # (arrangement, alignment) -> (largest deviation / twin envelope, where), for x and for the residual
_ENV = {}
_MAT = {}


def _problem(name):
    if name not in _MAT:
        n, ent, b, x0, ks = sr.problem(name)
        _MAT[name] = (n, ent, b, x0, ks, sr.csr_arrays(n, *ent))
    return _MAT[name]


def _envelope(name, label, precond):
    """the reference iterates and twin envelopes of one problem under one preconditioner (computed once: seconds at n = 10^6)"""
    if (name, label) not in _ENV:
        n, ent, b, x0, ks, _ = _problem(name)
        why = sr.available(n)
        if why:
            pytest.skip(why)
        _ENV[name, label] = sr.Envelope(ent, b, x0, ks, precond)
    return _ENV[name, label]


def _start_vector(ctx, x0, aligned):
    """x0 on the device, 256-byte aligned (spmv_vec_create) or 8 bytes past a 16-byte boundary (a wrapped pointer into a vector of
    n + 1: an ordinary, legal double*)"""
    n = len(x0)
    if aligned:
        v = ctx.vector_from(x0)
        assert v.device_ptr % 16 == 0
        return v, None
    base = ctx.vector(n + 1)
    base.fill(0.0)
    ptr = base.device_ptr + 8
    assert ptr % 16 == 8
    v = ctx.wrap_vector(ptr, n)
    v.upload(x0)
    return v, base


def _note(key, kind, ratio, where):
    old = RATIO.setdefault(key, {})
    if ratio > old.get(kind, (0.0, ""))[0]:
        old[kind] = (ratio, where)


def _steps(ctx, monkeypatch, A, name, env, arrangement, aligned, graph=False, what=""):
    """every k of the problem's list with check_every in {1, k} (graph: k >= 4, check_every = k): iters, x_k, ||r_k|| / ||b||"""
    n, ent, b, x0, ks, _ = _problem(name)
    monkeypatch.setenv("SPMV_CG_THREE_LAUNCHES", "1" if arrangement.startswith("three") else "0")
    monkeypatch.setenv("SPMV_CG_GRAPH", "1" if graph else "0")
    kw = {"jacobi": arrangement.endswith("jacobi"), "symgs": arrangement.startswith("symgs")}
    db = ctx.vector_from(b)
    width = "wide" if aligned and n >= 2 else "scalar"
    misses = []
    for k in ks:
        if graph and k < 4:
            continue
        for check_every in ((k,) if graph or k == 1 else (1, k)):
            x, keep = _start_vector(ctx, x0, aligned)
            replays = ctx.get_param("cg_graph_replays")
            iters, relres = ctx.cg(A, db, x, max_iter=k, rel_tol=0.0, check_every=check_every, **kw)
            got = x.download()
            del x, keep
            tag = f"{name} {arrangement}{' graph' if graph else ''} {width} {what}k={k} check_every={check_every}"
            assert iters == k, (tag, iters)
            if graph:
                assert ctx.get_param("cg_graph_replays") - replays == k // 4, (tag, "the captured iterations were not replayed")
            dev, rdev = env.x_dev(k, got), env.resid_dev(k, relres)
            print(f"{tag}: x deviation {dev:.2e} (twins {env.envelope(k):.2e}, gate {env.gate(k):.2e}); residual {relres:.6e} "
                  f"deviation {rdev:.2e} (twins {env.envelope(k, 1):.2e}, gate {env.gate_resid(k):.2e})")
            key = ("graph" if graph else arrangement, width)
            _note(key, "x", dev / env.envelope(k), tag)
            _note(key, "residual", rdev / env.envelope(k, 1), tag)
            if not dev <= env.gate(k):
                misses.append(f"{tag}: max|x_k - ref_k| / max|ref_k| = {dev:.3e} > gate {env.gate(k):.3e}")
            if not rdev <= env.gate_resid(k):
                misses.append(f"{tag}: rel_resid {relres!r} against {env.ref_resid[k]!r}: {rdev:.3e} > gate {env.gate_resid(k):.3e}")
    SEEN.add(("graph" if graph else arrangement, width))
    return misses


def _symgs_precond(ctx, orc, A, name, order):
    """the sweep order the engine reports, and - where the colouring is proper - its colour classes for the vectorised reference"""
    n, _, _, _, _, (rp, cc, cv) = _problem(name)
    A.set_param("symgs_order", order)
    seq = ctx.symgs_order(A)
    if order == 0:
        assert np.array_equal(seq, np.arange(n))
        return ("symgs", seq)
    ncol, colour, want_seq = ol.greedy_colour_order(orc, rp, cc)
    assert np.array_equal(seq, want_seq) and A.get_param("symgs_colours") == ncol
    if n <= 3 or not A.get_param("symgs_fused"):
        return ("symgs", seq)  # sequential in the reported order
    return ("symgs", seq, colour)


def _cases():
    out = []
    for name in sr.PROBLEMS:
        for arrangement in ARRANGEMENTS:
            if arrangement.startswith("symgs") and (name == "lap1025" or (name == "lap725" and arrangement == "symgs rows")):
                continue  # the sequential reference sweep is for small n; n = 525,625 runs red-black, one vector operation per colour
            out.append((name, arrangement))
    return out


@pytest.mark.parametrize("name,arrangement", _cases(), ids=lambda v: v.replace(" ", "_"))
def test_cg_iterates_match_the_extended_precision_recurrence(ctx, orc, pkg, monkeypatch, name, arrangement):
    n, ent, b, x0, ks, (rp, cc, cv) = _problem(name)
    A = ctx.csr(n, n, rp, cc, cv)
    if arrangement.startswith("symgs"):
        precond = _symgs_precond(ctx, orc, A, name, 0 if arrangement == "symgs rows" else 1)
        if name == "lap725":
            assert len(precond) == 3 and A.get_param("symgs_colours") == 2, "red-black is a proper colouring"
    else:
        precond = "jacobi" if arrangement.endswith("jacobi") else None
    label = arrangement.split("+")[1] if "+" in arrangement else (arrangement if precond else "plain")
    env = _envelope(name, label, precond)
    misses = []
    for aligned in (True, False):
        misses += _steps(ctx, monkeypatch, A, name, env, arrangement, aligned)
    assert not misses, "\n".join(misses)
    RUNS["steps"] += 1


# every arrangement without a sweep replays on the two mid-size systems, the default one on the large system as well
GRAPH_CASES = [(name, a) for name in ("lap33", "rand4097") for a in ARRANGEMENTS[:4]] + [("lap725", "fused")]


@pytest.mark.parametrize("name,arrangement", GRAPH_CASES, ids=lambda v: v.replace(" ", "_"))
def test_cg_graph_replay_iterates_match_the_recurrence(ctx, pkg, monkeypatch, name, arrangement):
    """SPMV_CG_GRAPH=1, check_every = k >= 4: k // 4 replays of the captured four iterations, the rest as plain launches"""
    n, ent, b, x0, ks, (rp, cc, cv) = _problem(name)
    A = ctx.csr(n, n, rp, cc, cv)
    precond = "jacobi" if arrangement.endswith("jacobi") else None
    env = _envelope(name, "jacobi" if precond else "plain", precond)
    misses = []
    for aligned in (True, False):
        misses += _steps(ctx, monkeypatch, A, name, env, arrangement, aligned, graph=True)
    assert not misses, "\n".join(misses)
    RUNS["graph"] += 1


KERNELS = (("vector", VECTOR), ("scalar", SCALAR), ("panel", PANEL), ("twophase", TWOPHASE), ("split", SPLIT))


@pytest.mark.parametrize("name", ["rand4097", "lap725"])
@pytest.mark.parametrize("kernel", KERNELS, ids=lambda v: v[0])
def test_cg_iterates_under_every_product_kernel(ctx, pkg, monkeypatch, name, kernel):
    """p.Ap (u.Au) comes from the product kernel's own fused dot (VECTOR, PANEL, TWOPHASE, SPLIT's short rows) or from the dot pass
    behind it (SCALAR, SPLIT): the same iterates under each (AUTO runs in the test above)"""
    n, ent, b, x0, ks, (rp, cc, cv) = _problem(name)
    A = ctx.csr(n, n, rp, cc, cv)
    label, kid = kernel
    if kid == SPLIT:
        A.set_param("split_row_threshold", 3)  # rows of more than 3 entries are long: both halves of the split have rows
        A.set_param("split_mode", 0)
    A.set_kernel(kid)
    assert A.info.kernel == kid
    misses = []
    for arrangement, aligned in (("fused", True), ("three+jacobi", False), ("fused+jacobi", False), ("three", True)):
        precond = "jacobi" if arrangement.endswith("jacobi") else None
        env = _envelope(name, "jacobi" if precond else "plain", precond)
        misses += _steps(ctx, monkeypatch, A, name, env, arrangement, aligned, what=f"kernel={label} ")
    assert not misses, "\n".join(misses)
    assert A.info.kernel == kid
    SEEN.add(("kernel", label))
    RUNS["kernels"] += 1


def test_every_arrangement_ran():
    """{fused, fused+jacobi, three, three+jacobi, symgs rows, symgs colours, graph} x {wide, scalar} and every product kernel ran"""
    expect = {"steps": len(_cases()), "graph": len(GRAPH_CASES), "kernels": 2 * len(KERNELS)}
    if any(RUNS[f] != c for f, c in expect.items()):
        pytest.skip(f"the coverage check needs every test of this module (ran {dict(RUNS)}, expected {expect})")
    need = {(a, w) for a in ARRANGEMENTS + ("graph",) for w in ("wide", "scalar")} | {("kernel", k) for k, _ in KERNELS}
    assert need <= SEEN, f"never ran: {sorted(need - SEEN)}"
    lines = ["# spmv_cg iterate by iterate (tests/test_gpu_solver_steps.py): the largest deviation of the GPU's x_k, and of its",
             "# ||r_k|| / ||b||, from the np.longdouble recurrence, in units of the float64 twins' own largest deviation at that k",
             "# (the gate is 8).  arrangement | kernels' width | x ratio | residual ratio | where the x ratio was largest"]
    for (a, w), r in sorted(RATIO.items()):
        lines.append(f"{a:14s} {w:6s}  x {r['x'][0]:6.3f}  residual {r['residual'][0]:6.3f}  ({r['x'][1]})")
        assert r["x"][0] <= sr.F and r["residual"][0] <= sr.F
    print("\n".join(lines))
    out = os.environ.get("SPMV_SOLVER_RATIOS")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
