"""The preconditioners that the solvers apply by launches (csrc/precond.hip: by_launches), as fixed linear operators that a reference
recurrence can run in any arithmetic - TEST INFRASTRUCTURE ONLY (no GPU needed).

Three classes with one shape: apply(u, kind, variant) returns M^-1 u in the arithmetic `kind` of tests/solver_ref.py ("ld": np.longdouble,
"mp": mpmath, "f64") from float64 DATA - the factor values, the coefficient table, the scaling vector - so the extended-precision
reference and the float64 twins apply the same operator, and where that data is read back from the engine (tests/test_gpu_bicgstab.py,
test_gpu_gmres.py, test_gpu_minres.py) the engine applies it too: a deviation then belongs to the solver.  `variant` is the twin's
(row order, dot order) of cgls_ref.ROW_ORDERS x solver_ref.DOT_ORDERS: what each operator makes of it is its own business.

  FsaiOp       z = G^T (G u), G a CSR factor (fsai_ref.Fsai's or ctx.fsai_factor's); the row order is the order in which a row's (for
               G^T: a column's) products are added
  Ilu0Op       z = U^-1 L^-1 u in the natural row order, from factor values aligned to the CSR entries (ilu0_ref.Ilu0.values with
               order = arange(n), or ctx.ilu0_factors under ilu0_order = 0); trsv_ref.solve_longdouble in extended precision, and
               trsv_ref.solve_twin for the twins with LANES[dot order] lanes per row: the twins rotate through 1, 4 and 16
  ChebyshevOp  z = p_d(diag(s) A) diag(s) u, chebyshev_ref.apply over cgls_ref.Operator.mv with the float64 table of
               chebyshev_ref.coefficients - what csrc/chebyshev.hip computes on the host - and s_i = 1 / a_ii rounded to float64 as the
               engine's Jacobi kernel leaves it (scaled) or none

BICGSTAB_CASES, GMRES_CASES and SYM_CASES name the (system, preconditioner) pairs that the step-by-step tests run, shared by the CPU
and the GPU files.
"""
from __future__ import annotations

import collections

import numpy as np

import chebyshev_ref as cr
import fsai_ref as fr
import ilu0_ref as ir
import trsv_ref as tr
from cgls_ref import Operator
from solver_ref import _conv

LANES = {"forward": 1, "reversed": 4, "pairwise": 16}  # Ilu0Op: the lanes of the substitution twin, by the twin's dot order
REFERENCE_VARIANT = ("stored", "pairwise")


def entries_of(n, rp, cc, cv):
    """(row, col, val) of CSR arrays"""
    return np.repeat(np.arange(n), np.diff(np.asarray(rp, np.int64))), np.asarray(cc, np.int64), np.asarray(cv, np.float64)


class FsaiOp:
    name = "fsai"

    def __init__(self, n, g_rp, g_cc, g_val):
        self.n, self.entries, self._ops = n, entries_of(n, g_rp, g_cc, g_val), {}

    def apply(self, u, kind, variant=REFERENCE_VARIANT):
        key = (kind, variant[0])
        if key not in self._ops:
            self._ops[key] = Operator(self.entries, (self.n, self.n), kind, variant[0])
        G = self._ops[key]
        return G.rmv(G.mv(u))


def _substitute(n, ptr, col, val, diag, lower, b, unit):
    """trsv_ref.solve_longdouble's substitution in the arithmetic of b (object arrays of mpmath numbers included)"""
    x = b.copy()
    p = np.asarray(ptr).tolist()
    for i in (range(n) if lower else range(n - 1, -1, -1)):
        a, e = p[i], p[i + 1]
        if e > a:
            x[i] = x[i] - (val[a:e] * x[col[a:e]]).sum()
        if not unit:
            x[i] = x[i] / diag[i]
    return x


class Ilu0Op:
    name = "ilu0"

    def __init__(self, n, rp, cc, values):
        self.n = n
        lp, lc, lv, _, _, l_lower = tr.extract(n, rp, cc, values, tr.TRSV_LOWER)
        up, uc, uv, ud, has, u_lower = tr.extract(n, rp, cc, values, tr.TRSV_UPPER)
        assert l_lower and not u_lower and tr.bad_diagonal_row(ud, has) < 0
        self.L, self.U = (lp, lc, lv, np.ones(n), True), (up, uc, uv, ud, False)

    def apply(self, u, kind, variant=REFERENCE_VARIANT):
        z = u
        for (ptr, col, val, diag, lower), unit in ((self.L, True), (self.U, False)):
            if kind == "f64":
                z = tr.solve_twin(self.n, ptr, col, val, diag, lower, z, unit, lanes=LANES[variant[1]])
            elif kind == "ld":
                z = tr.solve_longdouble(self.n, ptr, col, val, diag, lower, z, unit)
            else:
                z = _substitute(self.n, ptr, col, _conv(val, kind), _conv(diag, kind), lower, z, unit)
        return z


class ChebyshevOp:
    name = "chebyshev"

    def __init__(self, n, entries, degree, scaled, lmin, lmax):
        self.n, self.entries, self.info, self._ops = n, entries, (degree, scaled, lmin, lmax), {}
        self.table = cr.coefficients(degree, lmin, lmax)  # float64: the engine's own table
        self.s = cr.inverse_diagonal(n, *_csr(n, entries)) if scaled else None

    def apply(self, u, kind, variant=REFERENCE_VARIANT):
        key = (kind, variant[0])
        if key not in self._ops:
            c0, c1, c2 = self.table
            self._ops[key] = (Operator(self.entries, (self.n, self.n), kind, variant[0]).mv, _conv(self.s, kind) if self.s is not None else None,
                              _conv(np.array([c0]), kind)[0], _conv(c1, kind), _conv(c2, kind))
        return cr.apply(*self._ops[key][:2], u, *self._ops[key][2:])


def _csr(n, entries):
    row, col, val = entries
    o = np.argsort(row, kind="stable")
    return np.searchsorted(np.asarray(row)[o], np.arange(n + 1)).astype(np.int32), np.asarray(col)[o].astype(np.int32), np.asarray(val, np.float64)[o]


def is_op(precond):
    return hasattr(precond, "apply")


def bound(precond, kind, row_order, dot_order):
    """u -> M^-1 u of one run of a recurrence: the operator in that run's arithmetic and as that twin's variant"""
    return lambda u: precond.apply(u, kind, (row_order, dot_order))


# ---- the (system, preconditioner) pairs of the step-by-step tests -------------------------------------------------------------------
# Set-up parameters: what the GPU tests hand to ctx.fsai_setup / ctx.chebyshev_setup (explicit bounds: no Lanczos estimate enters) and
# the CPU tests to fsai_ref.Fsai / ChebyshevOp; ILU(0) is in the natural row order (ilu0_order = 0) everywhere.
Spec = collections.namedtuple("Spec", "kind level degree scaled lmin lmax", defaults=(0, 0, True, 0.0, 0.0))
FSAI1, FSAI2, ILU0 = Spec("fsai", level=1), Spec("fsai", level=2), Spec("ilu0")
CHEB4 = Spec("chebyshev", degree=4, scaled=True, lmin=2.0 / 30, lmax=2.0)  # diag(s) A of a Laplacian has its spectrum in (0, 2)
CHEB2_SMALL = Spec("chebyshev", degree=2, scaled=True, lmin=0.25, lmax=2.0)
CHEB2_BIG = Spec("chebyshev", degree=2, scaled=True, lmin=0.5, lmax=1.5)  # a dominant diagonal 2 sum |off|: Gershgorin's disc around 1
CHEB2_PLAIN = Spec("chebyshev", degree=2, scaled=False, lmin=4.0 / 30, lmax=4.0)  # the 1-D Laplacian (2, -1) as it stands


def build(spec, n, entries, factor=None):
    """the operator of `spec` on the matrix `entries` (grouped by row).  factor: the engine's own values - (rp, cc, val) of G for FSAI,
    the values aligned to the CSR entries for ILU(0), chebyshev_info's (degree, scaled, lmin, lmax) - else the twins' (the CPU tests)"""
    rp, cc, cv = _csr(n, entries)
    if spec.kind == "fsai":
        if factor is None:
            f = fr.Fsai(n, rp, cc, cv, spec.level)
            factor = (f.rp, f.cc, f.values)
        return FsaiOp(n, *factor)
    if spec.kind == "ilu0":
        return Ilu0Op(n, rp, cc, factor if factor is not None else ir.Ilu0(n, rp, cc, cv, np.arange(n)).values)
    assert spec.kind == "chebyshev"
    degree, scaled, lmin, lmax = factor if factor is not None else spec[2:]
    assert (degree, bool(scaled), lmin, lmax) == (spec.degree, spec.scaled, spec.lmin, spec.lmax), "the handle's Chebyshev state is not the one asked for"
    return ChebyshevOp(n, (rp_rows(n, rp), cc.astype(np.int64), cv), degree, scaled, lmin, lmax)


def rp_rows(n, rp):
    return np.repeat(np.arange(n), np.diff(np.asarray(rp, np.int64)))


# BiCGSTAB and GMRES: bicgstab_ref's n1, n2, n3 (nonsymmetric; FSAI reads their lower triangles, which are positive definite), band4099
# and big; the 33 x 33 Laplacian (n = 1089, odd) for the two preconditioners that want a symmetric positive definite matrix; upwind
# convection-diffusion on 45 x 45 (n = 2025, odd, nonsymmetric) for ILU(0).  big runs under Chebyshev alone: ILU(0)'s substitution twin
# is a Python loop per row.
# band4099 under ILU(0) is GMRES's alone: its reference loses k = 13 there and nothing else, BiCGSTAB's (two products an iteration)
# loses three of the eight k, one more than bicgstab_ref.MAX_DROPPED allows.
LAP, CONV = "lap33", "convdiff45"
BICGSTAB_CASES = ([(name, spec) for spec in (FSAI1, ILU0, CHEB2_SMALL) for name in ("n1", "n2", "n3")]
                  + [(LAP, FSAI2), (LAP, CHEB4), (CONV, ILU0), ("big", CHEB2_BIG)])
GMRES_CASES = BICGSTAB_CASES[:-1] + [("band4099", ILU0), ("big", CHEB2_BIG)]
# MINRES, M from a separate positive definite handle P: minres_ref's shifted (P the Laplacian) and saddle (P = blockdiag(K, I)); n1, n2,
# n3 with P the 1-D Laplacian (2, -1) of that size; big with the 1-D Laplacian, unscaled.  ILU(0) is refused by spmv_minres.
SYM_CASES = ([(name, spec) for spec in (FSAI1, CHEB2_SMALL) for name in ("n1", "n2", "n3")]
             + [("shifted", FSAI2), ("shifted", CHEB4), ("saddle", FSAI1), ("saddle", CHEB4), ("big", CHEB2_PLAIN)])
BIG_KS = (1, 2, 3, 4, 5)  # (as tests/test_gpu_gmres.py asks of its big problem: the references take seconds per iteration there)


def label(name, spec):
    return f"{name}+{spec.kind}" + (str(spec.level) if spec.kind == "fsai" else str(spec.degree) if spec.kind == "chebyshev" else "")


def nonsym_problem(name, big_n=None):
    """(n, entries, b, x0, ks) of a BICGSTAB_CASES or GMRES_CASES system; b then x0 from default_rng(seed).uniform(-1, 1)"""
    import bicgstab_ref as br

    if name in br.PROBLEMS:
        n, ent, b, x0, ks = br.problem(name, big_n)
        return n, ent, b, x0, (BIG_KS if name == "big" else ks)
    n, rp, cc, cv = fr.laplacian_2d(33) if name == LAP else ir.convection_diffusion_2d(45)
    rng = np.random.default_rng(3100 + (LAP, CONV).index(name))
    b, x0 = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    return n, entries_of(n, rp, cc, cv), b, x0, br.KS


def laplacian_1d(n):
    i = np.arange(n)
    row, col = np.concatenate([i[1:], i, i[:-1]]), np.concatenate([i[:-1], i, i[1:]])
    val = np.concatenate([np.full(n - 1, -1.0), np.full(n, 2.0), np.full(n - 1, -1.0)])
    o = np.lexsort((col, row))
    return row[o], col[o], val[o]


def sym_problem(name, big_n=None):
    """minres_ref.problem's Problem with p_entries always set: the matrix the preconditioner is built from, grouped by row"""
    import minres_ref as mr

    p = mr.problem(name, big_n)
    if p.p_entries is None:
        p = p._replace(p_entries=laplacian_1d(p.n))
    if name == "big":
        p = p._replace(ks=BIG_KS)
    o = np.argsort(p.p_entries[0], kind="stable")
    return p._replace(p_entries=tuple(np.asarray(a)[o] for a in p.p_entries))
