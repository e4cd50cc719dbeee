"""Every kernel of the forward, transposed and multi-vector products on EXACT, POISONED inputs (`pytest -m gpu`).

Values, x and y0 are dyadic (tests/exact.py): every sum is exact in any order, so every kernel - the ones that reorder a row's
sum (panel, two-phase, segmented scan, split, the CSC scatter, the COO scan, every companion of the transposed product) as
well as the ones that keep the reference's order - must return the bits of an integer reference that owes nothing to the
oracle, np.array_equal, after one call and after several accumulating calls.  The smallest term of an output can sit 2^40
below its largest: the dropped or doubled term that the parity gate (1e-10 x (|A||x|)_i) cannot see changes the bits here.
Every x entry no stored entry reads is NaN or +-inf, and in a third of the seeds the columns where pad reads land (0, the
last, multiples of 16, two-phase panel bases) are left unread: a pad product that is not thrown away shows as NaN.

Shapes are seeded (SPMV_FUZZ_BASE moves them, as in test_gpu_fuzz.py, whose CSR shape generator this shares).  Each test
records what actually ran (kernel, layouts, padded copies); test_every_kernel_ran asserts at the end that the seeds reached
every kernel named here.  The full-size cases (C3 ELL, C4 COO transposed; C3 multi) use the generators' U(-1,1) values and
the parity gate.
"""
import collections
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import exact as ex
import oracle_lib as ol
from test_gpu_fuzz import _random_csr

pytestmark = pytest.mark.gpu
BASE = int(os.environ.get("SPMV_FUZZ_BASE", "0"))
REPS = 3  # y after 1 call and after REPS accumulating calls
AUTO, VECTOR, LDSWIN, SCALAR, PANEL, TWOPHASE, SEGSCAN, SPLIT, ELLK = range(9)
PANEL_COLS = (20_000, 7_000)  # the two-phase panel widths run below: their bases are among the columns left unread
SEEN = collections.defaultdict(set)  # test family -> what ran
RUNS = collections.Counter()  # test family -> seeds run
N_CSR, N_COO, N_CSC, N_ELL, N_DIA, N_MULTI = 22, 12, 12, 12, 10, 10


def _fail(got, want):
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
    i = int(bad[0]) if bad.size else -1
    return f"{bad.size} outputs differ; first {i}: got {got[i]!r}, want {want[i]!r}" if bad.size else "equal"


def _check_apply(ctx, apply, dx, y0, want1, wantr, what):
    """y0 -> one call -> want1; REPS - 1 more calls -> wantr"""
    dy = ctx.vector_from(y0)
    apply(dx, dy)
    ctx.sync()
    got = dy.download()
    assert np.array_equal(got, want1), f"{what}, 1 call: {_fail(got, want1)}"
    for _ in range(REPS - 1):
        apply(dx, dy)
    ctx.sync()
    got = dy.download()
    assert np.array_equal(got, wantr), f"{what}, {REPS} calls: {_fail(got, wantr)}"


class Exact:
    """one entry list with its dyadic x (poisoned where unread), y0 and the exact results after 1 and REPS calls"""

    def __init__(self, rng, nout, nin, entries, bits, e, used=None):
        self.entries, self.e = entries, e
        self.x = ex.dyadic(rng, nin, bits, e)
        self.y0 = ex.dyadic(rng, nout, bits, e)
        self.want1 = ex.exact_product(nout, *entries, self.x, e, y0=self.y0)
        self.wantr = ex.exact_product(nout, *entries, self.x, e, y0=self.y0, reps=REPS)
        self.xp = ex.poison(self.x, entries[1] if used is None else used)

    def check(self, ctx, A, what, transpose=False, dx=None):
        fn = ctx.apply_transpose if transpose else ctx.apply
        _check_apply(ctx, lambda x, y: fn(A, x, y), dx if dx is not None else ctx.vector_from(self.xp), self.y0, self.want1, self.wantr, what)


def _bits(*outs):
    """(B, E) for the longest output of several entry lists: [(out_idx, nout), ...]"""
    return ex.choose_bits(max(ex.max_terms(o, n) for o, n in outs), REPS)


def _dyadic_values(rng, n, bits, e, zeros):
    v = ex.dyadic(rng, n, bits, e)
    if zeros:
        v[rng.random(n) < 0.02] = 0.0  # explicit zeros: their columns count as read
    return v


# ---- CSR: every kernel, forward and transposed --------------------------------------------------------------------------------
def _special_csr(i):
    """the edges: 1 x 1, one long row, one column, empty rows beside rows longer than every chunk, wide and tall"""
    rng = np.random.default_rng(BASE + 11_500 + i)
    if i == 0:
        nrow, ncol, lens = 1, 1, np.array([1])
    elif i == 1:
        nrow, ncol, lens = 1, 200_000, np.array([70_000])
    elif i == 2:
        nrow, ncol = 70_000, 1
        lens = rng.integers(0, 3, nrow)
    elif i == 3:  # empty rows and rows longer than every chunk / batch (split chunks of 4096, panel and two-phase chunks)
        nrow, ncol = 30_000, 30_000
        lens = np.where(rng.random(nrow) < 0.3, 0, rng.integers(1, 12, nrow))
        lens[[5, 17_000, nrow - 1]] = [9000, 40_000, 5000]
    elif i == 4:  # tall: 400K rows x 50 columns
        nrow, ncol = 400_000, 50
        lens = rng.poisson(3, nrow)
    else:  # wide: 40 rows x 3M columns
        nrow, ncol = 40, 3_000_000
        lens = rng.integers(0, 9000, nrow)
    rp = np.zeros(nrow + 1, np.int64)
    rp[1:] = np.cumsum(lens)
    cc = rng.integers(0, ncol, int(rp[-1]))
    return nrow, ncol, rp.astype(np.int32), cc.astype(np.int32)


def _csr_shape(seed):
    if seed < 6:
        return _special_csr(seed)
    rng = np.random.default_rng(BASE + 1000 + seed)  # test_gpu_fuzz.py's shapes for the same seeds
    nrow, ncol, rp, cc, _ = _random_csr(rng)
    return nrow, ncol, rp, cc


def _csr_kernel_runs(capi, A, rng, nnz, ncol):
    """(label, setup) of every CSR kernel and parameter set test_gpu_fuzz.py runs"""
    runs = [("auto", lambda: None)]
    for lanes in (1, 4, 32):
        runs.append((f"vector lanes={lanes}", lambda lanes=lanes: A.set_kernel(VECTOR, lanes)))
    runs.append(("scalar", lambda: A.set_kernel(SCALAR)))
    if A.get_param("window_max_span") and A.get_param("window_max_span") <= 8192:
        runs.append(("lds window", lambda: A.set_kernel(LDSWIN, 8)))
    if nnz:
        combos = [(int(rng.choice([0, 3, 4])), int(rng.choice([2, 4, 8, 16])), int(rng.choice([0, 1, 2])), int(rng.choice([0, 1, 3])),
                   int(rng.choice([0, 0, 7, 333, 20_000])), int(rng.choice([0, 16, 4096]))) for _ in range(3)]
        combos.append((4, 8, 2, 1, 0, 0))
        for combo in combos:
            def panel(combo=combo):
                for k, v in zip(("panel_aos", "panel_unroll", "panel_pipe", "panel_sync", "panel_rows", "panel_width"), combo):
                    A.set_param(k, v)
                A.set_kernel(PANEL)
            runs.append((f"panel {combo}", panel))
        if nnz + 16 * ((ncol + 6999) // 7000) * 256 < 2**31:
            for cols, rotate in ((20_000, 256), (7_000, 0), (20_000, 8)):
                def twophase(cols=cols, rotate=rotate):
                    A.set_param("twophase_panel_cols", cols)
                    A.set_param("twophase_rotate", rotate)
                    A.set_kernel(TWOPHASE)
                runs.append((f"two-phase cols={cols} rotate={rotate}", twophase))
        runs.append(("segscan", lambda: A.set_kernel(SEGSCAN)))
        for mode in (0, 1, 2):
            for thr in (1, 3):
                def split(mode=mode, thr=thr):
                    A.set_param("split_row_threshold", thr)
                    A.set_param("split_mode", mode)
                    A.set_kernel(SPLIT)
                runs.append((f"split mode={mode} threshold={thr}", split))

    def ell_copy():
        try:
            A.set_kernel(ELLK)
        except capi.SpmvError as err:
            assert "out of proportion" in str(err) or "empty row" in str(err), err
            return False
        return True

    runs.append(("ell copy", ell_copy))
    return runs


def _record_csr(A, label, family="csr"):
    k = A.info.kernel
    SEEN[family].add(k)
    if k == PANEL:
        SEEN[family + ":panel_layout"].add(A.get_param("panel_layout"))
    if k == TWOPHASE:
        SEEN[family + ":twophase_padded"].add(A.get_param("twophase_padded") > 0)
    if k == SPLIT and label.startswith("split mode="):
        SEEN[family + ":split_mode"].add(int(label.split()[1][5:]))  # the mode asked for (0: chosen by the rows' density)


@pytest.mark.parametrize("seed", range(N_CSR))
def test_exact_csr_every_kernel_forward_and_transposed(ctx, pkg, seed):
    capi = pkg.capi
    nrow, ncol, rp, cc = _csr_shape(seed)
    rng = np.random.default_rng(BASE + 11_000 + seed)
    if seed % 3 == 0:
        cc = ex.avoid_columns(cc, ncol, PANEL_COLS)
    fwd = ex.csr_entries(rp, cc, np.zeros(len(cc)))
    bits, e = _bits((fwd[0], nrow), (fwd[1], ncol))
    cv = _dyadic_values(rng, len(cc), bits, e, zeros=seed % 4 == 1)
    fwd = ex.csr_entries(rp, cc, cv)
    F = Exact(rng, nrow, ncol, fwd, bits, e)
    T = Exact(rng, ncol, nrow, ex.transposed(fwd), bits, e)  # x poisoned on the empty rows
    what = f"seed {seed}: CSR {nrow} x {ncol}, {len(cc)} entries"
    A = ctx.csr(nrow, ncol, rp, cc, cv)
    dx = ctx.vector_from(F.xp)
    for label, setup in _csr_kernel_runs(capi, A, rng, len(cc), ncol):
        if setup() is False:
            continue
        F.check(ctx, A, f"{what}, {label} (kernel {A.info.kernel})", dx=dx)
        _record_csr(A, label)
        if label == "ell copy":
            SEEN["csr"].add("ell copy")
    # the small-vector path of spmv_apply_host (x + y under 1 MB) for a few kernels
    if 8 * (nrow + ncol) < (1 << 20):
        for kernel in (AUTO, SCALAR, PANEL, SEGSCAN):
            if kernel in (PANEL, SEGSCAN) and not len(cc):
                continue
            A.set_kernel(kernel)
            y = F.y0.copy()
            ctx.apply_host(A, F.xp.copy(), y)
            assert np.array_equal(y, F.want1), f"{what}: apply_host kernel {kernel}: {_fail(y, F.want1)}"
            SEEN["apply_host"].add(kernel)
    # the transposed product: the CSC companion under AUTO, its scatter, its row-grouped copy
    for kernel in (AUTO, VECTOR, PANEL):
        B = ctx.csr(nrow, ncol, rp, cc, cv)
        B.set_param("transpose_kernel", kernel)
        T.check(ctx, B, f"{what}, transposed, companion kernel {kernel}", transpose=True)
        SEEN["csr^T"].add(B.get_param("transpose_kernel"))
    RUNS["csr"] += 1


def _host_stores_child(mode):
    child = Path(__file__).with_name("child_exact_host.py")
    env = dict(os.environ, SPMV_HOST_STORES=mode, SPMV_FUZZ_BASE=str(BASE))
    r = subprocess.run([sys.executable, str(child)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "EXACT_HOST_OK" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.parametrize("mode", ["1", "0"])
def test_exact_apply_host_with_host_stores_on_and_off(mode):
    """spmv_apply_host on exact poisoned inputs in a fresh process per SPMV_HOST_STORES value (read once per context)"""
    out = _host_stores_child(mode)
    assert f"host_stores={mode}" in out or mode == "1", out


# ---- COO ----------------------------------------------------------------------------------------------------------------------
def _coo_shape(rng, seed):
    nrow = int(rng.choice([1, 17, 3000, 90_000, 500_000]))
    ncol = int(rng.choice([1, 100, 50_000, 2_000_000]))
    nnz = int(rng.choice([0, 1, 1000, 400_000, 2_200_000]))
    if seed == 0:
        nrow, ncol, nnz = 1, 1, 3
    row = rng.integers(0, nrow, nnz).astype(np.int32)
    if rng.uniform() < 0.5:
        row = np.sort(row)
    if nnz > 10 and rng.uniform() < 0.5:
        row[: nnz // 50] = row[0]  # a hub row
    col = rng.integers(0, ncol, nnz).astype(np.int32)
    if nnz > 10:  # duplicates, in file order
        src, dst = rng.integers(0, nnz, nnz // 20), rng.integers(0, nnz, nnz // 20)
        row[dst], col[dst] = row[src], col[src]
    return nrow, ncol, row, col


@pytest.mark.parametrize("seed", range(N_COO))
def test_exact_coo_forward_and_transposed(ctx, pkg, seed):
    capi = pkg.capi
    rng = np.random.default_rng(BASE + 12_000 + seed)
    nrow, ncol, row, col = _coo_shape(rng, seed)
    if seed % 3 == 0:
        col = ex.avoid_columns(col, ncol, PANEL_COLS)
    bits, e = _bits((row, nrow), (col, ncol))
    val = _dyadic_values(rng, len(row), bits, e, zeros=seed % 4 == 1)
    ent = ex.coo_entries(row, col, val)
    F = Exact(rng, nrow, ncol, ent, bits, e)
    T = Exact(rng, ncol, nrow, ex.transposed(ent), bits, e)
    what = f"seed {seed}: COO {nrow} x {ncol}, {len(row)} entries"
    A = ctx.coo(nrow, ncol, row, col, val)
    dx = ctx.vector_from(F.xp)
    rr = ctx.xcd_round_robin()[0]
    for kernel in (AUTO, VECTOR, PANEL):
        A.set_kernel(kernel)
        F.check(ctx, A, f"{what}, kernel {kernel} (runs {A.info.kernel}, copy {A.get_param('rowgrouped_kernel')})", dx=dx)
        SEEN["coo"].add(A.info.kernel)
        if A.info.kernel == PANEL:
            SEEN["coo:rowgrouped"].add(A.get_param("rowgrouped_kernel"))
    if rr == 1 and len(row):
        A.set_kernel(VECTOR)
        per_xcd = int(rng.integers(1, 9))
        A.set_param("coo_column_bins", per_xcd)
        assert A.get_param("coo_column_bins") == 8 * per_xcd
        F.check(ctx, A, f"{what}, scan over {8 * per_xcd} column bins", dx=dx)
        SEEN["coo"].add("bins")
        SEEN["coo:bins_padded"].add(A.get_param("coo_bins_padded") > len(row))
        A.set_param("coo_column_bins", 0)
        F.check(ctx, A, f"{what}, scan without column bins", dx=dx)
    for kernel in (AUTO, VECTOR, PANEL):
        B = ctx.coo(nrow, ncol, row, col, val)
        B.set_param("transpose_kernel", kernel)
        T.check(ctx, B, f"{what}, transposed, companion kernel {kernel}", transpose=True)
        SEEN["coo^T"].add(B.get_param("transpose_kernel"))
    RUNS["coo"] += 1


def test_exact_coo_transposed_over_column_bins(ctx, pkg):
    """the COO companion of a large handle (more than 393,216 rows of A, 2M+ entries) under VECTOR: its scan over column bins
    where workgroups are dealt round-robin over the XCDs (16 bytes per padded entry), else over the borrowed arrays"""
    rng = np.random.default_rng(BASE + 12_900)
    nrow, ncol, nnz = 600_000, 250_000, 2_300_000
    row = rng.integers(0, nrow, nnz).astype(np.int32)
    col = np.sort(rng.integers(0, ncol, nnz)).astype(np.int32)
    bits, e = _bits((row, nrow), (col, ncol))
    val = ex.dyadic(rng, nnz, bits, e)
    T = Exact(rng, ncol, nrow, ex.transposed(ex.coo_entries(row, col, val)), bits, e)
    A = ctx.coo(nrow, ncol, row, col, val)
    A.set_param("transpose_kernel", VECTOR)
    A.transpose_setup()
    tb = A.get_param("transpose_bytes")
    if ctx.xcd_round_robin()[0] == 1:
        assert tb >= 16 * nnz, f"the companion's column bins were not built: transpose_bytes {tb}"
        SEEN["coo^T"].add("bins")
    else:
        assert tb < 16 * nnz, tb
        SEEN["coo^T"].add("scan in place")
    T.check(ctx, A, f"COO {nrow} x {ncol}, transposed, companion scan (transpose_bytes {tb})", transpose=True)


# ---- CSC ----------------------------------------------------------------------------------------------------------------------
def _csc_shape(rng, seed):
    """columns of Poisson length, a few very long ones (SPLIT on the companion: its threshold is a sixteenth of the longest),
    rows banded around the column's diagonal in half the seeds (an LDS window on the companion)"""
    nrow = int(rng.choice([1, 300, 40_000, 200_000]))
    ncol = int(rng.choice([1, 77, 30_000, 120_000]))
    if seed == 0:
        nrow, ncol = 1, 1
    if seed in (1, 2):  # a narrow band (the LDS window fits); no empty and no long column (the ELL copy is accepted)
        nrow, ncol = 40_000, 30_000
    lens = rng.poisson(rng.uniform(0.5, 12), ncol)
    if seed == 2:
        lens = 1 + rng.poisson(4, ncol)
    elif ncol > 10:
        lens[rng.integers(0, ncol, 3)] = int(rng.choice([2000, 20_000, 60_000]))
    cp = np.zeros(ncol + 1, np.int64)
    cp[1:] = np.cumsum(lens)
    cols = np.repeat(np.arange(ncol, dtype=np.int64), lens)
    if (seed % 2 == 0 or seed == 1) and nrow > 100:
        w = 8 if seed == 1 else int(rng.choice([8, 100, 1000]))
        r = np.clip(cols * nrow // max(ncol, 1) + rng.integers(-w, w + 1, len(cols)), 0, nrow - 1)
    else:
        r = rng.integers(0, nrow, len(cols))
    return nrow, ncol, cp.astype(np.int32), cols, r.astype(np.int32)


@pytest.mark.parametrize("seed", range(N_CSC))
def test_exact_csc_forward_and_every_companion_kernel(ctx, pkg, seed):
    capi = pkg.capi
    rng = np.random.default_rng(BASE + 13_000 + seed)
    nrow, ncol, cp, cols, cr = _csc_shape(rng, seed)
    bits, e = _bits((cr, nrow), (cols, ncol))
    cv = _dyadic_values(rng, len(cr), bits, e, zeros=seed % 4 == 1)
    ent = ex.csc_entries(cp, cr, cv)
    F = Exact(rng, nrow, ncol, ent, bits, e)
    T = Exact(rng, ncol, nrow, ex.transposed(ent), bits, e)
    what = f"seed {seed}: CSC {nrow} x {ncol}, {len(cr)} entries"
    A = ctx.csc(nrow, ncol, cp, cr, cv)
    dx = ctx.vector_from(F.xp)
    for kernel in (AUTO, VECTOR, PANEL):
        A.set_kernel(kernel)
        F.check(ctx, A, f"{what}, kernel {kernel} (runs {A.info.kernel})", dx=dx)
        SEEN["csc"].add(A.info.kernel)
    for kernel in range(9):  # the CSR companion takes every CSR kernel id
        B = ctx.csc(nrow, ncol, cp, cr, cv)
        B.set_param("transpose_kernel", kernel)
        try:
            B.transpose_setup()
            T.check(ctx, B, f"{what}, transposed, companion kernel {kernel} (runs {B.get_param('transpose_kernel')})", transpose=True)
        except capi.SpmvError as err:
            # only these two are refused where the matrix does not fit them: the LDS window (too wide: at the product), the ELL copy
            assert kernel in (LDSWIN, ELLK) or not len(cr), (kernel, str(err))
            continue
        if len(cr):
            SEEN["csc^T"].add(B.get_param("transpose_kernel"))
    RUNS["csc"] += 1


# ---- ELL ----------------------------------------------------------------------------------------------------------------------
def _ell_shape(rng):
    """test_gpu_fuzz.py's ELL family: diagonal slots, padding (column 0, value 0) and noise"""
    nrow = int(rng.choice([1, 1024, 1026, 5000, 33_334, 120_000]))
    ncol = int(rng.choice([nrow, nrow + 77, max(64, nrow // 3), 4 * nrow]))
    k = int(rng.integers(1, 12))
    far = int(rng.choice([3, 200, 9000]))
    offs = np.sort(rng.choice(np.arange(-far, far + 1), size=k, replace=k > 2 * far + 1))
    rows = np.arange(nrow)
    col = rows[None, :] * ncol // nrow + offs[:, None] if rng.uniform() < 0.3 else rows[None, :] + offs[:, None]
    pad = np.zeros(col.shape, bool)
    if rng.uniform() < 0.5:
        col = col % ncol
    else:
        pad = (col < 0) | (col >= ncol)
        col[pad] = 0
    noise = rng.choice([0.0, 0.001, 0.2])
    bad = (rng.uniform(size=(k, nrow)) < noise) & ~pad
    col[bad] = rng.integers(0, ncol, int(bad.sum()))
    return nrow, ncol, k, col.astype(np.int32).ravel(), pad.ravel()


@pytest.mark.parametrize("seed", range(N_ELL))
def test_exact_ell_forward_and_transposed(ctx, pkg, seed):
    capi = pkg.capi
    rng = np.random.default_rng(BASE + 14_000 + seed)
    nrow, ncol, k, col, pad = _ell_shape(rng)
    ent = ex.ell_entries(nrow, k, col, np.zeros(len(col)))
    bits, e = _bits((ent[0], nrow), (ent[1], ncol))
    val = ex.dyadic(rng, len(col), bits, e)
    val[pad] = 0.0
    ent = ex.ell_entries(nrow, k, col, val)
    F = Exact(rng, nrow, ncol, ent, bits, e)  # every slot's column is read, padding's column 0 included
    T = Exact(rng, ncol, nrow, ex.transposed(ent), bits, e)
    what = f"seed {seed}: ELL {nrow} x {ncol}, k = {k}, {int(pad.sum())} pad slots"
    A = ctx.ell(nrow, ncol, k, int((~pad).sum()), col, val)
    dx = ctx.vector_from(F.xp)
    F.check(ctx, A, f"{what}, AUTO (kernel {A.info.kernel}, variant {A.get_param('ell_variant')})", dx=dx)
    SEEN["ell"].add(("auto", A.info.kernel))
    for lanes in (1, 2):
        A.set_kernel(VECTOR, lanes)
        for flags in (0, 8):
            A.set_flags(flags)
            F.check(ctx, A, f"{what}, lanes={lanes} flags={flags} (diagonal slots {A.get_param('ell_diagonal_slots')})", dx=dx)
            SEEN["ell"].add((lanes, flags))
    A.set_flags(0)
    if A.get_param("ell_diagonal_slots") == 1:
        try:
            A.set_param("ell_dia_order", 1)
        except capi.SpmvError:
            pass
        else:
            F.check(ctx, A, f"{what}, DIA-order copy ({A.get_param('ell_non_conforming_rows')} non-conforming rows)", dx=dx)
            SEEN["ell"].add("dia_order")
            A.set_param("ell_dia_order", 0)
    A.set_kernel(PANEL)
    F.check(ctx, A, f"{what}, PANEL (copy runs {A.get_param('rowgrouped_kernel')})", dx=dx)
    SEEN["ell"].add(("panel", A.info.kernel))
    for kernel in (AUTO, VECTOR, PANEL):  # ELL^T: no row without slots, so nothing of x is left unread
        B = ctx.ell(nrow, ncol, k, int((~pad).sum()), col, val)
        B.set_param("transpose_kernel", kernel)
        T.check(ctx, B, f"{what}, transposed, companion kernel {kernel}", transpose=True, dx=ctx.vector_from(T.x))
        SEEN["ell^T"].add(B.get_param("transpose_kernel"))
    RUNS["ell"] += 1


# ---- ELL: every launch the handle's settings can reach, on the smallest handles where each path can go wrong -----------------------
ELL_READ_COLUMNS = 8  # SPMV_FLAG_ELL_READ_COLUMNS
ELL_HOME_ROWS = (1024, 1536, 1025)  # the 4 * 256 floor of diagonal detection; one and a half tiles of 512 rows; odd: no descriptors
ELL_HOME_PATTERNS = ("tridiagonal", "eleven_far_diagonals", "tridiagonal_with_strays")


def _ell_home_shape(rng, nrow, pattern):
    """(ncol, k, offsets, col (k, nrow), pad (k, nrow)): slot s of row i holds column i + offsets[s]; a column outside the matrix
    is padding (column 0, value 0.0)"""
    if pattern == "eleven_far_diagonals":
        # more than 1024 apart: eleven clusters of 512 doubles, 5632 > the 5120-double cap, so no x windows
        offs, ncol = np.arange(11) * 1100, nrow + 10 * 1100 + 8
    else:
        offs, ncol = np.array([-1, 0, 1]), nrow
    col = np.arange(nrow)[None, :] + offs[:, None]
    pad = (col < 0) | (col >= ncol)
    col[pad] = 0
    if pattern == "tridiagonal_with_strays":  # about 1 % of the slots point elsewhere: rows for the side kernel, far fewer than 1/16
        stray = (rng.uniform(size=col.shape) < 0.01) & ~pad
        col[stray] = rng.integers(0, ncol, int(stray.sum()))
    return ncol, len(offs), offs, col, pad


@pytest.mark.parametrize("pattern", ELL_HOME_PATTERNS)
@pytest.mark.parametrize("nrow", ELL_HOME_ROWS)
def test_exact_ell_every_setting_launches_and_reports_as_before(ctx, pkg, nrow, pattern):
    """lanes_per_row (0, 1, 4, 8) x flags (0, read columns) x "ell_tiled_values" (0, 1) x "ell_dia_order" (0, 1) on ELL handles of
    1024, 1536 and 1025 rows whose slots are diagonals that fit the x windows, that exceed them, and that have stray columns:
    every product equals the exact reference bit for bit, and after every setting the handle reports what the rules of the
    engine say (written out here, not read off the code under test):
      * the slots are found to be diagonals on an even handle of 1024 rows and more (here every pattern conforms in far more than
        half of its row pairs), never on an odd one;
      * set_kernel(VECTOR) makes variant 0 run; "ell_dia_order" 1 builds the copy and makes variant 3 run - refused without
        diagonal slots - and 0 drops the copy; "ell_variant" says so whatever the flags are;
      * the tiled copy exists where it was asked for and the slots are diagonals; without them the request is a no-op;
      * the side kernel's rows are those with a slot off its diagonal, padding included;
      * with both copies dropped device_bytes is back where it began.
    These handles are below the size at which AUTO times anything: no trial takes part."""
    capi = pkg.capi
    rng = np.random.default_rng(BASE + 14_500 + 7 * nrow + ELL_HOME_PATTERNS.index(pattern))
    ncol, k, offs, col2, pad2 = _ell_home_shape(rng, nrow, pattern)
    col, pad = col2.astype(np.int32).ravel(), pad2.ravel()
    ent = ex.ell_entries(nrow, k, col, np.zeros(len(col)))
    bits, e = _bits((ent[0], nrow))
    val = ex.dyadic(rng, len(col), bits, e)
    val[pad] = 0.0
    F = Exact(rng, nrow, ncol, ex.ell_entries(nrow, k, col, val), bits, e)
    diagonal = nrow % 2 == 0 and nrow >= 1024
    off_diagonal_rows = int(np.any(col2 != np.arange(nrow)[None, :] + offs[:, None], axis=0).sum())
    assert 0 < off_diagonal_rows * 16 <= nrow or pattern == "eleven_far_diagonals" and off_diagonal_rows == 0
    what = f"ELL {nrow} x {ncol}, k = {k}, {pattern}"
    A = ctx.ell(nrow, ncol, k, int((~pad).sum()), col, val)
    dx = ctx.vector_from(F.xp)
    bytes0 = A.get_param("device_bytes")
    assert A.get_param("ell_diagonal_slots") == int(diagonal), what
    assert (A.info.kernel, A.get_param("ell_variant"), A.get_param("ell_tiled_values"), A.get_param("ell_dia_order")) == (VECTOR, 0, 0, 0), what
    F.check(ctx, A, f"{what}, as created", dx=dx)
    for lanes in (0, 1, 4, 8):
        for flags in (0, ELL_READ_COLUMNS):
            for tiled in (0, 1):
                for dia in (0, 1):
                    A.set_kernel(VECTOR, lanes)
                    assert A.get_param("ell_variant") == 0, what  # (a copy that was asked for stays; the variant does not)
                    A.set_flags(flags)
                    A.set_param("ell_tiled_values", tiled)
                    if dia and not diagonal:
                        with pytest.raises(capi.SpmvError, match="were not found to be diagonals"):
                            A.set_param("ell_dia_order", 1)
                        A.set_param("ell_dia_order", 0)
                        continue  # (refused: the setting does not exist on this handle)
                    A.set_param("ell_dia_order", dia)
                    now = f"{what}, lanes={lanes} flags={flags} tiled={tiled} dia_order={dia}"
                    F.check(ctx, A, now, dx=dx)
                    got = {n: A.get_param(n) for n in ("ell_variant", "ell_tiled_values", "ell_dia_order", "ell_non_conforming_rows", "ell_diagonal_slots")}
                    want = {"ell_variant": 3 if dia else 0, "ell_tiled_values": int(bool(tiled and diagonal)), "ell_dia_order": dia,
                            "ell_non_conforming_rows": off_diagonal_rows if dia else 0, "ell_diagonal_slots": int(diagonal)}
                    assert got == want and A.info.kernel == VECTOR, now
                    assert (A.get_param("device_bytes") > bytes0) == bool(dia or (tiled and diagonal)), now
    A.set_param("ell_tiled_values", 0)
    A.set_param("ell_dia_order", 0)
    assert A.get_param("device_bytes") == bytes0 and A.get_param("ell_variant") == 0, what
    A.set_flags(0)
    F.check(ctx, A, f"{what}, both copies dropped", dx=dx)


@pytest.mark.parametrize("nrow", ELL_HOME_ROWS)
def test_exact_ell_copy_of_a_csr_handle_leaves_its_padding_out(ctx, pkg, nrow):
    """the masked kernels: a tridiagonal CSR handle in which every eighth row (and the first and the last) holds k - 1 = 2 entries,
    forced onto its ELL copy.  The product is exact; the copy's slots are diagonals on an even handle (three of four row pairs
    conform in every slot), not on an odd one.  That the padding takes no part in the sums shows where x is not finite: a padding
    slot holds 0.0 and points at its row's own last column, so with x = inf there a row ends at +-inf, the sign of its stored entry,
    as in the reference's CSR loop - a kernel that multiplied the padding would add 0.0 * inf and end at NaN."""
    rng = np.random.default_rng(BASE + 14_600 + nrow)
    rows = np.arange(nrow)
    keep = np.stack([rows >= 1, np.ones(nrow, bool), (rows + 1 < nrow) & (rows % 8 != 3)], axis=1)  # columns i - 1, i, i + 1
    lens = keep.sum(axis=1)
    assert set(lens.tolist()) == {2, 3}
    row_ptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
    col = (rows[:, None] + np.array([-1, 0, 1])[None, :])[keep].astype(np.int32)
    ent = ex.csr_entries(row_ptr, col, np.zeros(len(col)))
    bits, e = _bits((ent[0], nrow))
    val = ex.dyadic(rng, len(col), bits, e)
    F = Exact(rng, nrow, nrow, ex.csr_entries(row_ptr, col, val), bits, e)
    A = ctx.csr(nrow, nrow, row_ptr, col, val)
    A.set_kernel(ELLK)
    what = f"CSR {nrow} x {nrow}, rows of 2 and 3 entries, ELL copy"
    assert A.info.kernel == ELLK and A.get_param("ell_copy_slots") == 3 * nrow, what
    assert A.get_param("ell_copy_diagonal_slots") == int(nrow % 2 == 0) and A.get_param("ell_copy_variant") == 0, what
    F.check(ctx, A, what)
    short = np.flatnonzero(lens == 2)[1:-1:5]  # short rows (i % 8 == 3): their last column is i, which rows i - 1, i, i + 1 read
    x_inf = F.x.copy()
    x_inf[short] = np.inf
    want = F.want1.copy()
    for j in short:
        for i in (j - 1, j, j + 1):  # (one inf per row: the short rows are eight apart)
            want[i] = np.inf * np.sign(val[row_ptr[i] + int(np.flatnonzero(col[row_ptr[i]:row_ptr[i + 1]] == j)[0])])
    dy = ctx.vector_from(F.y0)
    ctx.apply(A, ctx.vector_from(x_inf), dy)
    ctx.sync()
    got = dy.download()
    assert len(short) >= 20 and np.array_equal(got, want), f"{what}, x = inf at the last column of {len(short)} short rows: {_fail(got, want)}"


def test_ell_transposed_carries_inf_through_padding_as_nan(ctx, orc):
    """an inf in x at a padded row reaches y[pad column] as NaN under every companion kernel (0.0 * inf), as the slot-list oracle
    says"""
    rng = np.random.default_rng(BASE + 14_900)
    nrow, ncol, k = 3000, 2500, 5
    col = rng.integers(1, ncol, (k, nrow))
    val = rng.uniform(-1, 1, (k, nrow))
    short = rng.random(nrow) < 0.3
    col[3:, short], val[3:, short] = 0, 0.0  # rows of 3 entries: two pad slots at column 0
    col, val = ol.i32(col.ravel()), ol.f64(val.ravel())
    slot_rows = ol.i32(np.tile(np.arange(nrow, dtype=np.int32), k))
    x = rng.uniform(-1, 1, nrow)
    x[np.flatnonzero(short)[::7]] = np.inf
    y0 = rng.uniform(-1, 1, ncol)
    ref = y0.copy()
    ol.coo_spmv(orc, col, slot_rows, val, x, ref, fma=True)
    assert np.isnan(ref[0])
    for kernel in (AUTO, VECTOR, PANEL):
        A = ctx.ell(nrow, ncol, k, int((val != 0).sum()), col, val)
        A.set_param("transpose_kernel", kernel)
        dy = ctx.vector_from(y0)
        ctx.apply_transpose(A, ctx.vector_from(x), dy)
        ctx.sync()
        got = dy.download()
        assert np.isnan(got[0]), kernel
        assert np.array_equal(np.isfinite(got), np.isfinite(ref)), kernel
        fin = np.isfinite(ref)
        scale = np.zeros(ncol)
        ol.coo_spmv(orc, col, slot_rows, np.abs(val), np.where(np.isfinite(x), np.abs(x), 0.0), scale)
        ol.assert_parity(got[fin], ref[fin], scale[fin] + np.abs(y0[fin]), f"ELL^T kernel {kernel}, finite outputs")


# ---- DIA ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(N_DIA))
def test_exact_dia_forward_and_transposed(ctx, pkg, seed):
    rng = np.random.default_rng(BASE + 15_000 + seed)
    nrow = int(rng.choice([1, 255, 256, 257, 5000, 70_001]))
    ncol = int(rng.choice([nrow, max(1, nrow // 2), nrow + 300, 3 * nrow]))
    nd = int(rng.integers(1, 20))
    span = int(rng.choice([2, 40, 900, max(2, nrow)]))
    offs = ol.i32(np.sort(rng.choice(np.arange(-span, span + 1), size=min(nd, 2 * span + 1), replace=False)))
    if rng.random() < 0.3:
        offs = ol.i32(offs[::-1].copy())  # slot order need not be sorted
    bound = 0
    if seed % 3 == 2 and ncol > 2:  # a row shard's column bound: the whole matrix's
        bound = int(rng.integers(1, ncol + 1))
    fwd = ex.dia_entries(nrow, ncol, offs, np.zeros(nrow * len(offs)), bound)
    bits, e = _bits((fwd[0], nrow), (fwd[1], ncol))
    val = ex.dyadic(rng, nrow * len(offs), bits, e)
    fwd = ex.dia_entries(nrow, ncol, offs, val, bound)
    F = Exact(rng, nrow, ncol, fwd, bits, e)
    T = Exact(rng, ncol, nrow, ex.transposed(fwd), bits, e)
    what = f"seed {seed}: DIA {nrow} x {ncol}, offsets {list(offs)[:8]}.., bound {bound}"
    A = ctx.dia(nrow, ncol, offs, val)
    if bound:
        A.set_param("dia_col_bound", bound)
    dx = ctx.vector_from(F.xp)
    for flags in (0, 4):  # 4: x from global memory
        A.set_flags(flags)
        F.check(ctx, A, f"{what}, flags {flags}", dx=dx)
    T.check(ctx, A, f"{what}, transposed", transpose=True)
    spread = max((int(offs[i:i + 16].max()) - int(offs[i:i + 16].min()) for i in range(0, len(offs), 16)), default=0)
    SEEN["dia^T"].add("tiled" if spread <= 64 else "general")
    SEEN["dia"].add("bound" if bound else "plain")
    RUNS["dia"] += 1


# ---- wrapped handles ----------------------------------------------------------------------------------------------------------
def _device_ints(ctx, a):
    """int32 array bytes in a Vector's device memory (Vector holds float64 words: the bytes travel as they are)"""
    a = np.ascontiguousarray(a, dtype=np.int32)
    buf = np.zeros(2 * ((a.size + 1) // 2), np.int32)
    buf[: a.size] = a
    v = ctx.vector(max(1, buf.size // 2))
    if buf.size:
        v.upload(buf.view(np.float64))
    return v


def test_exact_wrapped_coo_and_ell_handles(ctx, pkg):
    rng = np.random.default_rng(BASE + 16_000)
    nrow, ncol, nnz = 20_000, 15_000, 120_000
    row = rng.integers(0, nrow, nnz).astype(np.int32)
    col = ex.avoid_columns(rng.integers(0, ncol, nnz), ncol, PANEL_COLS)
    bits, e = _bits((row, nrow), (col, ncol))
    val = ex.dyadic(rng, nnz, bits, e)
    ent = ex.coo_entries(row, col, val)
    keep = []
    dr, dc, dv = _device_ints(ctx, row), _device_ints(ctx, col), ctx.vector_from(val)
    A = ctx.wrap_coo(nrow, ncol, nnz, dr.device_ptr, dc.device_ptr, dv.device_ptr)
    keep += [dr, dc, dv]
    Exact(rng, nrow, ncol, ent, bits, e).check(ctx, A, "wrap_coo forward")
    Exact(rng, ncol, nrow, ex.transposed(ent), bits, e).check(ctx, A, "wrap_coo transposed", transpose=True)
    # ELL: rows of 1..9 slots, padded with column 0 / value 0
    k = 9
    lens = rng.integers(1, k + 1, nrow)
    ec = ex.avoid_columns(rng.integers(0, ncol, (k, nrow)), ncol, PANEL_COLS).reshape(k, nrow)
    pad = np.arange(k)[:, None] >= lens[None, :]
    ec[pad] = 0
    ent = ex.ell_entries(nrow, k, ec.ravel(), np.zeros(k * nrow))
    bits, e = _bits((ent[0], nrow), (ent[1], ncol))
    ev = ex.dyadic(rng, (k, nrow), bits, e)
    ev[pad] = 0.0
    ec, ev = ec.ravel(), ev.ravel()
    ent = ex.ell_entries(nrow, k, ec, ev)
    dc2, dv2 = _device_ints(ctx, ec), ctx.vector_from(ev)
    E = ctx.wrap_ell(nrow, ncol, k, int(lens.sum()), dc2.device_ptr, dv2.device_ptr)
    keep += [dc2, dv2]
    Exact(rng, nrow, ncol, ent, bits, e).check(ctx, E, "wrap_ell forward")
    T = Exact(rng, ncol, nrow, ex.transposed(ent), bits, e)
    T.check(ctx, E, "wrap_ell transposed", transpose=True, dx=ctx.vector_from(T.x))
    _check_multi(ctx, E, rng, nrow, ncol, ent, ent[1], (5, 17), "wrap_ell multi", bits, e)
    SEEN["wrapped"].update({"coo", "ell"})


# ---- the multi-vector product -------------------------------------------------------------------------------------------------
KS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64)


def _check_multi(ctx, A, rng, nrow, ncol, ent, used, ks, what, bits, e):
    """Y += A X (Y = A X with overwrite, Y filled with NaN before) on dyadic X (the values' grid: bits, e) whose unread rows are
    poison: exact, 1 and REPS calls"""
    for k in ks:
        X = ex.dyadic(rng, (ncol, k), bits, e)
        Y0 = ex.dyadic(rng, (nrow, k), bits, e)
        want1 = ex.exact_multi(nrow, *ent, X, e, Y0=Y0)
        wantr = ex.exact_multi(nrow, *ent, X, e, Y0=Y0, reps=REPS)
        want0 = ex.exact_multi(nrow, *ent, X, e)
        Xp = ex.poison(X.ravel(), (np.unique(np.asarray(used, np.int64))[:, None] * k + np.arange(k)[None, :]).ravel()).reshape(ncol, k)
        dX = ctx.vector_from(Xp.ravel())
        for overwrite in (False, True):
            dY = ctx.vector(nrow * k)
            if overwrite:
                dY.fill(np.nan)  # Y is not read
            else:
                dY.upload(Y0.ravel())
            for call in range(REPS):
                ctx.apply_multi(A, dX, dY, k, overwrite=overwrite)
                if call == 0:
                    ctx.sync()
                    got = dY.download().reshape(nrow, k)
                    want = want0 if overwrite else want1
                    assert np.array_equal(got, want), f"{what} k={k} overwrite={overwrite}, 1 call: {_fail(got.ravel(), want.ravel())}"
            ctx.sync()
            got = dY.download().reshape(nrow, k)
            want = want0 if overwrite else wantr
            assert np.array_equal(got, want), f"{what} k={k} overwrite={overwrite}, {REPS} calls: {_fail(got.ravel(), want.ravel())}"
        SEEN["multi:k"].add(k)


@pytest.mark.parametrize("seed", range(N_MULTI))
def test_exact_multi_csr_and_ell_every_tile_boundary(ctx, pkg, seed):
    """CSR and ELL handles on the CSR fuzz shapes (their first rows, up to 300K entries), every k across the tile boundaries"""
    nrow, ncol, rp, cc = _csr_shape(seed)
    r1 = int(np.searchsorted(rp, 300_000, side="right")) - 1
    if r1 < nrow:
        nrow, rp, cc = max(r1, 1), rp[: max(r1, 1) + 1].copy(), cc[: rp[max(r1, 1)]].copy()
    rng = np.random.default_rng(BASE + 17_000 + seed)
    if seed % 3 == 0:
        cc = ex.avoid_columns(cc, ncol, PANEL_COLS)
    lens = np.diff(rp)
    bits, e = ex.choose_bits(int(lens.max(initial=0)), REPS)
    cv = ex.dyadic(rng, len(cc), bits, e)
    ent = ex.csr_entries(rp, cc, cv)
    A = ctx.csr(nrow, ncol, rp, cc, cv)
    _check_multi(ctx, A, rng, nrow, ncol, ent, cc, KS, f"seed {seed}: CSR {nrow} x {ncol} multi", bits, e)
    SEEN["multi"].add("csr")
    k = int(lens.max(initial=0))
    if k and nrow * k <= 4_000_000:
        slot = np.arange(len(cc)) - np.repeat(rp[:-1].astype(np.int64), lens)
        ec, ev = np.zeros((k, nrow), np.int32), np.zeros((k, nrow))
        rows = np.repeat(np.arange(nrow), lens)
        ec[slot, rows], ev[slot, rows] = cc, cv
        ec, ev = ec.ravel(), ev.ravel()
        E = ctx.ell(nrow, ncol, k, len(cc), ec, ev)
        ent = ex.ell_entries(nrow, k, ec, ev)
        _check_multi(ctx, E, rng, nrow, ncol, ent, ec, KS, f"seed {seed}: ELL {nrow} x {ncol}, {k} slots, multi", bits, e)
        SEEN["multi"].add("ell")
    RUNS["multi"] += 1


def spmm_lanes(k, cap=16):
    """kernels_spmm.hip spmm_lanes: the next power of two >= k, at most the cap (16; SPMV_SPMM_LANES = 32 or 64)"""
    t = 1
    while t < k and t < cap:
        t *= 2
    return t


def spmm_virtual_blocks(nrow, k, T, csr=True):
    """kernels_spmm.hip spmm_shape: ceil(nrow / rows per workgroup) x column tiles (CSR: groups of max(T, 8) lanes; ELL: T)"""
    rows = 256 // (max(T, 8) if csr else T)
    return -(-nrow // rows) * -(-k // T)


def grid_stride_case(ctx, cap):
    """~4.5M rows of 2-3 entries, 800 columns, k = 64: more than 2^20 virtual blocks, so the kernels loop.  Sampled rows (the first,
    both sides of the first sweep's end, the last) against the exact product; CSR and ELL.  Returns the virtual-block counts."""
    nrow, ncol, k = 4_500_000, 800, 64
    T = spmm_lanes(k, cap)
    rng = np.random.default_rng(BASE + 18_000 + cap)
    lens = 2 + (rng.random(nrow) < 0.5)
    rp = np.zeros(nrow + 1, np.int64)
    rp[1:] = np.cumsum(lens)
    cc = rng.integers(0, ncol, int(rp[-1])).astype(np.int32)
    bits, e = ex.choose_bits(3, 1)
    cv = ex.dyadic(rng, len(cc), bits, e)
    X = ex.dyadic(rng, (ncol, k), bits, e)
    dX = ctx.vector_from(X.ravel())
    y0 = 0.25
    out = {}
    for fmt in ("csr", "ell"):
        if fmt == "csr":
            A = ctx.csr(nrow, ncol, rp.astype(np.int32), cc, cv)
            rows_per = 256 // max(T, 8)
        else:
            ec, ev = np.zeros((3, nrow), np.int32), np.zeros((3, nrow))
            slot = np.arange(len(cc)) - np.repeat(rp[:-1], lens)
            rr = np.repeat(np.arange(nrow), lens)
            ec[slot, rr], ev[slot, rr] = cc, cv
            A = ctx.ell(nrow, ncol, 3, len(cc), ec.ravel(), ev.ravel())
            rows_per = 256 // T
            del slot, rr
        nvb = spmm_virtual_blocks(nrow, k, T, csr=fmt == "csr")
        assert nvb > (1 << 20), nvb
        sweep = (1 << 20) // -(-k // T) * rows_per  # rows the first sweep of 2^20 workgroups covers
        dY = ctx.vector(nrow * k)
        dY.fill(y0)
        ctx.apply_multi(A, dX, dY, k)
        ctx.sync()
        for r0 in (0, sweep - 40, nrow - 80):
            got = dY.download(int(r0) * k, 80 * k).reshape(80, k)
            b, en = rp[r0], rp[r0 + 80]
            sub_rows = np.repeat(np.arange(80), lens[r0:r0 + 80])
            want = ex.exact_multi(80, sub_rows, cc[b:en], cv[b:en], X, e, Y0=np.full((80, k), y0))  # (ELL padding: 0.0 * X[0, c])
            assert np.array_equal(got, want), f"{fmt} T={T}: rows {r0}..{r0 + 80}: {_fail(got.ravel(), want.ravel())}"
        out[fmt] = nvb
        del A, dY
    return T, out


def test_exact_multi_grid_stride_loop(ctx):
    T, nvb = grid_stride_case(ctx, 16)
    assert T == 16
    SEEN["multi:grid_stride"].add(T)


@pytest.mark.parametrize("lanes", ["32", "64"])
def test_exact_multi_wide_lane_groups_in_a_child(lanes):
    """SPMV_SPMM_LANES = 32 / 64 is read once per process: tests/child_spmm_lanes.py runs the exact multi checks for k = 17..64 (and,
    with 64 lanes, the grid-stride case) in a fresh process"""
    child = Path(__file__).with_name("child_spmm_lanes.py")
    env = dict(os.environ, SPMV_SPMM_LANES=lanes, SPMV_FUZZ_BASE=str(BASE))
    r = subprocess.run([sys.executable, str(child)], capture_output=True, text=True, timeout=420, env=env)
    assert r.returncode == 0 and f"SPMM_LANES_OK {lanes}" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    seen = {int(t) for line in r.stdout.splitlines() if line.startswith("T=") for t in [line.split()[0][2:]]}
    assert int(lanes) in seen, seen
    if lanes == "64":
        assert "grid-stride" in r.stdout, r.stdout[-2000:]
    SEEN["multi:lanes"].update(seen)


# ---- full size (U(-1,1) values: the parity gate) ------------------------------------------------------------------------------
def _adjoint(ctx, A, n_rows, n_cols, x, w, max_row, max_col, amax, what):
    """w . (A x) against (A^T w) . x over the whole vectors; the bound: every product's rounding over the longest row / column"""
    y, z = ctx.vector(n_rows), ctx.vector(n_cols)
    y.fill(0.0)
    z.fill(0.0)
    ctx.apply(A, x, y)
    ctx.apply_transpose(A, w, z)
    ctx.sync()
    a, b = ctx.dot(w, y), ctx.dot(z, x)
    xmax, wmax = float(np.max(np.abs(x.download()))), float(np.max(np.abs(w.download())))
    nnz = A.info.nnz if A.info.format != 3 else A.info.nrow * A.info.ell_k
    tol = (max_row + max_col + 2 * np.log2(max(n_rows, n_cols)) + 4) * 2.0**-52 * nnz * amax * xmax * wmax
    assert abs(a - b) <= tol, f"{what}: w.(Ax) = {a!r}, (A^T w).x = {b!r}, |diff| {abs(a - b):.3e} > {tol:.3e}"


def test_full_size_c3_ell_and_c4_coo_transposed(ctx, orc, pkg):
    """C3 (ELL 4M x 64 circulant band) and C4 (COO 2M power-law) transposed under AUTO and each companion kernel: sampled outputs
    against the host twins of the generators, and the adjoint identity over the whole vectors"""
    synth = pkg.synth
    n, k = 4_000_000, 64
    key = synth.stream_key(1, synth.STREAM_VAL)
    x = ctx.gen_vector(n, seed=11)
    hx = synth.vec_uniform(n, seed=11)
    js = np.unique(np.concatenate([np.arange(2000), np.arange(1_777_000, 1_779_000), np.arange(n - 2000, n)]))
    # C3: output j reads rows i = (j - d + k/2) mod n, value index i * k + d
    d = np.arange(k, dtype=np.int64)
    I = (js[:, None] - d[None, :] + k // 2) % n
    V = synth.to_sym(synth._draw(key, (I * k + d[None, :]).astype(np.uint64).ravel())).reshape(I.shape)
    ref = (V * hx[I]).sum(axis=1)
    scale = (np.abs(V) * hx[I]).sum(axis=1)
    for kernel in (AUTO, VECTOR, PANEL):
        E = ctx.gen_ell_banded(n, n, k, seed=1)
        E.set_param("transpose_kernel", kernel)
        y = ctx.vector(n)
        y.fill(0.0)
        ctx.apply_transpose(E, x, y)
        ctx.sync()
        got = y.download()
        ol.assert_parity(got[js], ref, scale, f"C3 transposed, companion kernel {kernel} (runs {E.get_param('transpose_kernel')})")
        SEEN["full:c3^T"].add(E.get_param("transpose_kernel"))
        if kernel == AUTO:
            _adjoint(ctx, E, n, n, x, ctx.gen_vector(n, seed=12), k, k, 1.0, "C3")
        del E, y
    # C4: the entries whose column is sampled, regenerated in row chunks
    n, max_len = 2_000_000, 4096
    lens = synth.powerlaw_lengths(n, max_len, 1).astype(np.int64)
    kc = synth.stream_key(1, synth.STREAM_COL)
    want = np.zeros(n, bool)
    js = np.unique(np.concatenate([np.arange(1500), np.arange(999_000, 1_000_500), np.arange(n - 1500, n)]))
    want[js] = True
    rows_k, cols_k, gidx_k = [], [], []
    start = np.concatenate(([0], np.cumsum(lens)))
    for r0 in range(0, n, 250_000):
        r1 = min(n, r0 + 250_000)
        ln = lens[r0:r1]
        rr = np.repeat(np.arange(r0, r1, dtype=np.int64), ln)
        s = np.arange(rr.size, dtype=np.int64) - np.repeat(start[r0:r1] - start[r0], ln)
        g = (rr * max_len + s).astype(np.uint64)
        cc = synth.to_range(synth._draw(kc, g), n)
        m = want[cc]
        rows_k.append(rr[m])
        cols_k.append(cc[m])
        gidx_k.append(g[m])
    rr, cc, g = np.concatenate(rows_k), np.concatenate(cols_k), np.concatenate(gidx_k)
    vv = synth.to_sym(synth._draw(key, g))
    hx = synth.vec_uniform(n, seed=11)
    pos = ol.i32(np.searchsorted(js, cc))
    ref, scale = np.zeros(len(js)), np.zeros(len(js))
    ol.coo_spmv(orc, pos, ol.i32(rr), ol.f64(vv), hx[: n], ref)
    ol.coo_spmv(orc, pos, ol.i32(rr), np.abs(ol.f64(vv)), hx[: n], scale)
    x = ctx.gen_vector(n, seed=11)
    max_col = int(np.bincount(cc, minlength=1).max())
    for kernel in (AUTO, VECTOR, PANEL):
        P = ctx.gen_coo_powerlaw(n, n, max_len, seed=1)
        P.set_param("transpose_kernel", kernel)
        y = ctx.vector(n)
        y.fill(0.0)
        ctx.apply_transpose(P, x, y)
        ctx.sync()
        got = y.download()
        ol.assert_parity(got[js], ref, scale, f"C4 transposed, companion kernel {kernel} (runs {P.get_param('transpose_kernel')})")
        SEEN["full:c4^T"].add(P.get_param("transpose_kernel"))
        if kernel == AUTO:
            _adjoint(ctx, P, n, n, x, ctx.gen_vector(n, seed=12), int(lens.max()), max(max_col, 64), 1.0, "C4")
        del P, y


def test_full_size_c3_multi_k8_equals_the_ell_kernel_per_column(ctx):
    """C3 at k = 8: every column of apply_multi equals spmv_apply of the handle's own ELL kernel (one row per lane, slot order)
    on that column, bit for bit"""
    n, k = 4_000_000, 8
    E = ctx.gen_ell_banded(n, n, 64, seed=1)
    X = ctx.gen_vector(n * k, seed=21)
    Y0 = ctx.gen_vector(n * k, seed=22)
    Y = ctx.vector(n * k)
    Y.copy_from(Y0, n * k)
    ctx.apply_multi(E, X, Y, k)
    ctx.sync()
    got = Y.download().reshape(n, k)
    hX, hY0 = X.download().reshape(n, k), Y0.download().reshape(n, k)
    E.set_kernel(VECTOR, 1)
    for c in range(k):
        xc, yc = ctx.vector_from(np.ascontiguousarray(hX[:, c])), ctx.vector_from(np.ascontiguousarray(hY0[:, c]))
        ctx.apply(E, xc, yc)
        ctx.sync()
        assert np.array_equal(got[:, c], yc.download()), f"C3 k=8: column {c}"
    SEEN["full:c3 multi"].add(k)


# ---- overwrite and the fused dot product (spmv_apply_dot) -----------------------------------------------------------------------
# kernels_csr.hip: the kernels that take y = A x and w . y into their own write-back (SPLIT: into the kernel of its short rows,
# the dot behind); every other kernel runs behind a fill of y and in front of a dot pass
FUSES = {AUTO, VECTOR, PANEL, TWOPHASE, SPLIT}
EXTRAS_SEEDS = tuple(range(6)) + tuple(range(6, N_CSR, 2))  # the six edge shapes and every other random shape


def _vec(ctx, a):
    a = np.asarray(a, dtype=np.float64)
    return ctx.vector_from(a) if a.size else ctx.vector(0)


class ExactDot:
    """Exact with a dyadic w: y = A x over a y that is NaN / +-inf everywhere, y0 + A x once and REPS times, and w . y of each -
    all from integer arithmetic (the bits of choose_bits_dot keep the whole dot within 2^53)"""

    def __init__(self, rng, nout, nin, entries, bits, e, used=None):
        self.nout, self.e = nout, e
        self.x, self.y0, self.w = ex.dyadic(rng, nin, bits, e), ex.dyadic(rng, nout, bits, e), ex.dyadic(rng, nout, bits, e)
        self.want0 = ex.exact_product(nout, *entries, self.x, e)
        self.want1 = ex.exact_product(nout, *entries, self.x, e, y0=self.y0)
        self.wantr = ex.exact_product(nout, *entries, self.x, e, y0=self.y0, reps=REPS)
        self.dot0, self.dot1, self.dotr = (ex.exact_dot(self.w, y, e, 2 * e) for y in (self.want0, self.want1, self.wantr))
        self.xp = ex.poison(self.x, entries[1] if used is None else used)
        self.poisoned_y = ex.poison(np.zeros(nout), [])  # overwrite must not read it

    def check(self, ctx, A, what, dx=None, dw=None):
        dx = dx if dx is not None else _vec(ctx, self.xp)
        dw = dw if dw is not None else _vec(ctx, self.w)
        dy = _vec(ctx, self.poisoned_y)
        for call in range(2):  # y = A x twice: the second call must not add to the first
            d = ctx.apply_dot(A, dx, dy, dw, overwrite=True)
            got = dy.download()
            assert np.array_equal(got, self.want0), f"{what}, overwrite (call {call + 1}) onto NaN / inf: {_fail(got, self.want0)}"
            assert d == self.dot0, f"{what}, overwrite (call {call + 1}): w . y = {d!r}, exact {self.dot0!r}"
        dy = _vec(ctx, self.y0)
        for call in range(REPS):
            d = ctx.apply_dot(A, dx, dy, dw, overwrite=False)
            if call in (0, REPS - 1):
                want, wdot = (self.want1, self.dot1) if call == 0 else (self.wantr, self.dotr)
                got = dy.download()
                assert np.array_equal(got, want), f"{what}, y += A x, {call + 1} calls: {_fail(got, want)}"
                assert d == wdot, f"{what}, y += A x, {call + 1} calls: w . y = {d!r}, exact {wdot!r}"


@pytest.mark.parametrize("seed", EXTRAS_SEEDS)
def test_exact_apply_dot_every_kernel(ctx, pkg, seed):
    """spmv_apply_dot under every CSR kernel and parameter set of the forward test: y = A x over a y of NaN / +-inf (empty rows come
    back as 0), y0 + A x once and REPS times, and the dot w . y of each, all bit for bit"""
    capi = pkg.capi
    nrow, ncol, rp, cc = _csr_shape(seed)
    rng = np.random.default_rng(BASE + 19_000 + seed)
    if seed % 3 == 0:
        cc = ex.avoid_columns(cc, ncol, PANEL_COLS)
    bits, e = ex.choose_bits_dot(len(cc), nrow, REPS)
    cv = _dyadic_values(rng, len(cc), bits, e, zeros=seed % 4 == 1)
    D = ExactDot(rng, nrow, ncol, ex.csr_entries(rp, cc, cv), bits, e)
    empty = np.diff(rp) == 0
    assert np.all(D.want0[empty] == 0.0)
    what = f"seed {seed}: CSR {nrow} x {ncol}, {len(cc)} entries, {int(empty.sum())} empty rows"
    A = ctx.csr(nrow, ncol, rp, cc, cv)
    dx, dw = _vec(ctx, D.xp), _vec(ctx, D.w)
    for label, setup in _csr_kernel_runs(capi, A, rng, len(cc), ncol):
        if setup() is False:
            continue
        k = A.info.kernel
        D.check(ctx, A, f"{what}, {label} (kernel {k})", dx=dx, dw=dw)
        _record_csr(A, label, family="extras")
        SEEN["extras"].add(AUTO if label == "auto" else k)
        SEEN["extras:path"].add("fused" if (AUTO if label == "auto" else k) in FUSES else "behind")
        if empty.any():
            SEEN["extras:empty_rows"].add(AUTO if label == "auto" else k)
    RUNS["extras"] += 1


@pytest.mark.parametrize("seed", range(5))
def test_exact_apply_dot_coo_csc_ell_dia_handles(ctx, pkg, seed):
    """the same for the other formats: their own kernels (no extras of their own: fill, product, dot pass) and their row-grouped
    copies (a CSR handle, whose kernel takes the extras)"""
    capi = pkg.capi
    rng = np.random.default_rng(BASE + 19_500 + seed)
    # COO
    nrow, ncol, row, col = _coo_shape(rng, seed)
    bits, e = ex.choose_bits_dot(len(row), nrow, REPS)
    val = _dyadic_values(rng, len(row), bits, e, zeros=seed % 4 == 1)
    D = ExactDot(rng, nrow, ncol, ex.coo_entries(row, col, val), bits, e)
    A = ctx.coo(nrow, ncol, row, col, val)
    for kernel in (AUTO, VECTOR, PANEL):
        A.set_kernel(kernel)
        D.check(ctx, A, f"seed {seed}: COO {nrow} x {ncol}, {len(row)} entries, kernel {kernel} (runs {A.info.kernel})")
        SEEN["extras:coo"].add(A.info.kernel)
    # CSC
    nrow, ncol, cp, cols, cr = _csc_shape(rng, seed)
    bits, e = ex.choose_bits_dot(len(cr), nrow, REPS)
    cv = _dyadic_values(rng, len(cr), bits, e, zeros=seed % 4 == 1)
    D = ExactDot(rng, nrow, ncol, ex.csc_entries(cp, cr, cv), bits, e)
    A = ctx.csc(nrow, ncol, cp, cr, cv)
    for kernel in (AUTO, VECTOR, PANEL):
        A.set_kernel(kernel)
        D.check(ctx, A, f"seed {seed}: CSC {nrow} x {ncol}, {len(cr)} entries, kernel {kernel} (runs {A.info.kernel})")
        SEEN["extras:csc"].add(A.info.kernel)
    # ELL: pad products count as reads (0.0 * x[0])
    nrow, ncol, k, col, pad = _ell_shape(rng)
    bits, e = ex.choose_bits_dot(len(col), nrow, REPS)
    val = ex.dyadic(rng, len(col), bits, e)
    val[pad] = 0.0
    D = ExactDot(rng, nrow, ncol, ex.ell_entries(nrow, k, col, val), bits, e)
    A = ctx.ell(nrow, ncol, k, int((~pad).sum()), col, val)
    for kernel, lanes in ((AUTO, 0), (VECTOR, 1), (VECTOR, 2), (PANEL, 0)):
        if kernel != AUTO:  # (AUTO: the handle as created)
            A.set_kernel(kernel, lanes)
        D.check(ctx, A, f"seed {seed}: ELL {nrow} x {ncol}, k = {k}, {int(pad.sum())} pad slots, kernel {kernel} lanes {lanes} (runs {A.info.kernel})")
        SEEN["extras:ell"].add(A.info.kernel)
    # DIA
    nrow = int(rng.choice([1, 255, 257, 5000, 70_001]))
    ncol = int(rng.choice([nrow, max(1, nrow // 2), nrow + 300]))
    span = int(rng.choice([2, 40, max(2, nrow)]))
    offs = ol.i32(np.sort(rng.choice(np.arange(-span, span + 1), size=min(int(rng.integers(1, 20)), 2 * span + 1), replace=False)))
    bits, e = ex.choose_bits_dot(nrow * len(offs), nrow, REPS)
    val = ex.dyadic(rng, nrow * len(offs), bits, e)
    D = ExactDot(rng, nrow, ncol, ex.dia_entries(nrow, ncol, offs, val), bits, e)
    A = ctx.dia(nrow, ncol, offs, val)
    D.check(ctx, A, f"seed {seed}: DIA {nrow} x {ncol}, offsets {list(offs)[:8]}..")
    SEEN["extras:dia"].add("plain")
    RUNS["extras:formats"] += 1


def test_exact_apply_dot_wrapped_and_degenerate_handles(ctx, pkg):
    """borrowed arrays (COO, ELL); no entries in nrow > 0 rows (y = 0 over NaN, dot 0); no rows; an ELL handle that is all padding;
    a ragged ELL handle whose extras go to its row-grouped copy"""
    rng = np.random.default_rng(BASE + 19_900)
    nrow, ncol, nnz = 20_000, 15_000, 120_000
    row = rng.integers(0, nrow, nnz).astype(np.int32)
    col = ex.avoid_columns(rng.integers(0, ncol, nnz), ncol, PANEL_COLS)
    bits, e = ex.choose_bits_dot(nnz, nrow, REPS)
    val = ex.dyadic(rng, nnz, bits, e)
    dr, dc, dv = _device_ints(ctx, row), _device_ints(ctx, col), ctx.vector_from(val)
    A = ctx.wrap_coo(nrow, ncol, nnz, dr.device_ptr, dc.device_ptr, dv.device_ptr)
    ExactDot(rng, nrow, ncol, ex.coo_entries(row, col, val), bits, e).check(ctx, A, "wrap_coo")
    # ragged ELL, borrowed: rows of 1..9 slots padded with column 0 / value 0; then the same handle from its row-grouped copy
    k = 9
    lens = rng.integers(1, k + 1, nrow)
    ec = ex.avoid_columns(rng.integers(0, ncol, (k, nrow)), ncol, PANEL_COLS).reshape(k, nrow)
    pad = np.arange(k)[:, None] >= lens[None, :]
    ec[pad] = 0
    bits, e = ex.choose_bits_dot(k * nrow, nrow, REPS)
    ev = ex.dyadic(rng, (k, nrow), bits, e)
    ev[pad] = 0.0
    ec, ev = ec.ravel(), ev.ravel()
    ent = ex.ell_entries(nrow, k, ec, ev)
    dc2, dv2 = _device_ints(ctx, ec), ctx.vector_from(ev)
    E = ctx.wrap_ell(nrow, ncol, k, int(lens.sum()), dc2.device_ptr, dv2.device_ptr)
    D = ExactDot(rng, nrow, ncol, ent, bits, e)
    D.check(ctx, E, "wrap_ell")
    E2 = ctx.ell(nrow, ncol, k, int(lens.sum()), ec, ev)
    E2.set_kernel(PANEL)
    assert E2.info.kernel == PANEL and E2.get_param("rowgrouped_kernel") >= 0
    D.check(ctx, E2, f"ragged ELL from its row-grouped copy (kernel {E2.get_param('rowgrouped_kernel')})")
    SEEN["extras:wrapped"].update({"coo", "ell", "ell copy"})
    # rows without a single entry: y = 0 over NaN, w . y = 0; y += A x leaves y0 and returns w . y0
    i0, f0 = np.zeros(0, np.int32), np.zeros(0)
    nrow, ncol = 777, 50
    none = (np.zeros(0, np.int64), np.zeros(0, np.int64), f0)
    D = ExactDot(rng, nrow, ncol, none, 6, 4)
    assert D.dot0 == 0.0 and not D.want0.any() and not np.isfinite(D.xp).any()
    C = ctx.csr(nrow, ncol, np.zeros(nrow + 1, np.int32), i0, f0)
    for kernel in (AUTO, VECTOR, SCALAR, PANEL, TWOPHASE, SEGSCAN, SPLIT):
        try:
            C.set_kernel(kernel)
        except pkg.capi.SpmvError:
            continue  # a kernel that needs entries to build its layout says so; what can be selected must be right
        D.check(ctx, C, f"CSR {nrow} x {ncol} without entries, kernel {kernel} (runs {C.info.kernel})")
        SEEN["extras:no_entries"].add(C.info.kernel)
    for name, H in (("COO", ctx.coo(nrow, ncol, i0, i0, f0)), ("CSC", ctx.csc(nrow, ncol, np.zeros(ncol + 1, np.int32), i0, f0))):
        for kernel in (AUTO, VECTOR, PANEL):
            try:
                H.set_kernel(kernel)
            except pkg.capi.SpmvError:
                continue
            D.check(ctx, H, f"{name} {nrow} x {ncol} without entries, kernel {kernel}")
    # an ELL handle that is all padding: every slot reads x[0] (finite) times 0.0
    k = 3
    pads = ex.ell_entries(nrow, k, np.zeros(nrow * k, np.int32), np.zeros(nrow * k))
    P = ExactDot(rng, nrow, ncol, pads, 6, 4)
    assert np.isfinite(P.xp[0]) and not np.isfinite(P.xp[1:]).any() and not P.want0.any()
    H = ctx.ell(nrow, ncol, k, 0, np.zeros(nrow * k, np.int32), np.zeros(nrow * k))
    for kernel in (AUTO, VECTOR, PANEL):
        try:
            H.set_kernel(kernel)
        except pkg.capi.SpmvError:
            continue
        P.check(ctx, H, f"ELL {nrow} x {ncol}, all padding, kernel {kernel} (runs {H.info.kernel})")
    # no rows: nothing to write, w . y = 0
    Z = ExactDot(rng, 0, 5, none, 6, 4)
    for name, H in (("CSR", ctx.csr(0, 5, np.zeros(1, np.int32), i0, f0)), ("COO", ctx.coo(0, 5, i0, i0, f0)), ("ELL", ctx.ell(0, 5, 0, 0, i0, f0))):
        Z.check(ctx, H, f"{name} 0 x 5")
    SEEN["extras:degenerate"].update({"no entries", "all padding", "no rows"})


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 257, 524_289, 3_000_001])
def test_exact_dot(ctx, n):
    """spmv_dot on dyadic vectors whose whole sum stays within 2^53: the bits of the integer sum, at the edges of a wavefront, a
    workgroup and the grid (524,288 threads)"""
    rng = np.random.default_rng(BASE + 19_990 + n % 1000)
    bits, e = ex.choose_bits(max(n, 1), 1)  # n products of two dyadic factors: the budget of one output of n terms
    x, y = ex.dyadic(rng, n, bits, e), ex.dyadic(rng, n, bits, e)
    want = ex.exact_dot(x, y, e, e)
    got = ctx.dot(_vec(ctx, x), _vec(ctx, y))
    assert got == want, f"n = {n}: spmv_dot {got!r}, exact {want!r}"
    if n:
        y[n - 1] = -y[n - 1]  # the last element counts
        assert ctx.dot(_vec(ctx, x), _vec(ctx, y)) == ex.exact_dot(x, y, e, e) != want
    SEEN["dot"].add(n)


# ---- what ran ------------------------------------------------------------------------------------------------------------------
def test_every_kernel_ran():
    """across the seeds above: every kernel and layout this file names ran at least once"""
    expect = {"csr": N_CSR, "coo": N_COO, "csc": N_CSC, "ell": N_ELL, "dia": N_DIA, "multi": N_MULTI, "extras": len(EXTRAS_SEEDS), "extras:formats": 5}
    if any(RUNS[f] != n for f, n in expect.items()):
        pytest.skip(f"the coverage check needs every seed of this module (ran {dict(RUNS)})")
    need = {
        "csr": {VECTOR, SCALAR, LDSWIN, PANEL, TWOPHASE, SEGSCAN, SPLIT, ELLK, "ell copy"},
        "csr:panel_layout": {3, 4},
        "csr:twophase_padded": {True},
        "csr:split_mode": {0, 1, 2},
        "csr^T": {VECTOR, PANEL},
        "apply_host": {AUTO, SCALAR, PANEL, SEGSCAN},
        "coo": {VECTOR, PANEL},
        "coo^T": {VECTOR, PANEL},
        "csc": {VECTOR, PANEL},
        "csc^T": {SCALAR, VECTOR, PANEL, TWOPHASE, SEGSCAN, SPLIT, LDSWIN, ELLK},
        "ell": {(1, 0), (1, 8), (2, 0), (2, 8), "dia_order", ("panel", PANEL)},
        "ell^T": {VECTOR, PANEL},
        "dia": {"bound", "plain"},
        "dia^T": {"tiled", "general"},
        "multi": {"csr", "ell"},
        "multi:k": set(KS),
        "multi:lanes": {32, 64},
        "multi:grid_stride": {16},
        "wrapped": {"coo", "ell"},
        # spmv_apply_dot: every CSR kernel id, the kernels that fuse the extras and the ones that run behind a fill and before a dot pass
        "extras": {AUTO, VECTOR, SCALAR, LDSWIN, PANEL, TWOPHASE, SEGSCAN, SPLIT, ELLK},
        "extras:path": {"fused", "behind"},
        "extras:empty_rows": {AUTO, VECTOR, SCALAR, PANEL, TWOPHASE, SEGSCAN, SPLIT},
        "extras:panel_layout": {3, 4},
        "extras:split_mode": {0, 1, 2},
        "extras:coo": {VECTOR, PANEL},
        "extras:csc": {VECTOR, PANEL},
        "extras:ell": {VECTOR, PANEL},
        "extras:wrapped": {"coo", "ell", "ell copy"},
        "extras:no_entries": {VECTOR, SCALAR},
        "extras:degenerate": {"no entries", "all padding", "no rows"},
        "dot": {0, 1, 63, 64, 65, 255, 257, 524_289, 3_000_001},
    }
    missing = {f: sorted(map(str, want - SEEN[f])) for f, want in need.items() if not want <= SEEN[f]}
    assert not missing, f"never ran: {missing}; ran: { {f: sorted(map(str, v)) for f, v in SEEN.items()} }"
