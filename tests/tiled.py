"""Block-diagonal copies as an oracle for kernels that loop over their grid - TEST INFRASTRUCTURE ONLY (no GPU needed).

A streaming or row-group kernel launches at most kMaxGrid workgroups (csrc/common.hpp) and loops beyond that; on a later trip a
workgroup reuses its LDS, its barriers and its offsets for other rows.  If A is the block-diagonal matrix of k copies of A0, every
row of a later copy poses the problem of its row in copy 0 with shifted indices, so the result is the base result tiled: the
pattern shifted by the copy's offset, the values the same bytes.  The twin runs on the base alone.  Rows are listed by class in
ascending index (one stable pass of sort_ids_by_key), so copy 0 lies in the first trip and later copies in later ones.

tile_csr is the tiling (of an input as of a result), tiled_mismatch the comparison that names copy, row and trip, and the readers
below take every threshold from the settings headers: where a header gives an expression, its text is asserted and the expression
recomputed here, so that a changed setting fails a coverage assertion instead of quietly taking the loop out of a test."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np

CSRC = Path(__file__).resolve().parent.parent / "arm-spmv_amd" / "csrc"


# ---- the settings ------------------------------------------------------------------------------------------------------------------
def _code(name):
    """a source file without its // comments, every run of white space one blank"""
    text = re.sub(r"//[^\n]*", "", (CSRC / name).read_text())
    return re.sub(r"\s+", " ", text)


def _constant(code, name):
    """constexpr int NAME = a product of integers;"""
    m = re.search(rf"constexpr int {name} = ([0-9* ]+);", code)
    assert m, f"{name} is no product of integers any more"
    return int(np.prod([int(f) for f in m.group(1).split("*")]))


def block_lanes():
    return _constant(_code("common.hpp"), "kBlock")


def max_grid():
    """kMaxGrid: the most workgroups a streaming or row-group kernel launches"""
    code = _code("common.hpp")
    assert "constexpr int kMaxGrid = kNumCu * 8;" in code, "common.hpp no longer says kMaxGrid = kNumCu * 8"
    return _constant(code, "kNumCu") * 8


def spgemm_classes():
    """[(lanes of a row, capacity in products, rows a workgroup)] of spgemm's LDS classes, ascending"""
    code = _code("spgemm_settings.hpp")
    lanes_of_block = _constant(code, "kSpgemmBlockLanes")
    assert "constexpr int spgemm_rows_per_block(int cls) { return spgemm_info(cls).lanes ? kSpgemmBlockLanes / spgemm_info(cls).lanes : 0; }" in code
    found = sorted((int(c), int(l)) for l, c in re.findall(r"spgemm_class_info\{(\d+), (\d+)\}", code) if int(c) > 0)
    assert len(found) == 3 and lanes_of_block == block_lanes(), "three LDS classes in a default workgroup"
    return [(l, c, lanes_of_block // l) for c, l in found]


def fsai_lanes():
    """the lane classes of the FSAI row kernel: 4, 8, 16, 32, 64"""
    code = _code("fsai_settings.hpp")
    assert "constexpr int fsai_lanes(int cls) { return kFsaiMinLanes << cls; }" in code
    return [_constant(code, "kFsaiMinLanes") << c for c in range(_constant(code, "kFsaiClasses"))]


def fsai_class_of(m):
    """the class of a row of m pattern columns: the narrowest group that holds it (fsai_class_of)"""
    code = _code("fsai_settings.hpp")
    assert "while (c < kFsaiClasses && ((int64_t)kFsaiMinLanes << c) < m) ++c;" in code
    return int(np.searchsorted(fsai_lanes(), max(int(m), 1)))


def fsai_groups_per_block(lanes):
    """groups of `lanes` lanes a workgroup of the FSAI row kernel holds: the header's text, recomputed"""
    code = _code("fsai_settings.hpp")
    for text in ("constexpr int64_t fsai_tri(int64_t p) { return p * (p + 1) / 2; }",
                 "constexpr int fsai_group_doubles(int lanes) { return (int)fsai_tri(lanes) + lanes + lanes / 2; }",
                 "constexpr int fsai_groups_per_block(int lanes) { int g = kFsaiBlockLanes / lanes; "
                 "while (g > 1 && g * fsai_group_doubles(lanes) * 8 > kFsaiLdsPerBlock) --g; "
                 "while (g > 1 && (g * lanes) % kFsaiWave) --g; return g; }"):
        assert text in code, f"fsai_settings.hpp no longer says: {text}"
    doubles = lanes * (lanes + 1) // 2 + lanes + lanes // 2
    g = _constant(code, "kFsaiBlockLanes") // lanes
    while g > 1 and g * doubles * 8 > _constant(code, "kFsaiLdsPerBlock"):
        g -= 1
    while g > 1 and (g * lanes) % _constant(code, "kFsaiWave"):
        g -= 1
    return g


def rcm_lanes(mean_degree):
    """lanes that share a frontier vertex in the breadth-first kernels (rcm_lanes): the header's text, recomputed"""
    code = _code("reorder_settings.hpp")
    text = "constexpr int rcm_lanes(double mean_degree) { int lanes = 4; while (lanes < 64 && lanes * 2 < mean_degree) lanes *= 4; return lanes; }"
    assert text in code, f"reorder_settings.hpp no longer says: {text}"
    lanes = 4
    while lanes < 64 and lanes * 2 < mean_degree:
        lanes *= 4
    return lanes


def rcm_row_lanes():
    """lanes a row in the kernels that walk the rows of A (the adjacency, the permutation's keys, the bandwidth)"""
    code = _code("reorder.hip")
    assert "constexpr int kPermuteLanes = kRowLanes;" in code
    return _constant(code, "kRowLanes")


def bsr_slots(bs):
    """whole blocks of bs x bs values a wavefront holds at a time (bsr_slots): S of the BSR tests"""
    code = _code("bsr_settings.hpp")
    assert "constexpr int bsr_slots(int bs) { return kBsrWave / (bs * bs); }" in code, "bsr_settings.hpp no longer says bsr_slots = kBsrWave / bs^2"
    return _constant(code, "kBsrWave") // (bs * bs)


def bsr_rows_per_workgroup(bs, lanes):
    """block rows a workgroup of the BSR product holds at `lanes` lanes a block row: the header's text, recomputed"""
    code = _code("bsr_settings.hpp")
    for text in ("constexpr int bsr_rows_per_wave(int bs, int lanes) { return bsr_slots(bs) / (lanes / (bs * bs)); }",
                 "constexpr int bsr_rows_per_workgroup(int bs, int lanes) { return (kBsrWorkgroup / kBsrWave) * bsr_rows_per_wave(bs, lanes); }"):
        assert text in code, f"bsr_settings.hpp no longer says: {text}"
    assert lanes % (bs * bs) == 0 and bsr_slots(bs) % (lanes // (bs * bs)) == 0, "lanes: bs^2 times a divisor of the slots"
    return (_constant(code, "kBsrWorkgroup") // _constant(code, "kBsrWave")) * (bsr_slots(bs) // (lanes // (bs * bs)))


def bsr_kernel_cases():
    """[(bs, G)] of the instances bsr_apply's switch launches (csrc/kernels_bsr.hip): G blocks of bs x bs values a step"""
    found = re.findall(r"case (\d+): return launch_bsr<(\d+), (\d+)>\(ctx, A, x, y\);", _code("kernels_bsr.hip"))
    assert found and all(int(label) == int(bs) * 100 + int(g) for label, bs, g in found), "bsr_apply's switch is keyed bs * 100 + g"
    return [(int(bs), int(g)) for _, bs, g in found]


# ---- the tiling --------------------------------------------------------------------------------------------------------------------
def tile_csr(k, ncol0, rp, cc, cv=None):
    """(row_ptr, col[, val]) of the block-diagonal matrix of k copies of the CSR matrix (rp, cc, cv) with ncol0 columns: copy c holds
    the base's rows with every column shifted by c ncol0 and the same values"""
    rp, cc = np.asarray(rp, dtype=np.int64), np.asarray(cc, dtype=np.int64)
    nnz0 = int(rp[-1])
    assert len(cc) == nnz0 and k >= 1 and k * max(nnz0, ncol0, len(rp)) < 2**31, "int32 offsets and columns"
    at = np.arange(k, dtype=np.int64)[:, None]
    out_rp = np.concatenate([[0], (rp[None, 1:] + nnz0 * at).ravel()]).astype(np.int32)
    out_cc = (cc[None, :] + ncol0 * at).ravel().astype(np.int32)
    return (out_rp, out_cc) if cv is None else (out_rp, out_cc, np.tile(np.asarray(cv, dtype=np.float64), k))


def tile_bsr(k, nbc0, bp, bc, bv, bs):
    """(brow_ptr, bcol, val) of the block-diagonal matrix of k copies of the BSR matrix (bp, bc, bv) with nbc0 block columns of
    bs x bs values: tile_csr on the block arrays, every copy's blocks the same bytes"""
    bv = np.asarray(bv, dtype=np.float64)
    assert len(bv) == len(bc) * bs * bs
    out_bp, out_bc = tile_csr(k, nbc0, bp, bc)
    return out_bp, out_bc, np.tile(bv, k)


def trips(rows, per_workgroup, grid):
    """the trips over a grid of at most `grid` workgroups that `rows` listed rows take at per_workgroup rows a workgroup"""
    return -(-(-(-rows // per_workgroup)) // grid)


def describe_trips(cls0, per_workgroup, grid, names=None):
    """where(copy, row) for tiled_mismatch.  cls0[r]: the class of base row r; per_workgroup[c]: the rows of class c a workgroup
    holds (a class that is not in it is named alone).  The rows of a class are listed in ascending index, so row r of copy c stands
    at place c * (rows of the class a copy) + (rank of r among them), in workgroup place // per_workgroup, which the kernel reaches
    on trip workgroup // grid."""
    cls0 = np.asarray(cls0)
    rank, count = np.zeros(len(cls0), dtype=np.int64), {}
    for c in np.unique(cls0):
        at = np.flatnonzero(cls0 == c)
        rank[at], count[int(c)] = np.arange(len(at)), len(at)

    def where(copy, row):
        c = int(cls0[row])
        label = names[c] if names else str(c)
        if c not in per_workgroup:
            return f"class {label}"
        place = copy * count[c] + int(rank[row])
        return f"place {place} of class {label}, trip {place // per_workgroup[c] // grid}"

    return where


def tiled_mismatch(got, base, k, ncol0, where=None):
    """None where `got` = (row_ptr, col, val) is tile_csr(k, ncol0, *base), integer for integer and the values as bytes; else one line
    on the first difference: the array, the copy, the row within the copy and what where(copy, row) says about it"""
    want = tile_csr(k, ncol0, *base)
    nrow0 = len(base[0]) - 1

    def named(row):
        copy, r = divmod(int(row), nrow0)
        return f"copy {copy}, row {r}" + (f" ({where(copy, r)})" if where else "")

    for part, g, w in zip(("row_ptr", "col", "val"), got, want):
        g = np.asarray(g)
        if g.dtype != w.dtype or g.shape != w.shape:
            return f"{part} has {g.shape} {g.dtype}, the tiled twin {w.shape} {w.dtype}"
        same = g == w if part != "val" else g.view(np.uint64) == w.view(np.uint64)
        if same.all():
            continue
        at = int(np.flatnonzero(~same)[0])
        # row_ptr[at] closes row at - 1; an entry lies in the row whose stretch of the tiled row_ptr holds it
        row = max(at - 1, 0) if part == "row_ptr" else int(np.searchsorted(want[0], at, side="right")) - 1
        shown = f"{g[at]!r} against {w[at]!r}" if part != "val" else f"{g[at]!r} ({g[at].hex()}) against {w[at]!r} ({w[at].hex()})"
        return f"{part}[{at}] is {shown}: {named(row)}"
    return None
