"""Small deterministic test matrices (inputs only).  Shared by tests/golden/make_golden.py and the tests.

The cases follow SURVEY.md 8c: (1) 8x8 tridiagonal, (2) 64x48 rectangular, unsorted, with duplicate entries
and empty rows, (3) one 4096-entry row among short rows (long-row / carry-out path), (4) BASELINE config 1:
10k x 10k, 16 entries per row, drawn from the engine's own counter-based generator.
"""
from __future__ import annotations

import hashlib

import numpy as np

from __graft_entry__ import load_package

synth = load_package().synth


def tri8():
    n = 8
    row, col, val = [], [], []
    for i in range(n):
        for j in (i - 1, i, i + 1):
            if 0 <= j < n:
                row.append(i)
                col.append(j)
                val.append(2.0 + 0.125 * i if i == j else -1.0 + 0.0625 * (i + j))
    x = np.arange(1, n + 1, dtype=np.float64) / 8.0
    return dict(name="tri8", nrow=n, ncol=n, row=np.array(row, np.int32), col=np.array(col, np.int32),
                val=np.array(val, np.float64), x=x)


def rect64x48():
    """unsorted COO, duplicates (same (i,j) several times), rows 5, 17, 40..44 and 63 empty"""
    rng = np.random.RandomState(20240607)
    nrow, ncol = 64, 48
    empty = {5, 17, 40, 41, 42, 43, 44, 63}
    rows = [r for r in range(nrow) if r not in empty]
    row = rng.choice(rows, size=400).astype(np.int32)
    col = rng.randint(0, ncol, size=400).astype(np.int32)
    val = rng.uniform(-1.0, 1.0, size=400)
    # force duplicates: repeat the first 40 coordinates with new values
    row = np.concatenate([row, row[:40]])
    col = np.concatenate([col, col[:40]])
    val = np.concatenate([val, rng.uniform(-1.0, 1.0, size=40)])
    perm = rng.permutation(row.size)
    x = rng.uniform(0.0, 1.0, size=ncol)
    return dict(name="rect64x48", nrow=nrow, ncol=ncol, row=row[perm], col=col[perm], val=val[perm], x=x)


def longrow():
    """300 x 5000, row 137 holds 4096 entries, the others 0..9; row-sorted"""
    rng = np.random.RandomState(7)
    nrow, ncol = 300, 5000
    lens = rng.randint(0, 10, size=nrow)
    lens[137] = 4096
    row = np.repeat(np.arange(nrow, dtype=np.int32), lens)
    col = rng.randint(0, ncol, size=row.size).astype(np.int32)
    val = rng.uniform(-1.0, 1.0, size=row.size)
    x = rng.uniform(0.0, 1.0, size=ncol)
    return dict(name="longrow", nrow=nrow, ncol=ncol, row=row, col=col, val=val, x=x)


C1_SEED = 2024


def c1():
    """BASELINE.json config 1: 10k x 10k, 16 entries per row, uniform columns, values U(-1,1), x U(0,1)"""
    n, k = 10_000, 16
    row_ptr, col, val = synth.csr_uniform(0, n, n, k, band=0, seed=C1_SEED)
    row = np.repeat(np.arange(n, dtype=np.int32), k)
    x = synth.vec_uniform(n, seed=C1_SEED)
    return dict(name="c1", nrow=n, ncol=n, row=row, col=col, val=val, x=x)


SMALL_CASES = (tri8, rect64x48, longrow)
ALL_CASES = SMALL_CASES + (c1,)


def digest(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# ------------------------------------------------ inputs of the tests against the compiled reference (golden: reader.npz, live.npz)
def live_matrices():
    """random COO matrices and x of test_oracle_golden.py::test_oracle_live_against_compiled_reference (fixed seed):
    yields (nrow, ncol, row, col, val, x)"""
    rng = np.random.RandomState(123)
    for nrow, ncol, nnz in ((1, 1, 1), (17, 5, 60), (200, 300, 5000), (1000, 1000, 16000)):
        row = rng.randint(0, nrow, size=nnz).astype(np.int32)
        col = rng.randint(0, ncol, size=nnz).astype(np.int32)
        val = rng.uniform(-1, 1, size=nnz)
        x = rng.uniform(0, 1, size=ncol)
        yield nrow, ncol, row, col, val, x


def odd_mtx_files(directory):
    """Matrix Market files whose reading is DEFINED in the reference (every `fscanf("%d %d %lg\\n")` of
    src/data_io.cpp:83-88 converts three tokens) but that a reader written from the format description would treat
    differently.  Written into `directory`; returns {file name: path}.  (Files with fewer than 3 x nnz tokens are left out:
    there the reference returns uninitialised heap for the missing entries, the shim stops with a message — no common
    answer exists.)"""
    rng = np.random.RandomState(11)
    files = {}

    def put(name, text):
        p = directory / name
        p.write_text(text)
        files[name] = p

    put("comments_blank_tabs.mtx",
        "%%MatrixMarket matrix coordinate real general\n% c1\n%\n%%% c3\n\n  5 4   6  \n\n1\t1\t 1.5\n\n2 3 -2.25   \n\n\n"
        "5 4 1e-3\n3 2 +4\n 4 1 .5\n1 4 -7.0E+2\n% a trailing comment is not an entry\n9 9 9\n")
    put("integer_field.mtx", "%%MatrixMarket matrix coordinate integer general\n3 3 4\n1 1 7\n2 2 -3\n3 1 12\n1 3 0\n")
    # symmetric / skew / hermitian-free variants: read as stored, NOT expanded
    put("symmetric.mtx", "%%MatrixMarket matrix coordinate real symmetric\n4 4 5\n1 1 2.0\n2 1 -1.0\n3 2 -1.0\n4 4 3.0\n4 1 0.25\n")
    put("skew.mtx", "%%MatrixMarket matrix coordinate real skew-symmetric\n3 3 2\n2 1 5.0\n3 1 -6.0\n")
    # four integer tokens per line: the reference re-chunks the token stream in threes, whatever the lines look like
    lines = "".join(f"{i + 1} {(i * 7) % 9 + 1} {i - 4} {i + 100}\n" for i in range(9))
    put("extra_column.mtx", "%%MatrixMarket matrix coordinate real general\n9 9 9\n" + lines)
    # a `pattern` file that declares fewer entries than it has tokens for: (i, j, next i) triples, all conversions succeed
    put("pattern_short_count.mtx", "%%MatrixMarket matrix coordinate pattern general\n6 6 4\n1 2\n3 4\n5 6\n6 1\n2 2\n4 4\n")
    # what %lg accepts: hex floats, infinities, nan, many digits
    put("float_forms.mtx", "%%MatrixMarket matrix coordinate real general\n2 8 8\n1 1 0x1.8p1\n1 2 inf\n1 3 -INF\n1 4 nan\n"
        "1 5 123456789012345678901234567890\n1 6 1e-400\n1 7 0.1000000000000000055511151231257827\n1 8 -0\n")
    put("more_lines_than_declared.mtx", "%%MatrixMarket matrix coordinate real general\n3 3 2\n1 1 1\n2 2 2\n3 3 3\n1 2 4\n")
    put("zero_entries.mtx", "%%MatrixMarket matrix coordinate real general\n7 5 0\n")
    put("array_of_ints_as_indices.mtx", "%%MatrixMarket matrix coordinate real general\n10 10 3\n007 +3 1\n10 010 2\n1 1 3\n")
    # big enough for the parallel parser (>= 65536 entries), with ragged formatting
    n = 70_001
    r, c = rng.randint(1, 5000, n), rng.randint(1, 4000, n)
    v = rng.uniform(-1, 1, n)
    seps = [" ", "\t", "  ", " \t "]
    body = []
    for k in range(n):
        s = seps[k % 4]
        val = ("%.17g" % v[k]) if k % 5 else ("%+.6e" % v[k])
        body.append(f"{r[k]}{s}{c[k]}{s}{val}" + ("\n\n" if k % 97 == 0 else "\n"))
    put("large_ragged.mtx", f"%%MatrixMarket matrix coordinate real general\n% big\n5000 4000 {n}\n" + "".join(body))
    big_sym = "".join(f"{max(a, b)} {min(a, b)} {k % 13 - 6}\n" for k, (a, b) in enumerate(zip(r, c)))
    put("large_symmetric_integer.mtx", f"%%MatrixMarket matrix coordinate integer symmetric\n5000 5000 {n}\n" + big_sym)
    return files
