"""NumPy twin of the reordering entry points (csrc/reorder.hip; include/spmv_abi.h, "reordering") - TEST INFRASTRUCTURE ONLY.

The reverse Cuthill-McKee ordering is a fixed permutation: the graph is the pattern of A + A^T without its diagonal (stored zeros
count, duplicates count once), deg is the number of distinct neighbours, and the Cuthill-McKee sequence cm is
  1. the vertices of degree 0 in ascending index;
  2. per component, a root: the unnumbered vertex of smallest (deg, index), refined by George and Liu's rule at most
     kRcmRootRepeats times (csrc/reorder_settings.hpp, read here);
  3. the root, then level by level: the unnumbered neighbours of the current level, ordered by (smallest position in cm among
     their neighbours in the current level, deg, index).
order[k] = cm[n-1-k].  rcm_levelwise is that rule (what the device runs); rcm_queue is the textbook queue (pop v, append its
unnumbered neighbours in ascending (deg, index)); tests/test_rcm_ref.py holds them equal.

The graph families the CPU and the GPU tests share are at the end.
"""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np

_SETTINGS = Path(__file__).resolve().parent.parent / "arm-spmv_amd" / "csrc" / "reorder_settings.hpp"


def root_repeats() -> int:
    return int(re.search(r"kRcmRootRepeats\s*=\s*(\d+)", _SETTINGS.read_text()).group(1))


# ---- the graph ---------------------------------------------------------------------------------------------------------------------
def adjacency(n: int, row_ptr, col):
    """(adj_rp, adj) of the pattern of A + A^T without its diagonal: every neighbour once, ascending inside a row"""
    rp = np.asarray(row_ptr, dtype=np.int64)
    c = np.asarray(col, dtype=np.int64)
    r = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    keep = r != c
    key = np.unique(np.concatenate([r[keep] * n + c[keep], c[keep] * n + r[keep]])) if n else np.zeros(0, np.int64)
    i, j = (key // n, key % n) if n else (key, key)
    adj_rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(i, minlength=n), out=adj_rp[1:])
    return adj_rp, j


def _neighbours(adj_rp, adj, frontier):
    """(place in `frontier` of the parent, neighbour) of every adjacency entry of the frontier's vertices, in (place, index) order"""
    f = np.asarray(frontier, dtype=np.int64)
    lens = adj_rp[f + 1] - adj_rp[f]
    parent = np.repeat(np.arange(len(f), dtype=np.int64), lens)
    start = np.repeat(adj_rp[f], lens)
    within = np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)
    return parent, adj[start + within]


def level_structure(adj_rp, adj, root: int, reached=None):
    """the levels of `root` as a list of arrays (ascending index inside a level); `reached` marks vertices to leave out"""
    seen = np.zeros(len(adj_rp) - 1, dtype=bool) if reached is None else reached.copy()
    seen[root] = True
    levels = [np.array([root], dtype=np.int64)]
    while True:
        _, w = _neighbours(adj_rp, adj, levels[-1])
        w = np.unique(w[~seen[w]])
        if not len(w):
            return levels
        seen[w] = True
        levels.append(w)


def _smallest(deg, vertices) -> int:
    v = np.asarray(vertices, dtype=np.int64)
    return int(v[np.lexsort((v, deg[v]))[0]])


def find_root(adj_rp, adj, deg, start: int, numbered, counters) -> int:
    """George and Liu's rule from `start`; counters["bfs"] counts the level structures built"""
    r, Lr = start, level_structure(adj_rp, adj, start, numbered)
    counters["bfs"] += 1
    for _ in range(root_repeats()):
        c = _smallest(deg, Lr[-1])
        Lc = level_structure(adj_rp, adj, c, numbered)
        counters["bfs"] += 1
        if len(Lc) <= len(Lr):
            break
        r, Lr = c, Lc
    return r


def _new_counters():
    return {"isolated": 0, "components": 0, "levels": 0, "bfs": 0}


def _sequence(n, adj_rp, adj, number_component):
    deg = np.diff(adj_rp)
    counters = _new_counters()
    lone = np.flatnonzero(deg == 0)
    counters["isolated"] = len(lone)
    cm = [lone]
    numbered = deg == 0
    widths = []  # per component: the widths of the levels of its numbering pass
    for v in np.lexsort((np.arange(n), deg)):
        if numbered[v]:
            continue
        counters["components"] += 1
        root = find_root(adj_rp, adj, deg, int(v), numbered, counters)
        part, w = number_component(adj_rp, adj, deg, root, numbered)
        counters["bfs"] += 1
        counters["levels"] += len(w)
        widths.append(w)
        cm.append(part)
    cm = np.concatenate(cm) if cm else np.zeros(0, np.int64)
    return cm.astype(np.int64), counters, widths


def _number_levelwise(adj_rp, adj, deg, root, numbered):
    numbered[root] = True
    out, level, widths = [np.array([root], dtype=np.int64)], np.array([root], dtype=np.int64), [1]
    while True:
        parent, w = _neighbours(adj_rp, adj, level)
        keep = ~numbered[w]
        parent, w = parent[keep], w[keep]
        if not len(w):
            return np.concatenate(out), widths
        o = np.lexsort((parent, w))  # every vertex once, with its smallest parent
        w, parent = w[o], parent[o]
        first = np.r_[True, w[1:] != w[:-1]]
        w, parent = w[first], parent[first]
        level = w[np.lexsort((w, deg[w], parent))]
        numbered[level] = True
        out.append(level)
        widths.append(len(level))


def _number_queue(adj_rp, adj, deg, root, numbered):
    numbered[root] = True
    queue, head = [root], 0
    while head < len(queue):
        v = queue[head]
        head += 1
        w = adj[adj_rp[v]:adj_rp[v + 1]]
        w = w[~numbered[w]]
        w = w[np.lexsort((w, deg[w]))]
        numbered[w] = True
        queue.extend(int(t) for t in w)
    part = np.array(queue, dtype=np.int64)
    return part, [len(lv) for lv in level_structure(adj_rp, adj, root)]


def rcm_levelwise(n: int, row_ptr, col):
    """(order, inverse, counters, widths): what spmv_perm_rcm returns and reports ("rcm_isolated", "rcm_components", "rcm_levels",
    "rcm_bfs"), and per component the widths of the levels of its numbering pass"""
    adj_rp, adj = adjacency(n, row_ptr, col)
    cm, counters, widths = _sequence(n, adj_rp, adj, _number_levelwise)
    order = cm[::-1].astype(np.int32)
    inverse = np.empty(n, dtype=np.int32)
    inverse[order] = np.arange(n, dtype=np.int32)
    return order, inverse, counters, widths


def rcm_queue(n: int, row_ptr, col):
    """the same by the textbook queue algorithm"""
    adj_rp, adj = adjacency(n, row_ptr, col)
    cm, counters, widths = _sequence(n, adj_rp, adj, _number_queue)
    order = cm[::-1].astype(np.int32)
    inverse = np.empty(n, dtype=np.int32)
    inverse[order] = np.arange(n, dtype=np.int32)
    return order, inverse, counters, widths


def level_widths(n: int, row_ptr, col):
    return rcm_levelwise(n, row_ptr, col)[3]


def bandwidth_bound(widths) -> int:
    """max over adjacent levels of w_i + w_{i+1}, minus 1: an entry joins vertices of one level or of two adjacent ones, and the
    levels stand one behind the other in the sequence (0 without edges)"""
    best = 0
    for w in widths:
        for a, b in zip(w[:-1], w[1:]):
            best = max(best, a + b - 1)
    return best


# ---- matrices ----------------------------------------------------------------------------------------------------------------------
def inverse_of(order):
    order = np.asarray(order, dtype=np.int64)
    inv = np.empty(len(order), dtype=np.int64)
    inv[order] = np.arange(len(order), dtype=np.int64)
    return inv


def permute_csr(nrow: int, ncol: int, row_ptr, col, val, order_r=None, order_c=None):
    """B[k][l] = A[order_r[k]][order_c[l]]: ascending new column inside a row, equal new columns in A's stored order, values as
    they are; None is the identity (the columns are still ordered)"""
    rp = np.asarray(row_ptr, dtype=np.int64)
    inv_r = np.arange(nrow, dtype=np.int64) if order_r is None else inverse_of(order_r)
    inv_c = np.arange(ncol, dtype=np.int64) if order_c is None else inverse_of(order_c)
    r = inv_r[np.repeat(np.arange(nrow, dtype=np.int64), np.diff(rp))]
    c = inv_c[np.asarray(col, dtype=np.int64)]
    o = np.lexsort((np.arange(len(c)), c, r))
    out_rp = np.zeros(nrow + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=nrow), out=out_rp[1:])
    return out_rp.astype(np.int32), c[o].astype(np.int32), np.asarray(val, dtype=np.float64)[o]


def bandwidth_profile(nrow: int, row_ptr, col):
    """(max |i - j| over the entries, sum over the non-empty rows of max(0, i - min j))"""
    rp = np.asarray(row_ptr, dtype=np.int64)
    c = np.asarray(col, dtype=np.int64)
    if not len(c):
        return 0, 0
    r = np.repeat(np.arange(nrow, dtype=np.int64), np.diff(rp))
    lo = np.full(nrow, np.iinfo(np.int64).max)
    np.minimum.at(lo, r, c)
    rows = np.flatnonzero(np.diff(rp) > 0)
    return int(np.max(np.abs(r - c))), int(np.sum(np.maximum(0, rows - lo[rows])))


# ---- graph families (CSR triples with int32 indices; the values are small integers unless a test draws its own) ----------------------
def csr_from_entries(n: int, r, c, v=None, ncol=None):
    """CSR of the entry list in (row, stored order): nothing is sorted inside a row, nothing merged"""
    r, c = np.asarray(r, dtype=np.int64), np.asarray(c, dtype=np.int64)
    v = np.ones(len(r)) if v is None else np.asarray(v, dtype=np.float64)
    o = np.argsort(r, kind="stable")
    rp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=rp[1:])
    return n, rp.astype(np.int32), c[o].astype(np.int32), v[o]


def from_edges(n: int, a, b, diagonal=True):
    """the symmetric matrix of the edges (a, b), both ways, with a diagonal; columns ascending, every entry once"""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    d = np.arange(n, dtype=np.int64) if diagonal else np.zeros(0, np.int64)
    key = np.unique(np.concatenate([a * n + b, b * n + a, d * n + d])) if n else np.zeros(0, np.int64)
    r, c = (key // n, key % n) if n else (key, key)
    return csr_from_entries(n, r, c, np.where(r == c, 4.0, -1.0))


def path(n: int):
    return from_edges(n, np.arange(n - 1), np.arange(1, n))


def grid(*shape):
    idx = np.arange(int(np.prod(shape))).reshape(shape)
    a, b = [], []
    for ax in range(len(shape)):
        lo = [slice(None)] * len(shape)
        hi = [slice(None)] * len(shape)
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        a.append(idx[tuple(lo)].ravel())
        b.append(idx[tuple(hi)].ravel())
    return from_edges(idx.size, np.concatenate(a), np.concatenate(b))


def star(leaves: int):
    return from_edges(leaves + 1, np.zeros(leaves, dtype=np.int64), np.arange(1, leaves + 1))


def broom(children: int, seed: int):
    """a root (vertex 0) with `children` children, every child with 0, 1 or 2 leaves of its own: a tree of mean degree 2 whose level
    structures hold two levels about as wide as `children`"""
    leaves = np.random.default_rng(seed).integers(0, 3, children)
    child = np.arange(1, children + 1, dtype=np.int64)
    n = 1 + children + int(leaves.sum())
    a = np.concatenate([np.zeros(children, dtype=np.int64), np.repeat(child, leaves)])
    b = np.concatenate([child, np.arange(1 + children, n, dtype=np.int64)])
    return from_edges(n, a, b)


def hairy_star(children: int, sibling_edges: int, seed: int):
    """a root (vertex 0) with `children` children, one leaf under every child, and random edges among the children: the edges among
    siblings raise the mean degree without changing who alone reaches a leaf - its parent, wherever that stands in its frontier"""
    rng = np.random.default_rng(seed)
    child = np.arange(1, children + 1, dtype=np.int64)
    s, t = rng.integers(1, children + 1, sibling_edges), rng.integers(1, children + 1, sibling_edges)
    keep = s != t
    a = np.concatenate([np.zeros(children, dtype=np.int64), child, s[keep]])
    b = np.concatenate([child, child + children, t[keep]])
    return from_edges(1 + 2 * children, a, b)


def complete(n: int):
    a, b = np.triu_indices(n, 1)
    return from_edges(n, a, b)


def random_graph(n: int, edges: int, seed: int):
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, n, edges), rng.integers(0, n, edges)
    keep = a != b
    return from_edges(n, a[keep], b[keep])


def band(n: int, half: int, per_row: int, seed: int):
    """per_row entries a row at random columns within `half` of the diagonal: an unsymmetric pattern"""
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(n), per_row)
    c = np.clip(r + rng.integers(-half, half + 1, n * per_row), 0, n - 1)
    key = np.unique(r * n + c)
    return csr_from_entries(n, key // n, key % n, 1.0 + (key % 7))


# Graphs whose widest frontier takes the breadth-first kernels (rcm_claim / count / fill_kernel<LANES>) on a second trip over their
# grid, for every lane count - name: (the graph, the lanes its mean degree selects) - and, the first two, with more rows than one trip
# of the 16-lanes-a-row kernels takes (the adjacency, the permutation's keys, the bandwidth).  tests/test_rcm_ref.py holds their widths and
# lane counts to the settings on the CPU, tests/test_gpu_reorder.py runs them.
GRID_LOOP_GRAPHS = {
    "broom131200": (lambda: shuffled(broom(131_200, 5), 6), 4),
    "random100000_deg10": (lambda: random_graph(100_000, 500_000, 7), 16),
    "random20000_deg40": (lambda: random_graph(20_000, 400_000, 8), 64),
    # in random20000_deg40 every vertex behind the wide frontier has about 29 parents in it, the first of them on the first trip: the
    # later trip claims, counts and fills nothing.  Here the last of 8299 parents each own a leaf that nobody else reaches
    "hairy8300_deg38": (lambda: shuffled(hairy_star(8300, 300_000, 9), 10), 64),
}


def later_trip_children(n, row_ptr, col, order, widths, one_trip):
    """the vertices of a one-component ordering whose first parent - the neighbour that claims them, the one of smallest place in
    the level before - stands at place one_trip or beyond in its level: what a later trip of the breadth-first kernels has to find"""
    adj_rp, adj = adjacency(n, row_ptr, col)
    cm = np.asarray(order, dtype=np.int64)[::-1]
    w = widths[0]
    start = n - sum(w) + np.concatenate([[0], np.cumsum(w)])  # (the vertices without neighbours come first)
    place = np.empty(n, dtype=np.int64)
    place[cm] = np.arange(n)
    found = 0
    for lv in range(1, len(w)):
        level = cm[start[lv]:start[lv + 1]]
        parent, nb = _neighbours(adj_rp, adj, level)
        ok = (place[nb] >= start[lv - 1]) & (place[nb] < start[lv])
        first = np.full(len(level), n, dtype=np.int64)
        np.minimum.at(first, parent[ok], place[nb[ok]] - start[lv - 1])
        assert np.all(first < n), "every vertex of a level has a parent in the level before"
        found += int(np.sum(first >= one_trip))
    return found


def grid_loop_facts(n, row_ptr, col, widths, isolated):
    """(the lanes the device picks for this graph, its widest frontier, the frontier beyond which those lanes loop, the rows beyond
    which the 16-lanes-a-row kernels loop): from the settings headers (tests/tiled.py)"""
    import tiled

    adj_rp, _ = adjacency(n, row_ptr, col)
    lanes = tiled.rcm_lanes(int(adj_rp[-1]) / (n - isolated))  # the mean degree of the vertices with neighbours
    per_block = tiled.block_lanes() // lanes
    return lanes, max(max(w) for w in widths), per_block * tiled.max_grid(), tiled.block_lanes() // tiled.rcm_row_lanes() * tiled.max_grid()


def shuffled(A, seed: int):
    """P A P^T under a random permutation: the same graph in a bad numbering (columns ascending inside a row)"""
    n, rp, c, v = A
    p = np.random.default_rng(seed).permutation(n)
    return (n,) + permute_csr(n, n, rp, c, v, p, p)


def one_sided_noisy(A, seed: int):
    """the entries above the diagonal only, every fifth one twice, every third value a stored zero, and a full diagonal: the same graph"""
    n, rp, c, v = A
    r = np.repeat(np.arange(n), np.diff(rp))
    keep = r < c
    r, c = r[keep], c[keep].astype(np.int64)
    r, c = np.concatenate([r, r[::5], np.arange(n)]), np.concatenate([c, c[::5], np.arange(n)])
    v = np.where(np.arange(len(r)) % 3 == 0, 0.0, 2.0)
    o = np.random.default_rng(seed).permutation(len(r))  # (unsorted columns as well)
    return csr_from_entries(n, r[o], c[o], v[o])
