// reorder.hip — renumbering on the device, on CDNA4 (gfx950): permutations as objects (spmv_perm_create), the reverse Cuthill-McKee
// ordering of a CSR handle's graph (spmv_perm_rcm), B = P_r A P_c^T as a CSR handle of its own (spmv_csr_permute), a vector permuted
// in one launch (spmv_vec_permute) and the bandwidth and profile of a CSR handle (spmv_csr_bandwidth).  include/spmv_abi.h
// ("reordering") is the specification; tests/rcm_ref.py is the NumPy twin of the ordering, integer for integer.
//
// Convention (that of spmv_symgs_order): order[k] is the old index that takes new position k, inverse[order[k]] = k.
//
// spmv_perm_rcm.
//   Adjacency.  Every off-diagonal entry (i, j) gives the keys (i, j) and (j, i); runs_by_key_pair (sorted_runs.hip) orders them and
//   drops the repeats, so that run_j IS the column array of the pattern of A + A^T without its diagonal, ascending inside a row, and
//   count_i the degrees; their scan is the row pointer.  Everything but order and inverse lives in a device_pool.
//   Breadth first.  cm holds the sequence; mark[w] is INT32_MAX for a vertex nobody reached, -1 for a root (and for a vertex without
//   neighbours) and otherwise the smallest position in cm among the vertices of the level before w's that are adjacent to w.  A level
//   [lo, hi) of cm is advanced by
//     claim   a group of lanes per frontier vertex v at position p: atomicMin(mark + w, p) for its neighbours w - after a plain load
//             that skips every w whose mark is already below p, which is all of a hub's neighbours but the first to arrive.  Positions
//             only grow from level to level, so a vertex reached earlier keeps its mark: no second array says "visited".  An integer
//             minimum does not depend on the order of the atomics.
//     count   the same groups count the neighbours whose mark is p: the children v won;
//     scan    exclusive_scan_i32 over the frontier; the host reads the sum, the size of the next level (the one read per level);
//     fill    the groups write their children at hi + off[k], in adjacency order (ascending index), by ballot and popcount;
//     order   (numbering passes only) the level is ordered by (mark, degree): the fill left it ordered by (mark, index) and the order
//             is stable.  A level of up to kRcmSmallLevel vertices is ranked by one workgroup in LDS, a larger one takes two passes of
//             sort_ids_by_key (degree, then mark - lo).  A level of one vertex is in order.
//   The work of a level is proportional to the edges of its frontier.  The loop over levels is the host's; no workgroup waits for
//   another one.  A root search (George and Liu) runs the same kernels without the ordering step, in the part of cm behind the
//   vertices numbered so far, and puts the marks of what it reached back to INT32_MAX.
//
// spmv_csr_permute.  New row lengths by gather, their scan is B's row pointer; a group of 16 lanes per new row writes, for every
//   entry, its new row, its new column and the entry of A it comes from, in A's stored order; two stable passes of sort_ids_by_key
//   (new column, then new row) order the entries, and one kernel copies column and value (as 64-bit words) through that order.
//   24 bytes of transient memory per entry beside the sort's own buffers.
#include "common.hpp"
#include "reorder_settings.hpp"
#include "solver_host.hpp"
#include "sorted_runs.hpp"

struct spmv_perm
{
    spmv_ctx* ctx     = nullptr;
    int64_t   n       = 0;
    int32_t*  order   = nullptr;  // [n] on the device
    int32_t*  inverse = nullptr;  // [n] on the device
    // what spmv_perm_rcm did ("rcm_*"; 0 for a permutation made by spmv_perm_create)
    int64_t isolated = 0, components = 0, levels = 0, bfs = 0, launches = 0, transient_bytes = 0;
};

namespace spmv
{
namespace
{
constexpr int32_t kUnreached = INT32_MAX;

// ---- permutations -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void perm_fill_kernel(int64_t n, int32_t value, int32_t* __restrict__ p)
{
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += (int64_t)gridDim.x * kBlock) p[k] = value;
}

// inverse[v] = the smallest k with order[k] = v (inverse starts at INT32_MAX)
__global__ __launch_bounds__(kBlock) void perm_invert_kernel(int64_t n, const int32_t* __restrict__ order, int32_t* __restrict__ inverse)
{
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += (int64_t)gridDim.x * kBlock)
    {
        const int32_t v = order[k];
        if (v >= 0 && v < n) atomicMin(inverse + v, (int32_t)k);
    }
}

// bad = the smallest k whose order[k] is out of range or stands at an earlier position already
__global__ __launch_bounds__(kBlock) void perm_check_kernel(int64_t n, const int32_t* __restrict__ order, const int32_t* __restrict__ inverse,
                                                           int32_t* __restrict__ bad)
{
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += (int64_t)gridDim.x * kBlock)
    {
        const int32_t v = order[k];
        if (v < 0 || v >= n || inverse[v] != (int32_t)k) atomicMin(bad, (int32_t)k);
    }
}

// BACK = false: dst[k] = src[order[k]] (the index loads and the stores are contiguous); BACK = true: dst[order[k]] = src[k] (the index
// loads and the loads).  64-bit words: no bit of a value is looked at.
template <bool BACK>
__global__ __launch_bounds__(kBlock) void vec_permute_kernel(int64_t n, const int32_t* __restrict__ order, const unsigned long long* __restrict__ src,
                                                            unsigned long long* __restrict__ dst)
{
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += (int64_t)gridDim.x * kBlock)
    {
        const int32_t o = order[k];
        if constexpr (BACK)
            dst[o] = src[k];
        else
            dst[k] = src[o];
    }
}

// ---- kernels that walk the rows of A: kRowLanes lanes a row, adjacent lanes on adjacent entries ----------------------------------------
constexpr int kRowLanes = 16;

// bandwidth and profile: out[0] = max |i - j|, out[1] = sum over the non-empty rows of max(0, i - min j)
__global__ __launch_bounds__(kBlock) void csr_bandwidth_kernel(int64_t m, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                              unsigned long long* __restrict__ out)
{
    const int          l  = threadIdx.x % kRowLanes;
    unsigned long long bw = 0, prof = 0;
    for (int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kRowLanes; i < m; i += (int64_t)gridDim.x * (kBlock / kRowLanes))
    {
        const int end = row_ptr[i + 1];
        int64_t   lo  = i;
        for (int e = row_ptr[i] + l; e < end; e += kRowLanes)
        {
            const int64_t j = col[e], d = j > i ? j - i : i - j;
            bw = d > (int64_t)bw ? (unsigned long long)d : bw;
            lo = j < lo ? j : lo;
        }
        for (int off = kRowLanes / 2; off > 0; off >>= 1)  // (the lanes of a group leave the row together)
        {
            const long long o = __shfl_xor((long long)lo, off);
            lo                = o < lo ? o : lo;
        }
        if (l == 0) prof += (unsigned long long)(i - lo);
    }
    for (int off = 32; off > 0; off >>= 1)
    {
        const unsigned long long b = __shfl_xor(bw, off);
        bw = b > bw ? b : bw;
        prof += __shfl_xor(prof, off);
    }
    if ((threadIdx.x & 63) == 0)  // (integer maximum and sum: the order does not matter)
    {
        if (bw) atomicMax(out, bw);
        if (prof) atomicAdd(out + 1, prof);
    }
}

// ---- the adjacency ------------------------------------------------------------------------------------------------------------------
// cnt[i] = the off-diagonal entries of row i, cnt[n] = 0
__global__ __launch_bounds__(kBlock) void rcm_offdiag_count_kernel(int64_t n, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                                  int32_t* __restrict__ cnt)
{
    const int l = threadIdx.x % kRowLanes;
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt[n] = 0;
    for (int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kRowLanes; i < n; i += (int64_t)gridDim.x * (kBlock / kRowLanes))
    {
        int       c   = 0;
        const int end = row_ptr[i + 1];
        for (int e = row_ptr[i] + l; e < end; e += kRowLanes) c += col[e] != (int32_t)i ? 1 : 0;
        for (int off = kRowLanes / 2; off > 0; off >>= 1) c += __shfl_xor(c, off);
        if (l == 0) cnt[i] = c;
    }
}

// the keys (i, j) and (j, i) of every off-diagonal entry, row i's from 2 first[i] on in stored order (ballot and popcount, as the
// fill of a level); total = the keys in all bounds every store
__global__ __launch_bounds__(kBlock) void rcm_keys_kernel(int64_t n, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                         const int32_t* __restrict__ first, int64_t total, int32_t* __restrict__ key_i,
                                                         int32_t* __restrict__ key_j)
{
    const int                l     = threadIdx.x % kRowLanes;
    const int                shift = (threadIdx.x % kWave) - l;  // the group's first lane in its wavefront
    const unsigned long long ones  = ~0ull >> (64 - kRowLanes);
    for (int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kRowLanes; i < n; i += (int64_t)gridDim.x * (kBlock / kRowLanes))
    {
        int64_t   at  = 2 * (int64_t)first[i];
        const int end = row_ptr[i + 1];
        for (int e0 = row_ptr[i]; e0 < end; e0 += kRowLanes)  // (the lanes of a group make the same trips)
        {
            const int                e    = e0 + l;
            const int32_t            j    = e < end ? col[e] : (int32_t)i;
            const bool               mine = j != (int32_t)i;
            const unsigned long long grp  = (__ballot(mine) >> shift) & ones;
            const int64_t            to   = at + 2 * (int64_t)__popcll(grp & ((1ull << l) - 1));
            if (mine && to + 1 < total)
            {
                key_i[to]     = (int32_t)i;
                key_j[to]     = j;
                key_i[to + 1] = j;
                key_j[to + 1] = (int32_t)i;
            }
            at += 2 * (int64_t)__popcll(grp);
        }
    }
}

// mark[i] = -1 for a vertex without neighbours, INT32_MAX for the others; counter += the former
__global__ __launch_bounds__(kBlock) void rcm_init_kernel(int64_t n, const int32_t* __restrict__ deg, int32_t* __restrict__ mark, int32_t* __restrict__ counter)
{
    int mine = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
    {
        const bool alone = deg[i] == 0;
        mark[i]          = alone ? -1 : kUnreached;
        mine += alone ? 1 : 0;
    }
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(counter, mine);
}

// ---- roots --------------------------------------------------------------------------------------------------------------------------
// One workgroup walks bydeg (the vertices by (degree, index)) from `cursor` on, 256 at a time, and stops at the first vertex nobody
// reached: out[0] = its place in bydeg (n: none), out[1] = the vertex.  The cursor only moves forward, so all calls of an ordering
// together read bydeg once.  Every barrier is reached by the whole workgroup: the loop's bounds and its exit are uniform.
__global__ __launch_bounds__(kBlock) void rcm_next_root_kernel(int64_t n, int64_t cursor, const int32_t* __restrict__ bydeg, const int32_t* __restrict__ mark,
                                                              int32_t* __restrict__ out)
{
    __shared__ int s_first;
    int            found = (int)n;
    for (int64_t base = cursor; base < n; base += kBlock)
    {
        if (threadIdx.x == 0) s_first = INT32_MAX;
        __syncthreads();
        const int64_t q = base + threadIdx.x;
        if (q < n && mark[bydeg[q]] == kUnreached) atomicMin(&s_first, (int)q);
        __syncthreads();
        const int first = s_first;
        __syncthreads();
        if (first != INT32_MAX)
        {
            found = first;
            break;
        }
    }
    if (threadIdx.x == 0)
    {
        out[0] = found;
        out[1] = found < n ? bydeg[found] : -1;
    }
}

__global__ void rcm_seed_kernel(int32_t root, int64_t at, int32_t* __restrict__ cm, int32_t* __restrict__ mark)
{
    if (blockIdx.x == 0 && threadIdx.x == 0)
    {
        cm[at]     = root;
        mark[root] = -1;
    }
}

// out = the smallest (degree << 32 | vertex) over cm[from, from + count)
__global__ __launch_bounds__(kBlock) void rcm_min_degree_kernel(int64_t from, int64_t count, int64_t n, const int32_t* __restrict__ cm, const int32_t* __restrict__ deg,
                                                               unsigned long long* __restrict__ out)
{
    unsigned long long best = ~0ull;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < count; t += (int64_t)gridDim.x * kBlock)
    {
        const int32_t w = cm[from + t];
        if (w < 0 || w >= n) continue;  // (never)
        const unsigned long long k = ((unsigned long long)(uint32_t)deg[w] << 32) | (uint32_t)w;
        best                       = k < best ? k : best;
    }
    for (int off = 32; off > 0; off >>= 1)
    {
        const unsigned long long b = __shfl_xor(best, off);
        best                       = b < best ? b : best;
    }
    if ((threadIdx.x & 63) == 0 && best != ~0ull) atomicMin(out, best);
}

// mark[cm[from + t]] = INT32_MAX: a root search gives back what it reached
__global__ __launch_bounds__(kBlock) void rcm_unmark_kernel(int64_t from, int64_t count, int64_t n, const int32_t* __restrict__ cm, int32_t* __restrict__ mark)
{
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < count; t += (int64_t)gridDim.x * kBlock)
    {
        const int32_t w = cm[from + t];
        if (w >= 0 && w < n) mark[w] = kUnreached;
    }
}

// ---- one level ----------------------------------------------------------------------------------------------------------------------
// the claim pass: LANES lanes per frontier vertex cm[lo + k], k < f
template <int LANES>
__global__ __launch_bounds__(kBlock) void rcm_claim_kernel(int64_t f, int64_t lo, int64_t n, const int32_t* __restrict__ cm, const int32_t* __restrict__ adj_rp,
                                                          const int32_t* __restrict__ adj_col, int32_t* __restrict__ mark)
{
    const int l = threadIdx.x % LANES;
    for (int64_t k = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES; k < f; k += (int64_t)gridDim.x * (kBlock / LANES))
    {
        const int32_t v = cm[lo + k], p = (int32_t)(lo + k);
        if (v < 0 || v >= n) continue;  // (never: cm holds vertices; no load may leave the arrays)
        const int     end = adj_rp[v + 1];
        for (int e = adj_rp[v] + l; e < end; e += LANES)
        {
            const int32_t w = adj_col[e];
            if (mark[w] > p) atomicMin(mark + w, p);  // (a mark only falls: a stale load costs an atomic, never a claim)
        }
    }
}

// cnt[k] = the neighbours of cm[lo + k] whose mark is lo + k, cnt[f] = 0
template <int LANES>
__global__ __launch_bounds__(kBlock) void rcm_count_kernel(int64_t f, int64_t lo, int64_t n, const int32_t* __restrict__ cm, const int32_t* __restrict__ adj_rp,
                                                          const int32_t* __restrict__ adj_col, const int32_t* __restrict__ mark, int32_t* __restrict__ cnt)
{
    const int l = threadIdx.x % LANES;
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt[f] = 0;
    for (int64_t k = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES; k < f; k += (int64_t)gridDim.x * (kBlock / LANES))
    {
        const int32_t v = cm[lo + k], p = (int32_t)(lo + k);
        if (v < 0 || v >= n)  // (never: cm holds vertices; no load may leave the arrays)
        {
            if (l == 0) cnt[k] = 0;
            continue;
        }
        const int     end = adj_rp[v + 1];
        int           c   = 0;
        for (int e = adj_rp[v] + l; e < end; e += LANES) c += mark[adj_col[e]] == p ? 1 : 0;
        for (int off = LANES / 2; off > 0; off >>= 1) c += __shfl_xor(c, off);
        if (l == 0) cnt[k] = c;
    }
}

// cm[hi + off[k] ...] = those neighbours, in adjacency order; n bounds every store
template <int LANES>
__global__ __launch_bounds__(kBlock) void rcm_fill_kernel(int64_t f, int64_t lo, int64_t hi, int64_t n, int32_t* __restrict__ cm, const int32_t* __restrict__ adj_rp,
                                                         const int32_t* __restrict__ adj_col, const int32_t* __restrict__ mark, const int32_t* __restrict__ off)
{
    const int                l     = threadIdx.x % LANES;
    const int                shift = (threadIdx.x % kWave) - l;  // the group's first lane in its wavefront
    const unsigned long long ones  = ~0ull >> (64 - LANES);
    for (int64_t k = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES; k < f; k += (int64_t)gridDim.x * (kBlock / LANES))
    {
        const int32_t v = cm[lo + k], p = (int32_t)(lo + k);
        if (v < 0 || v >= n) continue;  // (never: cm holds vertices; no load may leave the arrays)
        const int     end = adj_rp[v + 1];
        int64_t       at  = hi + off[k];
        for (int e0 = adj_rp[v]; e0 < end; e0 += LANES)  // (the lanes of a group make the same trips)
        {
            const int                e    = e0 + l;
            const int32_t            w    = e < end ? adj_col[e] : -1;
            const bool               mine = w >= 0 && mark[w] == p;
            const unsigned long long grp  = (__ballot(mine) >> shift) & ones;
            const int64_t            to   = at + __popcll(grp & ((1ull << l) - 1));
            if (mine && to < n) cm[to] = w;
            at += __popcll(grp);
        }
    }
}

// a level of c <= kRcmSmallLevel vertices at cm[hi ...], ordered by (mark, degree, place) by one workgroup: every vertex counts those before it
__global__ __launch_bounds__(kBlock) void rcm_order_small_kernel(int c, int64_t lo, int64_t hi, int64_t n, int32_t* __restrict__ cm, const int32_t* __restrict__ mark,
                                                                const int32_t* __restrict__ deg)
{
    __shared__ int32_t            s_w[kRcmSmallLevel];
    __shared__ unsigned long long s_key[kRcmSmallLevel];
    for (int t = threadIdx.x; t < c; t += kBlock)
    {
        const int32_t w  = cm[hi + t];
        const bool    ok = w >= 0 && w < n;  // (always)
        s_w[t]           = w;
        s_key[t]         = ok ? ((unsigned long long)(uint32_t)(mark[w] - (int32_t)lo) << 32) | (uint32_t)deg[w] : ~0ull;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < c; t += kBlock)
    {
        const unsigned long long key = s_key[t];
        int                      rank = 0;
        for (int u = 0; u < c; ++u)
        {
            const unsigned long long other = s_key[u];
            rank += (other < key || (other == key && u < t)) ? 1 : 0;
        }
        cm[hi + rank] = s_w[t];  // (ranks are a permutation of 0 .. c-1; every vertex was read before the barrier)
    }
}

// the two keys of a large level: key_p[t] = mark - lo, key_d[t] = degree
__global__ __launch_bounds__(kBlock) void rcm_level_keys_kernel(int64_t c, int64_t lo, int64_t hi, int64_t n, const int32_t* __restrict__ cm, const int32_t* __restrict__ mark,
                                                               const int32_t* __restrict__ deg, int32_t* __restrict__ key_p, int32_t* __restrict__ key_d)
{
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < c; t += (int64_t)gridDim.x * kBlock)
    {
        const int32_t w  = cm[hi + t];
        const bool    ok = w >= 0 && w < n;  // (always)
        key_p[t]         = ok ? mark[w] - (int32_t)lo : 0;
        key_d[t]         = ok ? deg[w] : 0;
    }
}

// out[t] = src[a[t]], or src[a[b[t]]] where b is given
__global__ __launch_bounds__(kBlock) void rcm_gather_kernel(int64_t c, const int32_t* __restrict__ src, const int32_t* __restrict__ a, const int32_t* __restrict__ b,
                                                           int32_t* __restrict__ out)
{
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < c; t += (int64_t)gridDim.x * kBlock) out[t] = src[a[b ? b[t] : t]];
}

// order[k] = cm[n - 1 - k], inverse[order[k]] = k
__global__ __launch_bounds__(kBlock) void rcm_reverse_kernel(int64_t n, const int32_t* __restrict__ cm, int32_t* __restrict__ order, int32_t* __restrict__ inverse)
{
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += (int64_t)gridDim.x * kBlock)
    {
        const int32_t v = cm[n - 1 - k];
        order[k]        = v;
        if (v >= 0 && v < n) inverse[v] = (int32_t)k;
    }
}

// ---- spmv_csr_permute ---------------------------------------------------------------------------------------------------------------
// len[k] = the length of row (rows ? rows[k] : k) of A, len[m] = 0
__global__ __launch_bounds__(kBlock) void permute_row_len_kernel(int64_t m, const int32_t* __restrict__ rows, const int32_t* __restrict__ a_rp, int32_t* __restrict__ len)
{
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k <= m; k += (int64_t)gridDim.x * kBlock)
    {
        int v = 0;
        if (k < m)
        {
            const int32_t i = rows ? rows[k] : (int32_t)k;
            v               = a_rp[i + 1] - a_rp[i];
        }
        len[k] = v;
    }
}

// the entries of new row k in A's stored order: their new row, their new column, the entry of A they are; 16 lanes a row
constexpr int kPermuteLanes = kRowLanes;
__global__ __launch_bounds__(kBlock) void permute_keys_kernel(int64_t m, const int32_t* __restrict__ rows, const int32_t* __restrict__ inv_cols,
                                                             const int32_t* __restrict__ a_rp, const int32_t* __restrict__ a_col, const int32_t* __restrict__ b_rp,
                                                             int32_t* __restrict__ key_i, int32_t* __restrict__ key_j, int32_t* __restrict__ from)
{
    const int l = threadIdx.x % kPermuteLanes;
    for (int64_t k = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kPermuteLanes; k < m; k += (int64_t)gridDim.x * (kBlock / kPermuteLanes))
    {
        const int32_t i   = rows ? rows[k] : (int32_t)k;
        const int     src = a_rp[i], len = a_rp[i + 1] - src;
        const int64_t dst = b_rp[k];
        for (int t = l; t < len; t += kPermuteLanes)
        {
            const int32_t j = a_col[src + t];
            key_i[dst + t]  = (int32_t)k;
            key_j[dst + t]  = inv_cols ? inv_cols[j] : j;
            from[dst + t]   = src + t;
        }
    }
}

// b_col[p] and b_val[p] of the p-th entry in (new row, new column, stored order): it is the entry ids1[ids2[p]] of the keys
__global__ __launch_bounds__(kBlock) void permute_place_kernel(int64_t nnz, const int32_t* __restrict__ ids1, const int32_t* __restrict__ ids2,
                                                              const int32_t* __restrict__ key_j, const int32_t* __restrict__ from,
                                                              const unsigned long long* __restrict__ a_val, int32_t* __restrict__ b_col,
                                                              unsigned long long* __restrict__ b_val)
{
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * kBlock)
    {
        const int32_t e = ids1[ids2[p]];
        b_col[p]        = key_j[e];
        b_val[p]        = a_val[from[e]];
    }
}

inline int group_grid(int64_t items, int lanes) { return (int)std::max<int64_t>(1, std::min<int64_t>(kMaxGrid, ceil_div(items, kBlock / lanes))); }

// ---- the ordering's host side -------------------------------------------------------------------------------------------------------
struct rcm_run
{
    spmv_ctx*      ctx;
    const char*    who;
    int64_t        n;
    int            lanes, deg_bits;
    const int32_t *adj_rp, *adj_col, *deg;
    int32_t *      mark, *cm, *cnt, *off, *key_p, *key_d, *ids1, *ids2, *tmp;
    int64_t        launches = 0, levels = 0, bfs = 0;
};

template <int LANES>
int rcm_level_launches(rcm_run& R, int64_t f, int64_t lo)
{
    hipStream_t s = R.ctx->stream;
    const dim3  grid((unsigned)group_grid(f, LANES));
    hipLaunchKernelGGL(rcm_claim_kernel<LANES>, grid, dim3(kBlock), 0, s, f, lo, R.n, (const int32_t*)R.cm, R.adj_rp, R.adj_col, R.mark);
    hipLaunchKernelGGL(rcm_count_kernel<LANES>, grid, dim3(kBlock), 0, s, f, lo, R.n, (const int32_t*)R.cm, R.adj_rp, R.adj_col, (const int32_t*)R.mark, R.cnt);
    return hip_step(hipGetLastError(), R.who, "a level's claim and count launches");
}

template <int LANES>
int rcm_fill_launch(rcm_run& R, int64_t f, int64_t lo, int64_t hi)
{
    hipLaunchKernelGGL(rcm_fill_kernel<LANES>, dim3((unsigned)group_grid(f, LANES)), dim3(kBlock), 0, R.ctx->stream, f, lo, hi, R.n, R.cm, R.adj_rp, R.adj_col,
                       (const int32_t*)R.mark, (const int32_t*)R.off);
    return hip_step(hipGetLastError(), R.who, "a level's fill launch");
}

// the level [hi, hi + c) behind the frontier [lo, hi), ordered by (mark, degree); the fill left it in (mark, index) order
int rcm_order_level(rcm_run& R, int64_t lo, int64_t hi, int64_t c)
{
    hipStream_t s = R.ctx->stream;
    if (c <= kRcmSmallLevel)
    {
        hipLaunchKernelGGL(rcm_order_small_kernel, dim3(1), dim3(kBlock), 0, s, (int)c, lo, hi, R.n, R.cm, (const int32_t*)R.mark, R.deg);
        R.launches += 1;
        return hip_step(hipGetLastError(), R.who, "a small level's ordering launch");
    }
    const dim3 grid((unsigned)stream_grid(c));
    hipLaunchKernelGGL(rcm_level_keys_kernel, grid, dim3(kBlock), 0, s, c, lo, hi, R.n, (const int32_t*)R.cm, (const int32_t*)R.mark, R.deg, R.key_p, R.key_d);
    SPMV_TRY(sort_ids_by_key(R.ctx, R.key_d, c, R.deg_bits, R.ids1));
    hipLaunchKernelGGL(rcm_gather_kernel, grid, dim3(kBlock), 0, s, c, (const int32_t*)R.key_p, (const int32_t*)R.ids1, (const int32_t*)nullptr, R.cnt);
    SPMV_TRY(sort_ids_by_key(R.ctx, R.cnt, c, key_bits(hi - lo), R.ids2));
    hipLaunchKernelGGL(rcm_gather_kernel, grid, dim3(kBlock), 0, s, c, (const int32_t*)(R.cm + hi), (const int32_t*)R.ids1, (const int32_t*)R.ids2, R.tmp);
    SPMV_TRY(hip_step(hipGetLastError(), R.who, "a large level's ordering launches"));
    SPMV_TRY(hip_step(hipMemcpyAsync(R.cm + hi, R.tmp, sizeof(int32_t) * (size_t)c, hipMemcpyDeviceToDevice, s), R.who, "a large level's copy"));
    R.launches += 6;
    return SPMV_OK;
}

// The level structure of `root` over the vertices nobody reached, written to cm from `base` on; ordered: a numbering pass.
// *nlev levels (the root's included), the last one at [*last, *end).
int rcm_bfs(rcm_run& R, int32_t root, int64_t base, bool ordered, int64_t* nlev, int64_t* last, int64_t* end)
{
    hipLaunchKernelGGL(rcm_seed_kernel, dim3(1), dim3(kWave), 0, R.ctx->stream, root, base, R.cm, R.mark);
    R.launches += 1;
    R.bfs += 1;
    int64_t lo = base, hi = base + 1, levels = 1;
    for (;;)
    {
        const int64_t f = hi - lo;
        SPMV_TRY(R.lanes == 4 ? rcm_level_launches<4>(R, f, lo) : (R.lanes == 16 ? rcm_level_launches<16>(R, f, lo) : rcm_level_launches<64>(R, f, lo)));
        SPMV_TRY(exclusive_scan_i32(R.ctx, R.cnt, R.off, f + 1));
        int32_t c = 0;
        SPMV_TRY(read_scalars(R.ctx, &c, R.off + f, sizeof(c), R.who));  // the one read of a level: the size of the next
        R.launches += 3;
        if (c == 0) break;
        SPMV_REQUIRE(c > 0 && hi + c <= R.n, "%s: a level of %d vertices behind %lld of %lld", R.who, c, (long long)hi, (long long)R.n);
        SPMV_TRY(R.lanes == 4 ? rcm_fill_launch<4>(R, f, lo, hi) : (R.lanes == 16 ? rcm_fill_launch<16>(R, f, lo, hi) : rcm_fill_launch<64>(R, f, lo, hi)));
        R.launches += 1;
        if (ordered && c > 1) SPMV_TRY(rcm_order_level(R, lo, hi, c));
        lo = hi;
        hi += c;
        ++levels;
    }
    *nlev = levels;
    *last = lo;
    *end  = hi;
    return SPMV_OK;
}

int rcm_unmark(rcm_run& R, int64_t from, int64_t count)
{
    hipLaunchKernelGGL(rcm_unmark_kernel, dim3((unsigned)stream_grid(count)), dim3(kBlock), 0, R.ctx->stream, from, count, R.n, (const int32_t*)R.cm, R.mark);
    R.launches += 1;
    return hip_step(hipGetLastError(), R.who, "the unmarking launch");
}

void perm_free(spmv_perm* p)
{
    if (!p) return;
    if (p->order) (void)hipFree(p->order);
    if (p->inverse) (void)hipFree(p->inverse);
    delete p;
}

// a permutation of n with its two arrays on the device (none for n = 0, where the device is not touched)
int perm_alloc(spmv_ctx* ctx, int64_t n, const char* who, spmv_perm** out)
{
    spmv_perm* p = new (std::nothrow) spmv_perm();
    if (!p) SPMV_FAIL(SPMV_ERR_ALLOC, "%s: out of host memory", who);
    p->ctx = ctx;
    p->n   = n;
    if (n > 0 && (hipMalloc(&p->order, sizeof(int32_t) * (size_t)n) != hipSuccess || hipMalloc(&p->inverse, sizeof(int32_t) * (size_t)n) != hipSuccess))
    {
        (void)hipGetLastError();
        perm_free(p);
        SPMV_FAIL(SPMV_ERR_ALLOC, "%s: out of device memory for a permutation of %lld", who, (long long)n);
    }
    *out = p;
    return SPMV_OK;
}

int perm_rcm_build(spmv_ctx* ctx, const spmv_mat* A, spmv_perm* P)
{
    const char* const who = "spmv_perm_rcm";
    hipStream_t       s   = ctx->stream;
    const int64_t     n   = A->nrow;
    device_pool       pool(ctx, who);
    rcm_run           R{};
    R.ctx = ctx;
    R.who = who;
    R.n   = n;
    int32_t *cnt, *off;
    SPMV_TRY(pool.get(cnt, (size_t)n + 1));
    SPMV_TRY(pool.get(off, (size_t)n + 1));
    SPMV_TRY(pool.get(R.cm, (size_t)n));
    R.cnt = cnt;
    R.off = off;
    // the adjacency
    hipLaunchKernelGGL(rcm_offdiag_count_kernel, dim3((unsigned)group_grid(n, kRowLanes)), dim3(kBlock), 0, s, n, A->a, A->b, cnt);
    SPMV_TRY(hip_step(hipGetLastError(), who, "the off-diagonal count's launch"));
    SPMV_TRY(exclusive_scan_i32(ctx, cnt, off, n + 1));
    int32_t offdiag = 0;
    SPMV_TRY(read_scalars(ctx, &offdiag, off + n, sizeof(offdiag), who));
    R.launches += 2;
    const int64_t total = 2 * (int64_t)offdiag;
    if (total > (int64_t)INT32_MAX)
        SPMV_FAIL(SPMV_ERR_UNSUPPORTED, "%s: the symmetrised adjacency takes %lld keys, its ids are int32 (at most %d)", who, (long long)total, INT32_MAX);
    int64_t isolated = n;
    if (total > 0)
    {
        int32_t *key_i, *key_j, *adj_rp, *bydeg, *counter;
        SPMV_TRY(pool.get(key_i, (size_t)total));
        SPMV_TRY(pool.get(key_j, (size_t)total));
        hipLaunchKernelGGL(rcm_keys_kernel, dim3((unsigned)group_grid(n, kRowLanes)), dim3(kBlock), 0, s, n, A->a, A->b, (const int32_t*)off, total, key_i, key_j);
        SPMV_TRY(hip_step(hipGetLastError(), who, "the keys' launch"));
        key_runs kr;
        SPMV_TRY(runs_by_key_pair(ctx, pool, who, key_i, n, key_j, n, total, &kr));
        SPMV_TRY(pool.get(adj_rp, (size_t)n + 1));
        SPMV_TRY(exclusive_scan_i32(ctx, kr.count_i, adj_rp, n + 1));
        R.adj_rp  = adj_rp;
        R.adj_col = kr.run_j;   // (the runs stand in (i, j) order: this is the column array)
        R.deg     = kr.count_i;
        int32_t maxdeg = 0;
        SPMV_TRY(reduce_max_i32(ctx, kr.count_i, n, &maxdeg));
        R.deg_bits = key_bits((int64_t)maxdeg + 1);
        SPMV_TRY(pool.get(R.mark, (size_t)n));
        SPMV_TRY(pool.get(bydeg, (size_t)n));
        SPMV_TRY(pool.get(counter, (size_t)4));
        SPMV_TRY(pool.get(R.key_p, (size_t)n));
        SPMV_TRY(pool.get(R.key_d, (size_t)n));
        SPMV_TRY(pool.get(R.ids1, (size_t)n));
        SPMV_TRY(pool.get(R.ids2, (size_t)n));
        SPMV_TRY(pool.get(R.tmp, (size_t)n));
        unsigned long long* slot;
        SPMV_TRY(pool.get(slot, (size_t)1));
        SPMV_TRY(hip_step(hipMemsetAsync(counter, 0, sizeof(int32_t) * 4, s), who, "clearing the counter"));
        hipLaunchKernelGGL(rcm_init_kernel, dim3((unsigned)stream_grid(n)), dim3(kBlock), 0, s, n, R.deg, R.mark, counter);
        SPMV_TRY(hip_step(hipGetLastError(), who, "the marks' launch"));
        SPMV_TRY(sort_ids_by_key(ctx, R.deg, n, R.deg_bits, bydeg));  // the vertices by (degree, index)
        int32_t alone = 0;
        SPMV_TRY(read_scalars(ctx, &alone, counter, sizeof(alone), who));
        SPMV_REQUIRE(alone >= 0 && alone < n, "%s: %d of %lld vertices without neighbours beside %lld keys", who, alone, (long long)n, (long long)total);
        isolated = alone;
        R.launches += 14;  // (keys, the runs' two sorts, two gathers, heads, scan and segments, the scan, the maximum, the marks, the sort, the copy)
        R.lanes = rcm_lanes((double)kr.runs / (double)(n - isolated));
        // the vertices without neighbours come first, in ascending index: the head of bydeg
        SPMV_TRY(hip_step(hipMemcpyAsync(R.cm, bydeg, sizeof(int32_t) * (size_t)isolated, hipMemcpyDeviceToDevice, s), who, "the copy of the lone vertices"));
        int64_t numbered = isolated, cursor = isolated;
        while (numbered < n)
        {
            int32_t found[2] = {0, 0};
            hipLaunchKernelGGL(rcm_next_root_kernel, dim3(1), dim3(kBlock), 0, s, n, cursor, (const int32_t*)bydeg, (const int32_t*)R.mark, counter);
            SPMV_TRY(hip_step(hipGetLastError(), who, "the root's launch"));
            SPMV_TRY(read_scalars(ctx, found, counter, sizeof(found), who));
            R.launches += 1;
            SPMV_REQUIRE(found[0] >= cursor && found[0] < n && found[1] >= 0 && found[1] < n, "%s: no root behind place %lld with %lld of %lld vertices numbered", who,
                         (long long)cursor, (long long)numbered, (long long)n);
            cursor       = (int64_t)found[0] + 1;
            int32_t root = found[1];
            P->components += 1;
            // George and Liu: the vertex of smallest (degree, index) in the last level takes over while its structure is deeper
            int64_t depth = 0, last = 0, end = 0;
            SPMV_TRY(rcm_bfs(R, root, numbered, false, &depth, &last, &end));
            for (int rep = 0; rep < kRcmRootRepeats; ++rep)
            {
                SPMV_TRY(hip_step(hipMemsetAsync(slot, 0xFF, sizeof(unsigned long long), s), who, "clearing the candidate"));
                hipLaunchKernelGGL(rcm_min_degree_kernel, dim3((unsigned)stream_grid(end - last)), dim3(kBlock), 0, s, last, end - last, n, (const int32_t*)R.cm, R.deg, slot);
                SPMV_TRY(hip_step(hipGetLastError(), who, "the candidate's launch"));
                unsigned long long best = 0;
                SPMV_TRY(read_scalars(ctx, &best, slot, sizeof(best), who));
                R.launches += 1;
                const int64_t cand = (int64_t)(best & 0xFFFFFFFFull);
                SPMV_REQUIRE(best != ~0ull && cand < n, "%s: no candidate in a last level of %lld", who, (long long)(end - last));
                SPMV_TRY(rcm_unmark(R, numbered, end - numbered));
                int64_t d2 = 0, l2 = 0, e2 = 0;
                SPMV_TRY(rcm_bfs(R, (int32_t)cand, numbered, false, &d2, &l2, &e2));
                SPMV_REQUIRE(e2 == end, "%s: two level structures of one component hold %lld and %lld vertices", who, (long long)(end - numbered), (long long)(e2 - numbered));
                if (d2 <= depth) break;
                root  = (int32_t)cand;
                depth = d2;
                last  = l2;
            }
            SPMV_TRY(rcm_unmark(R, numbered, end - numbered));
            SPMV_TRY(rcm_bfs(R, root, numbered, true, &depth, &last, &end));
            R.levels += depth;
            numbered = end;
        }
    }
    else
    {
        // no edge at all: cm is 0 .. n-1
        SPMV_TRY(sort_ids_by_key(ctx, cnt, n, 1, R.cm));  // (all keys 0: the ids in ascending order)
        R.launches += 1;
    }
    hipLaunchKernelGGL(rcm_reverse_kernel, dim3((unsigned)stream_grid(n)), dim3(kBlock), 0, s, n, (const int32_t*)R.cm, P->order, P->inverse);
    SPMV_TRY(hip_step(hipGetLastError(), who, "the reversal's launch"));
    SPMV_TRY(hip_step(hipStreamSynchronize(s), who, "waiting for the ordering"));
    R.launches += 1;
    P->isolated        = isolated;
    P->levels          = R.levels;
    P->bfs             = R.bfs;
    P->launches        = R.launches;
    P->transient_bytes = (int64_t)pool.bytes;
    return SPMV_OK;
}

// a CSR handle that holds the whole matrix with its arrays, on this context (the refusals of spmv_csr_transpose)
int check_csr_whole(const spmv_ctx* ctx, const spmv_mat* A, const char* who) { return csr_transpose_check(ctx, A, who); }

int check_perm_for(const spmv_ctx* ctx, const spmv_perm* p, const char* name, int64_t n, const char* of, const char* who)
{
    if (!p) return SPMV_OK;
    SPMV_REQUIRE(p->ctx == ctx, "%s: the permutation of the %s belongs to another context", who, name);
    SPMV_REQUIRE(p->n == n, "%s: the permutation of the %s has %lld entries, A has %lld %s", who, name, (long long)p->n, (long long)n, of);
    return SPMV_OK;
}

int csr_permute(spmv_ctx* ctx, const spmv_mat* A, const spmv_perm* rows, const spmv_perm* cols, spmv_mat** out)
{
    const char* const who = "spmv_csr_permute";
    hipStream_t       s   = ctx->stream;
    const int64_t     m = A->nrow, nnz = A->nnz;
    device_pool       pool(ctx, who);
    int32_t*          len;
    SPMV_TRY(pool.get(len, (size_t)m + 1));
    spmv_mat* B = nullptr;
    SPMV_TRY(mat_alloc(ctx, SPMV_FMT_CSR, A->nrow, A->ncol, nnz, 0, (size_t)m + 1, (size_t)nnz, (size_t)nnz, &B));
    int32_t* const b_rp = const_cast<int32_t*>(B->a);
    int            rc   = SPMV_OK;
    do
    {
        hipLaunchKernelGGL(permute_row_len_kernel, dim3((unsigned)stream_grid(m + 1)), dim3(kBlock), 0, s, m, rows ? (const int32_t*)rows->order : nullptr, A->a, len);
        if ((rc = hip_step(hipGetLastError(), who, "the row lengths' launch")) != SPMV_OK) break;
        if ((rc = exclusive_scan_i32(ctx, len, b_rp, m + 1)) != SPMV_OK) break;
        if (nnz == 0) break;
        int32_t *key_i, *key_j, *from, *ids1, *key_i1, *ids2;
        if ((rc = pool.get(key_i, (size_t)nnz)) != SPMV_OK || (rc = pool.get(key_j, (size_t)nnz)) != SPMV_OK || (rc = pool.get(from, (size_t)nnz)) != SPMV_OK ||
            (rc = pool.get(ids1, (size_t)nnz)) != SPMV_OK || (rc = pool.get(key_i1, (size_t)nnz)) != SPMV_OK || (rc = pool.get(ids2, (size_t)nnz)) != SPMV_OK)
            break;
        hipLaunchKernelGGL(permute_keys_kernel, dim3((unsigned)group_grid(m, kPermuteLanes)), dim3(kBlock), 0, s, m, rows ? (const int32_t*)rows->order : nullptr,
                           cols ? (const int32_t*)cols->inverse : nullptr, A->a, A->b, (const int32_t*)b_rp, key_i, key_j, from);
        if ((rc = hip_step(hipGetLastError(), who, "the keys' launch")) != SPMV_OK) break;
        const dim3 grid((unsigned)stream_grid(nnz));
        if ((rc = sort_ids_by_key(ctx, key_j, nnz, key_bits(A->ncol), ids1)) != SPMV_OK) break;
        hipLaunchKernelGGL(rcm_gather_kernel, grid, dim3(kBlock), 0, s, nnz, (const int32_t*)key_i, (const int32_t*)ids1, (const int32_t*)nullptr, key_i1);
        if ((rc = sort_ids_by_key(ctx, key_i1, nnz, key_bits(m), ids2)) != SPMV_OK) break;
        hipLaunchKernelGGL(permute_place_kernel, grid, dim3(kBlock), 0, s, nnz, (const int32_t*)ids1, (const int32_t*)ids2, (const int32_t*)key_j, (const int32_t*)from,
                           (const unsigned long long*)A->v, const_cast<int32_t*>(B->b), (unsigned long long*)const_cast<double*>(B->v));
        rc = hip_step(hipGetLastError(), who, "the placing launch");
    } while (0);
    if (rc == SPMV_OK) rc = hip_step(hipStreamSynchronize(s), who, "waiting for the permuted matrix");
    B->pb_trial = A->pb_trial;               // ("panel_trial" of the source handle holds for what is built from it)
    if (rc == SPMV_OK) rc = csr_analyse(B);  // the engine's usual selection
    if (rc != SPMV_OK)
    {
        (void)hipStreamSynchronize(s);
        mat_free(B);
        return rc;
    }
    *out = B;
    return SPMV_OK;
}
}  // namespace
}  // namespace spmv

using namespace spmv;

extern "C" {
int spmv_perm_create(spmv_ctx* ctx, int64_t n, const int32_t* order_host, spmv_perm** out)
{
    const char* const who = "spmv_perm_create";
    SPMV_REQUIRE(ctx && out && (order_host || n == 0), "%s: null argument", who);
    SPMV_REQUIRE(n >= 0 && n <= (int64_t)INT32_MAX, "%s: n=%lld, a permutation holds 0 .. %d int32 entries", who, (long long)n, INT32_MAX);
    spmv_perm* p = nullptr;
    if (n == 0)
    {
        SPMV_TRY(perm_alloc(ctx, 0, who, &p));
        *out = p;
        return SPMV_OK;
    }
    SPMV_HIP(hipSetDevice(ctx->device));
    SPMV_TRY(perm_alloc(ctx, n, who, &p));
    hipStream_t s   = ctx->stream;
    int32_t     bad = INT32_MAX;
    int         rc  = SPMV_OK;
    {
        device_pool pool(ctx, who);
        int32_t*    d_bad = nullptr;
        rc                = pool.get(d_bad, 1);
        if (rc == SPMV_OK) rc = hip_step(hipMemcpyAsync(p->order, order_host, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s), who, "the upload");
        if (rc == SPMV_OK) rc = hip_step(hipStreamSynchronize(s), who, "the upload");  // pageable host memory: the caller may free it on return
        if (rc == SPMV_OK)
        {
            const dim3 grid((unsigned)stream_grid(n));
            hipLaunchKernelGGL(perm_fill_kernel, grid, dim3(kBlock), 0, s, n, kUnreached, p->inverse);
            hipLaunchKernelGGL(perm_fill_kernel, dim3(1), dim3(kBlock), 0, s, (int64_t)1, kUnreached, d_bad);
            hipLaunchKernelGGL(perm_invert_kernel, grid, dim3(kBlock), 0, s, n, (const int32_t*)p->order, p->inverse);
            hipLaunchKernelGGL(perm_check_kernel, grid, dim3(kBlock), 0, s, n, (const int32_t*)p->order, (const int32_t*)p->inverse, d_bad);
            rc = hip_step(hipGetLastError(), who, "the inversion's launches");
        }
        if (rc == SPMV_OK) rc = read_scalars(ctx, &bad, d_bad, sizeof(bad), who);
    }
    if (rc == SPMV_OK && bad != kUnreached)
    {
        perm_free(p);
        SPMV_FAIL(SPMV_ERR_INVALID, "%s: not a permutation of 0 .. %lld: position %d holds a value that is out of range or stands at an earlier position", who,
                  (long long)(n - 1), bad);
    }
    if (rc != SPMV_OK)
    {
        perm_free(p);
        return rc;
    }
    *out = p;
    return SPMV_OK;
}

int spmv_perm_rcm(spmv_ctx* ctx, const spmv_mat* A, spmv_perm** out)
{
    const char* const who = "spmv_perm_rcm";
    SPMV_REQUIRE(ctx && A && out, "%s: null argument", who);
    SPMV_TRY(check_csr_whole(ctx, A, who));
    SPMV_REQUIRE(A->nrow == A->ncol, "%s: the matrix is %d x %d, not square", who, A->nrow, A->ncol);
    spmv_perm* p = nullptr;
    if (A->nrow == 0)
    {
        SPMV_TRY(perm_alloc(ctx, 0, who, &p));
        *out = p;
        return SPMV_OK;
    }
    SPMV_HIP(hipSetDevice(ctx->device));
    SPMV_TRY(perm_alloc(ctx, A->nrow, who, &p));
    const int rc = perm_rcm_build(ctx, A, p);  // (its set-up memory is gone when it returns)
    if (rc != SPMV_OK)
    {
        perm_free(p);
        return rc;
    }
    *out = p;
    return SPMV_OK;
}

int spmv_perm_download(const spmv_perm* p, int32_t* order_host, int32_t* inverse_host)
{
    SPMV_REQUIRE(p, "spmv_perm_download: null permutation");
    if (p->n == 0 || (!order_host && !inverse_host)) return SPMV_OK;
    SPMV_HIP(hipSetDevice(p->ctx->device));
    hipStream_t s = p->ctx->stream;
    if (order_host) SPMV_HIP(hipMemcpyAsync(order_host, p->order, sizeof(int32_t) * (size_t)p->n, hipMemcpyDeviceToHost, s));
    if (inverse_host) SPMV_HIP(hipMemcpyAsync(inverse_host, p->inverse, sizeof(int32_t) * (size_t)p->n, hipMemcpyDeviceToHost, s));
    SPMV_HIP(hipStreamSynchronize(s));
    return SPMV_OK;
}

int spmv_perm_info(const spmv_perm* p, const char* name, int64_t* value)
{
    SPMV_REQUIRE(p && name && value, "spmv_perm_info: null argument");
    if (!strcmp(name, "n"))
        *value = p->n;
    else if (!strcmp(name, "rcm_isolated"))
        *value = p->isolated;
    else if (!strcmp(name, "rcm_components"))
        *value = p->components;
    else if (!strcmp(name, "rcm_levels"))
        *value = p->levels;
    else if (!strcmp(name, "rcm_bfs"))
        *value = p->bfs;
    else if (!strcmp(name, "rcm_launches"))
        *value = p->launches;
    else if (!strcmp(name, "rcm_transient_bytes"))
        *value = p->transient_bytes;
    else
        SPMV_FAIL(SPMV_ERR_INVALID, "spmv_perm_info: unknown name '%s'", name);
    return SPMV_OK;
}

int spmv_perm_destroy(spmv_perm* p)
{
    if (!p) return SPMV_OK;
    if (p->order || p->inverse)
    {
        (void)hipSetDevice(p->ctx->device);
        (void)hipStreamSynchronize(p->ctx->stream);  // (spmv_vec_permute is asynchronous)
    }
    perm_free(p);
    return SPMV_OK;
}

int spmv_csr_permute(spmv_ctx* ctx, const spmv_mat* A, const spmv_perm* rows, const spmv_perm* cols, spmv_mat** out_B)
{
    const char* const who = "spmv_csr_permute";
    SPMV_REQUIRE(ctx && A && out_B, "%s: null argument", who);
    SPMV_TRY(check_csr_whole(ctx, A, who));
    SPMV_TRY(check_perm_for(ctx, rows, "rows", A->nrow, "rows", who));
    SPMV_TRY(check_perm_for(ctx, cols, "columns", A->ncol, "columns", who));
    SPMV_HIP(hipSetDevice(ctx->device));
    return csr_permute(ctx, A, rows, cols, out_B);
}

int spmv_vec_permute(spmv_ctx* ctx, const spmv_perm* p, int32_t back, const spmv_vec* src, spmv_vec* dst)
{
    const char* const who = "spmv_vec_permute";
    SPMV_REQUIRE(ctx && p && src && dst, "%s: null argument", who);
    SPMV_REQUIRE(back == 0 || back == 1, "%s: back=%d, must be 0 (dst[k] = src[order[k]]) or 1 (dst[order[k]] = src[k])", who, back);
    SPMV_REQUIRE(p->ctx == ctx, "%s: the permutation belongs to another context", who);
    SPMV_REQUIRE(src->ctx == ctx && dst->ctx == ctx, "%s: %s belongs to another context", who, src->ctx != ctx ? "src" : "dst");
    SPMV_REQUIRE(src->n == p->n && dst->n == p->n, "%s: src has %lld entries and dst %lld, the permutation %lld", who, (long long)src->n, (long long)dst->n,
                 (long long)p->n);
    SPMV_REQUIRE(vectors_disjoint(src, dst), "%s: src and dst must not overlap", who);
    if (p->n == 0) return SPMV_OK;
    SPMV_HIP(hipSetDevice(ctx->device));
    const dim3 grid((unsigned)stream_grid(p->n));
    if (back)
        hipLaunchKernelGGL(vec_permute_kernel<true>, grid, dim3(kBlock), 0, ctx->stream, p->n, (const int32_t*)p->order, (const unsigned long long*)src->d,
                           (unsigned long long*)dst->d);
    else
        hipLaunchKernelGGL(vec_permute_kernel<false>, grid, dim3(kBlock), 0, ctx->stream, p->n, (const int32_t*)p->order, (const unsigned long long*)src->d,
                           (unsigned long long*)dst->d);
    SPMV_HIP(hipGetLastError());
    return SPMV_OK;
}

int spmv_csr_bandwidth(spmv_ctx* ctx, const spmv_mat* A, int64_t* bandwidth, int64_t* profile)
{
    const char* const who = "spmv_csr_bandwidth";
    SPMV_REQUIRE(ctx && A && bandwidth && profile, "%s: null argument", who);
    SPMV_TRY(check_csr_whole(ctx, A, who));
    *bandwidth = 0;
    *profile   = 0;
    if (A->nrow == 0 || A->nnz == 0) return SPMV_OK;
    SPMV_HIP(hipSetDevice(ctx->device));
    device_pool         pool(ctx, who);
    unsigned long long* d = nullptr;
    SPMV_TRY(pool.get(d, (size_t)2));
    SPMV_TRY(hip_step(hipMemsetAsync(d, 0, sizeof(unsigned long long) * 2, ctx->stream), who, "clearing the result"));
    hipLaunchKernelGGL(csr_bandwidth_kernel, dim3((unsigned)group_grid(A->nrow, kRowLanes)), dim3(kBlock), 0, ctx->stream, (int64_t)A->nrow, A->a, A->b, d);
    SPMV_TRY(hip_step(hipGetLastError(), who, "the reduction's launch"));
    unsigned long long h[2] = {0, 0};
    SPMV_TRY(read_scalars(ctx, h, d, sizeof(h), who));
    *bandwidth = (int64_t)h[0];
    *profile   = (int64_t)h[1];
    return SPMV_OK;
}
}  // extern "C"
