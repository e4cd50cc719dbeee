// spgemm.hip — the sparse product C = A B of two CSR handles (spmv_spgemm) and the explicit transpose (spmv_csr_transpose), on the
// device, on CDNA4 (gfx950).  tests/spgemm_ref.py is the NumPy twin of the definition below.
//
// What is computed.  A is m x k, B is k x n; both may hold unsorted columns, duplicates and stored zeros.  C has one entry (i, j)
// for every pair that a stored a_ip and a stored b_pj reach - the pattern is structural - with ascending columns.  The scalar
// products of row i are taken in the order (position of the A entry in row i, position of the B entry in its row); each is
// t = a * b, rounded once, and c_ij is the sum of its t from 0.0, left to right in that order, in plain additions: no fma, no
// atomics on doubles, no tree.  Every method returns the same bytes.
//
// The first step of every method: ub_i = sum over the entries of row i of A of the length of the B row they name (int64), the
// class of the row (spgemm_settings.hpp) and the counters the host reads once: products in all and on the sort path, rows per class.
// The rows are then listed by class (one stable pass of sort_ids_by_key: ascending inside a class).
//
// ROWS.  A class with LANES lanes and CAP products a row: 256 / LANES rows share a workgroup.  The lanes of a row write its
// products into the row's slice of LDS, the key (column << 32 | ordinal of the product in the row) and, under the same ordinal, the
// value t.  The ordinal makes every key distinct, so ANY sort of the keys is the stable sort by column; here a bitonic network over
// the next power of two (the largest among the workgroup's rows, so that its barriers are uniform; the tail holds all-ones keys).
// Only the keys move: 8 bytes an exchange.  Every lane then takes a contiguous stretch of the sorted keys, counts the heads of runs
// of equal columns in it, and the lanes' counts are summed in LDS; a lane adds the run of every head of its stretch left to right,
// reading t through the ordinal.  Two passes: the first stops at the counts (no values are read or multiplied), the host scans them
// into row_ptr, the second fills col and val in place.  No transient global memory per product; 16 bytes of LDS per product.
// Banks (cdna_hip_programming.md 2): keys are read as ds_read_b64, bank (a / 4) % 64 over a 32-lane half; exchange distances of 32
// and more read 32 consecutive keys (256 B: no conflict), the distances below read every other group of j keys (2-way).
//
// SORT.  The rows beyond the largest capacity (every non-empty row under SPMV_SPGEMM_SORT) are expanded in (row, p, q) order into
// key_i (the row's place in the list), key_j (the column) and t; sorted_runs.hip orders them stably by (i, j), marks and counts the
// runs of equal keys, and one lane per run adds its t left to right, straight into C at the run's row.  40 bytes of transient
// global memory per product beside the sort's own buffers; the ids are int32, so more than 2^31 - 1 products on this path are refused.
//
// The transpose.  A's arrays read as COO with rows and columns swapped are A^T: the row of every entry is written out (4 bytes an
// entry, transient) and coo_to_csr (convert.hip) groups by row, stable inside a row - ascending i, equal (j, i) in A's order.
#include "common.hpp"
#include "solver_host.hpp"
#include "sorted_runs.hpp"
#include "spgemm_settings.hpp"

namespace spmv
{
namespace
{
// the counters of one product (unsigned 64-bit, on the device)
enum : int
{
    kCntProducts     = 0,  // scalar products in all
    kCntSortProducts = 1,  // of rows on the sort path
    kCntClassRows    = 2,  // [kSpgemmClasses] non-empty rows per class (kSpgemmNone stays 0)
    kCntLdsEntries   = 7,  // entries of C the LDS classes counted
    kCntCount        = 8
};
static_assert(kCntClassRows + kSpgemmClasses == kCntLdsEntries, "one counter per class");

// ub, the class and the counters: one lane per row
__global__ __launch_bounds__(kBlock) void spgemm_products_kernel(int64_t m, const int32_t* __restrict__ a_rp, const int32_t* __restrict__ a_col,
                                                                 const int32_t* __restrict__ b_rp, int force_sort, int64_t* __restrict__ ub,
                                                                 int32_t* __restrict__ cls, unsigned long long* __restrict__ counters)
{
    __shared__ unsigned long long s_cnt[kCntCount];
    if (threadIdx.x < kCntCount) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += (int64_t)gridDim.x * kBlock)
    {
        int64_t   u   = 0;
        const int end = a_rp[i + 1];
        for (int e = a_rp[i]; e < end; ++e)
        {
            const int p = a_col[e];
            u += b_rp[p + 1] - b_rp[p];
        }
        int c = spgemm_class_of(u);
        if (force_sort && c != kSpgemmNone) c = kSpgemmSort;
        ub[i]  = u;
        cls[i] = c;
        if (u > 0)  // (integer sums: the order does not matter)
        {
            atomicAdd(&s_cnt[kCntProducts], (unsigned long long)u);
            if (c == kSpgemmSort) atomicAdd(&s_cnt[kCntSortProducts], (unsigned long long)u);
            atomicAdd(&s_cnt[kCntClassRows + c], 1ull);
        }
    }
    __syncthreads();
    if (threadIdx.x < kCntCount && s_cnt[threadIdx.x]) atomicAdd(counters + threadIdx.x, s_cnt[threadIdx.x]);
}

// The LDS classes: LANES lanes own a row of at most CAP products.  FILL = false counts the entries of every listed row of C
// (row_count, and their sum into the counters); FILL = true writes them at c_rp.  Every barrier is reached by the whole workgroup:
// the loop over row groups, the network size and the exchange loops are uniform across it.
template <int LANES, int CAP, bool FILL>
__global__ __launch_bounds__(kBlock) void spgemm_rows_kernel(int64_t nlist, const int32_t* __restrict__ rows, const int32_t* __restrict__ a_rp,
                                                             const int32_t* __restrict__ a_col, const double* __restrict__ a_val,
                                                             const int32_t* __restrict__ b_rp, const int32_t* __restrict__ b_col,
                                                             const double* __restrict__ b_val, const int64_t* __restrict__ ub,
                                                             int32_t* __restrict__ row_count, const int32_t* __restrict__ c_rp,
                                                             int32_t* __restrict__ c_col, double* __restrict__ c_val,
                                                             unsigned long long* __restrict__ counters)
{
    constexpr int RPB = kBlock / LANES;
    static_assert((CAP & (CAP - 1)) == 0 && RPB * CAP * kSpgemmLdsBytesPerProduct <= kSpgemmLdsAllocation, "a power of two that fits the allocation");
    __shared__ uint64_t           s_key[RPB * CAP];
    __shared__ double             s_val[FILL ? RPB * CAP : 1];
    __shared__ int                s_heads[kBlock];
    __shared__ int                s_net;
    __shared__ unsigned long long s_entries;
    const int       r = threadIdx.x / LANES, l = threadIdx.x % LANES;
    uint64_t* const key = s_key + r * CAP;
    double* const   val = s_val + (FILL ? r * CAP : 0);
    if (threadIdx.x == 0) s_entries = 0;
    unsigned long long mine   = 0;
    const int64_t      groups = (nlist + RPB - 1) / RPB;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x)
    {
        const int64_t k = g * RPB + r;
        const int32_t i = k < nlist ? rows[k] : -1;
        const int     u = i >= 0 ? (int)ub[i] : 0;  // (<= CAP: the class says so)
        if (threadIdx.x == 0) s_net = 2;
        __syncthreads();  // (and the row group before this one is done with its slices)
        if (i >= 0)
        {
            int       off = 0;
            const int end = a_rp[i + 1];
            for (int e = a_rp[i]; e < end; ++e)
            {
                const int    p = a_col[e], bb = b_rp[p], len = b_rp[p + 1] - bb;
                const double a = FILL ? a_val[e] : 0.0;
                for (int q = l; q < len; q += LANES)
                {
                    const int o = off + q;
                    key[o]      = ((uint64_t)(uint32_t)b_col[bb + q] << 32) | (uint32_t)o;
                    if constexpr (FILL) val[o] = __dmul_rn(a, b_val[bb + q]);
                }
                off += len;
            }
        }
        if (l == 0) atomicMax(&s_net, spgemm_network(u));
        __syncthreads();
        const int P = s_net;  // (<= CAP)
        for (int o = u + l; o < P; o += LANES) key[o] = ~(uint64_t)0;
        __syncthreads();
        for (int kk = 2; kk <= P; kk <<= 1)
            for (int j = kk >> 1; j > 0; j >>= 1)
            {
                for (int t = l; t < (P >> 1); t += LANES)
                {
                    const int      lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                    const uint64_t x = key[lo], y = key[hi];
                    if ((x > y) == ((lo & kk) == 0))
                    {
                        key[lo] = y;
                        key[hi] = x;
                    }
                }
                __syncthreads();
            }
        // heads of runs in this lane's stretch [from, to) of the sorted keys
        const int per = (u + LANES - 1) / LANES, from = min(u, l * per), to = min(u, from + per);
        int       heads = 0;
        for (int s = from; s < to; ++s) heads += (s == 0 || (uint32_t)(key[s] >> 32) != (uint32_t)(key[s - 1] >> 32)) ? 1 : 0;
        s_heads[threadIdx.x] = heads;
        __syncthreads();
        int before = 0;
        for (int t = 0; t < l; ++t) before += s_heads[r * LANES + t];
        if constexpr (!FILL)
        {
            if (l == LANES - 1 && i >= 0)
            {
                row_count[i] = before + heads;
                mine += (unsigned long long)(before + heads);
            }
        }
        else if (heads)
        {
            int64_t at = (int64_t)c_rp[i] + before;
            for (int s = from; s < to; ++s)
            {
                const uint32_t c = (uint32_t)(key[s] >> 32);
                if (s > 0 && c == (uint32_t)(key[s - 1] >> 32)) continue;
                double acc = 0.0;
                for (int t = s; t < u && (uint32_t)(key[t] >> 32) == c; ++t) acc = __dadd_rn(acc, val[(uint32_t)key[t]]);
                c_col[at] = (int32_t)c;
                c_val[at] = acc;
                ++at;
            }
        }
    }
    if constexpr (!FILL)
    {
        __syncthreads();
        if (mine) atomicAdd(&s_entries, mine);  // (integer sums)
        __syncthreads();
        if (threadIdx.x == 0 && s_entries) atomicAdd(counters + kCntLdsEntries, s_entries);
    }
}

// ---- the sort path ----------------------------------------------------------------------------------------------------------------
// out[k] = ub of the k-th listed row, out[nlist] = 0: the scan of nlist + 1 entries ends on the number of products
__global__ __launch_bounds__(kBlock) void spgemm_list_products_kernel(int64_t nlist, const int32_t* __restrict__ rows, const int64_t* __restrict__ ub,
                                                                      int32_t* __restrict__ out)
{
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k <= nlist; k += (int64_t)gridDim.x * kBlock)
        out[k] = k < nlist ? (int32_t)ub[rows[k]] : 0;
}

// the keys (place in the list, column) and the value of every product, in (row, p, q) order: 16 lanes a listed row
constexpr int kExpandLanes = 16;
__global__ __launch_bounds__(kBlock) void spgemm_expand_kernel(int64_t nlist, const int32_t* __restrict__ rows, const int32_t* __restrict__ a_rp,
                                                               const int32_t* __restrict__ a_col, const double* __restrict__ a_val,
                                                               const int32_t* __restrict__ b_rp, const int32_t* __restrict__ b_col,
                                                               const double* __restrict__ b_val, const int32_t* __restrict__ first,
                                                               int32_t* __restrict__ key_i, int32_t* __restrict__ key_j, double* __restrict__ t)
{
    const int l = threadIdx.x % kExpandLanes;
    for (int64_t k = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kExpandLanes; k < nlist; k += (int64_t)gridDim.x * (kBlock / kExpandLanes))
    {
        const int32_t i   = rows[k];
        int64_t       off = first[k];
        const int     end = a_rp[i + 1];
        for (int e = a_rp[i]; e < end; ++e)
        {
            const int    p = a_col[e], bb = b_rp[p], len = b_rp[p + 1] - bb;
            const double a = a_val[e];
            for (int q = l; q < len; q += kExpandLanes)
            {
                key_i[off + q] = (int32_t)k;
                key_j[off + q] = b_col[bb + q];
                t[off + q]     = __dmul_rn(a, b_val[bb + q]);
            }
            off += len;
        }
    }
}

// row_count[rows[k]] = list_count[k]
__global__ __launch_bounds__(kBlock) void spgemm_scatter_counts_kernel(int64_t nlist, const int32_t* __restrict__ rows,
                                                                       const int32_t* __restrict__ list_count, int32_t* __restrict__ row_count)
{
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < nlist; k += (int64_t)gridDim.x * kBlock) row_count[rows[k]] = list_count[k];
}

// ---- the transpose ----------------------------------------------------------------------------------------------------------------
// row[e] = the row of entry e: one lane per row
__global__ __launch_bounds__(kBlock) void spgemm_entry_rows_kernel(int64_t m, const int32_t* __restrict__ row_ptr, int32_t* __restrict__ row)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += (int64_t)gridDim.x * kBlock)
    {
        const int end = row_ptr[i + 1];
        for (int e = row_ptr[i]; e < end; ++e) row[e] = (int32_t)i;
    }
}

// what the sort path leaves for the second pass
struct sorted_part
{
    key_runs kr;  // i: the place in the list of rows, j: the column
    int32_t *rows = nullptr, *run_first = nullptr;
    double*  t = nullptr;
};

template <int CLS, bool FILL>
void launch_rows(hipStream_t s, int64_t nlist, const int32_t* rows, const spmv_mat* A, const spmv_mat* B, const int64_t* ub, int32_t* row_count,
                 const spmv_mat* C, unsigned long long* counters)
{
    constexpr spgemm_class_info info = spgemm_info(CLS);
    const int64_t               groups = ceil_div(nlist, kBlock / info.lanes);
    hipLaunchKernelGGL((spgemm_rows_kernel<info.lanes, info.capacity, FILL>), dim3((unsigned)std::min<int64_t>(kMaxGrid, groups)), dim3(kBlock), 0, s, nlist,
                       rows, A->a, A->b, A->v, B->a, B->b, B->v, ub, row_count, C ? C->a : nullptr, C ? const_cast<int32_t*>(C->b) : nullptr,
                       C ? const_cast<double*>(C->v) : nullptr, counters);
}

// the first pass of the sort path over the listed rows: their runs, and the entries of every listed row into row_count
int sort_path_count(spmv_ctx* ctx, device_pool& pool, const spmv_mat* A, const spmv_mat* B, const int64_t* ub, int64_t nlist, int32_t* rows,
                    int64_t total, int32_t* row_count, sorted_part* out)
{
    const char* const who = "spmv_spgemm";
    hipStream_t       s   = ctx->stream;
    const int         grid_l = stream_grid(nlist + 1);
    int32_t *         len, *first, *key_i, *key_j;
    SPMV_TRY(pool.get(len, (size_t)nlist + 1));
    SPMV_TRY(pool.get(first, (size_t)nlist + 1));
    hipLaunchKernelGGL(spgemm_list_products_kernel, dim3(grid_l), dim3(kBlock), 0, s, nlist, (const int32_t*)rows, ub, len);
    SPMV_TRY(exclusive_scan_i32(ctx, len, first, nlist + 1));
    SPMV_TRY(pool.get(key_i, (size_t)total));
    SPMV_TRY(pool.get(key_j, (size_t)total));
    SPMV_TRY(pool.get(out->t, (size_t)total));
    hipLaunchKernelGGL(spgemm_expand_kernel, dim3(stream_grid(nlist * kExpandLanes)), dim3(kBlock), 0, s, nlist, (const int32_t*)rows, A->a, A->b, A->v,
                       B->a, B->b, B->v, (const int32_t*)first, key_i, key_j, out->t);
    SPMV_TRY(hip_step(hipGetLastError(), who, "the expansion's launch"));
    SPMV_TRY(runs_by_key_pair(ctx, pool, who, key_i, nlist, key_j, B->ncol, total, &out->kr));
    SPMV_TRY(pool.get(out->run_first, (size_t)nlist + 1));
    SPMV_TRY(exclusive_scan_i32(ctx, out->kr.count_i, out->run_first, nlist + 1));
    hipLaunchKernelGGL(spgemm_scatter_counts_kernel, dim3(grid_l), dim3(kBlock), 0, s, nlist, (const int32_t*)rows, (const int32_t*)out->kr.count_i, row_count);
    SPMV_TRY(hip_step(hipGetLastError(), who, "the counts' launch"));
    out->rows = rows;
    return SPMV_OK;
}

int check_csr_operand(const spmv_mat* m, const char* who, const char* name)
{
    SPMV_REQUIRE(m->row_begin == 0, "%s: %s must be the whole matrix, not a shard (first row %lld)", who, name, (long long)m->row_begin);
    SPMV_REQUIRE(m->a && (m->nnz == 0 || (m->b && m->v)), "%s: the CSR arrays of %s are gone (panel_keep_csr = 0 released them)", who, name);
    return SPMV_OK;
}
}  // namespace

// ---- checks on the host: the leading fields of the handles alone -------------------------------------------------------------------
int spgemm_check(const spmv_ctx* ctx, const spmv_mat* A, const spmv_mat* B, int32_t method, const char* who)
{
    if (A->format != SPMV_FMT_CSR || B->format != SPMV_FMT_CSR)
        SPMV_FAIL(SPMV_ERR_UNSUPPORTED, "%s: both matrices must be CSR handles (A has format %d, B format %d)", who, A->format, B->format);
    SPMV_TRY(check_csr_operand(A, who, "A"));
    SPMV_TRY(check_csr_operand(B, who, "B"));
    SPMV_REQUIRE(A->ctx == ctx && B->ctx == ctx, "%s: %s belongs to another context", who, A->ctx != ctx ? "A" : "B");
    SPMV_REQUIRE(A->ncol == B->nrow, "%s: A is %d x %d and B is %d x %d: the columns of A must be the rows of B", who, A->nrow, A->ncol, B->nrow, B->ncol);
    SPMV_REQUIRE(method >= SPMV_SPGEMM_AUTO && method <= SPMV_SPGEMM_SORT, "%s: method=%d, must be 0 (AUTO), 1 (ROWS) or 2 (SORT)", who, method);
    return SPMV_OK;
}

int csr_transpose_check(const spmv_ctx* ctx, const spmv_mat* A, const char* who)
{
    if (A->format != SPMV_FMT_CSR) SPMV_FAIL(SPMV_ERR_UNSUPPORTED, "%s: A must be a CSR handle (format %d)", who, A->format);
    SPMV_TRY(check_csr_operand(A, who, "A"));
    SPMV_REQUIRE(A->ctx == ctx, "%s: A belongs to another context", who);
    return SPMV_OK;
}

bool spgemm_get_param(const spmv_mat* m, const char* name, int64_t* value)
{
    if (!strcmp(name, "spgemm_products"))
        *value = m->spgemm_products;
    else if (!strcmp(name, "spgemm_rows_lds"))
        *value = m->spgemm_rows_lds;
    else if (!strcmp(name, "spgemm_rows_sorted"))
        *value = m->spgemm_rows_sorted;
    else if (!strcmp(name, "spgemm_lds_products"))
        *value = m->spgemm_made ? kSpgemmLdsProducts : 0;
    else if (!strcmp(name, "spgemm_transient_bytes"))
        *value = m->spgemm_transient_bytes;
    else
        return false;
    return true;
}

// ---- C = A B; synchronous ----------------------------------------------------------------------------------------------------------
int spgemm(spmv_ctx* ctx, const spmv_mat* A, const spmv_mat* B, int32_t method, spmv_mat** out, int32_t force_kernel)
{
    const char* const who = "spmv_spgemm";
    SPMV_TRY(spgemm_check(ctx, A, B, method, who));
    const int64_t       m = A->nrow;
    hipStream_t         s = ctx->stream;
    device_pool         pool(ctx, who);
    int64_t*            ub;
    int32_t *           cls, *ids, *row_count;
    unsigned long long* counters;
    SPMV_TRY(pool.get(ub, (size_t)m));
    SPMV_TRY(pool.get(cls, (size_t)m));
    SPMV_TRY(pool.get(ids, (size_t)m));
    SPMV_TRY(pool.get(row_count, (size_t)m + 1));
    SPMV_TRY(pool.get(counters, (size_t)kCntCount));
    SPMV_TRY(hip_step(hipMemsetAsync(counters, 0, sizeof(unsigned long long) * kCntCount, s), who, "clearing the counters"));
    SPMV_TRY(hip_step(hipMemsetAsync(row_count, 0, sizeof(int32_t) * ((size_t)m + 1), s), who, "clearing the row counts"));
    // AUTO is ROWS: see DESIGN.md 19
    hipLaunchKernelGGL(spgemm_products_kernel, dim3(stream_grid(m)), dim3(kBlock), 0, s, m, A->a, A->b, B->a, method == SPMV_SPGEMM_SORT ? 1 : 0, ub, cls,
                       counters);
    SPMV_TRY(hip_step(hipGetLastError(), who, "the product count's launch"));
    unsigned long long h[kCntCount];
    SPMV_TRY(read_scalars(ctx, h, counters, sizeof(h), who));
    const unsigned long long products = h[kCntProducts], sort_products = h[kCntSortProducts];
    int64_t                  nrows[kSpgemmClasses], first[kSpgemmClasses + 1];
    int64_t                  nonempty = 0;
    for (int c = 1; c < kSpgemmClasses; ++c) nonempty += (nrows[c] = (int64_t)h[kCntClassRows + c]);
    nrows[kSpgemmNone] = m - nonempty;
    first[0]           = 0;
    for (int c = 0; c < kSpgemmClasses; ++c) first[c + 1] = first[c] + nrows[c];
    if (sort_products > (unsigned long long)INT32_MAX)
        SPMV_FAIL(SPMV_ERR_UNSUPPORTED, "%s: %llu scalar products on the sort path, its ids are int32 (at most %d)", who, sort_products, INT32_MAX);
    sorted_part sp;
    if (nonempty > 0)
    {
        SPMV_TRY(sort_ids_by_key(ctx, cls, m, key_bits(kSpgemmClasses), ids));  // the rows by class, ascending inside a class
        if (nrows[kSpgemmLane16]) launch_rows<kSpgemmLane16, false>(s, nrows[kSpgemmLane16], ids + first[kSpgemmLane16], A, B, ub, row_count, nullptr, counters);
        if (nrows[kSpgemmWave]) launch_rows<kSpgemmWave, false>(s, nrows[kSpgemmWave], ids + first[kSpgemmWave], A, B, ub, row_count, nullptr, counters);
        if (nrows[kSpgemmBlock]) launch_rows<kSpgemmBlock, false>(s, nrows[kSpgemmBlock], ids + first[kSpgemmBlock], A, B, ub, row_count, nullptr, counters);
        SPMV_TRY(hip_step(hipGetLastError(), who, "a launch of the counting pass"));
        if (nrows[kSpgemmSort])
            SPMV_TRY(sort_path_count(ctx, pool, A, B, ub, nrows[kSpgemmSort], ids + first[kSpgemmSort], (int64_t)sort_products, row_count, &sp));
        SPMV_TRY(read_scalars(ctx, h, counters, sizeof(h), who));
    }
    const unsigned long long entries = h[kCntLdsEntries] + (unsigned long long)sp.kr.runs;
    if (entries > (unsigned long long)INT32_MAX)
        SPMV_FAIL(SPMV_ERR_UNSUPPORTED, "%s: the product holds %llu entries, a CSR handle at most %d (int32 offsets)", who, entries, INT32_MAX);
    spmv_mat* C = nullptr;
    SPMV_TRY(mat_alloc(ctx, SPMV_FMT_CSR, A->nrow, B->ncol, (int64_t)entries, 0, (size_t)m + 1, (size_t)entries, (size_t)entries, &C));
    int rc = exclusive_scan_i32(ctx, row_count, const_cast<int32_t*>(C->a), m + 1);
    if (rc == SPMV_OK && nonempty > 0)
    {
        if (nrows[kSpgemmLane16]) launch_rows<kSpgemmLane16, true>(s, nrows[kSpgemmLane16], ids + first[kSpgemmLane16], A, B, ub, nullptr, C, counters);
        if (nrows[kSpgemmWave]) launch_rows<kSpgemmWave, true>(s, nrows[kSpgemmWave], ids + first[kSpgemmWave], A, B, ub, nullptr, C, counters);
        if (nrows[kSpgemmBlock]) launch_rows<kSpgemmBlock, true>(s, nrows[kSpgemmBlock], ids + first[kSpgemmBlock], A, B, ub, nullptr, C, counters);
        rc = hip_step(hipGetLastError(), who, "a launch of the filling pass");
        if (rc == SPMV_OK && sp.kr.runs)
            rc = runs_sum_into_csr(ctx, who, sp.kr, sp.t, sp.run_first, sp.rows, C->a, const_cast<int32_t*>(C->b), const_cast<double*>(C->v));
    }
    if (rc == SPMV_OK) rc = hip_step(hipStreamSynchronize(s), who, "waiting for the product");
    C->pb_trial = A->pb_trial;               // ("panel_trial" of the source handle holds for what is built from it)
    if (force_kernel != SPMV_CSR_AUTO)       // (a caller that builds the handle for itself: amg.hip)
    {
        C->kernel_forced = true;
        C->kernel        = force_kernel;
    }
    if (rc == SPMV_OK) rc = csr_analyse(C);  // the engine's usual selection
    if (rc != SPMV_OK)
    {
        mat_free(C);
        return rc;
    }
    C->spgemm_made            = true;
    C->spgemm_products        = (int64_t)products;
    C->spgemm_rows_lds        = nrows[kSpgemmLane16] + nrows[kSpgemmWave] + nrows[kSpgemmBlock];
    C->spgemm_rows_sorted     = nrows[kSpgemmSort];
    C->spgemm_transient_bytes = (int64_t)pool.bytes;
    *out                      = C;
    return SPMV_OK;
}

// ---- A^T as a CSR handle of its own; synchronous -------------------------------------------------------------------------------------
int csr_transpose(spmv_ctx* ctx, const spmv_mat* A, spmv_mat** out, int32_t force_kernel)
{
    const char* const who = "spmv_csr_transpose";
    SPMV_TRY(csr_transpose_check(ctx, A, who));
    device_pool pool(ctx, who);
    int32_t*    row;
    SPMV_TRY(pool.get(row, (size_t)A->nnz));
    hipLaunchKernelGGL(spgemm_entry_rows_kernel, dim3(stream_grid(A->nrow)), dim3(kBlock), 0, ctx->stream, (int64_t)A->nrow, A->a, row);
    SPMV_TRY(hip_step(hipGetLastError(), who, "the entry rows' launch"));
    spmv_mat coo;  // A's arrays read as COO with rows and columns swapped (borrowed: nothing of it outlives this call)
    coo.ctx    = ctx;
    coo.format = SPMV_FMT_COO;
    coo.nrow   = A->ncol;
    coo.ncol   = A->nrow;
    coo.nnz    = A->nnz;
    coo.a      = A->b;
    coo.b      = row;
    coo.v      = A->v;
    coo.pb_trial = A->pb_trial;  // ("panel_trial" of the source handle holds for what is built from it)
    return coo_to_csr(ctx, &coo, out, force_kernel);
}
}  // namespace spmv
