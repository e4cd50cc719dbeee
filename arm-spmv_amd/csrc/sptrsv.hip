// sptrsv.hip — triangular solves with a matrix the caller supplies: x = op(T)^-1 b for one right-hand side (spmv_trsv_solve) or k of
// them, row-major (spmv_trsv_solve_multi).  T is the strictly lower or strictly upper part of a square CSR handle, selected by row
// and column index, plus the diagonal (SPMV_TRSV_UNIT: the diagonal is 1 and stored diagonal entries are ignored); op is the identity
// or, under SPMV_TRSV_TRANSPOSE, the transpose.  Entries of the other triangle are ignored, so the combined LU array of
// spmv_ilu0_factors on A's own pattern is an input for both of its solves.
//
// Set-up (trsv_setup; synchronous, once per handle and (uplo, transpose) pair): a working copy of the selected triangle as a
// tri_part - duplicates of the diagonal entry summed (split_count_kernel's rule), every other stored entry a term of its own in
// stored order (split_fill_kernel's with pos = nullptr); under TRANSPOSE the transpose of that copy, a row's entries in ascending
// column index (a stable sort by column: duplicates keep their stored order) - then analyse_part of tri_levels.hpp: levels, rows by
// level, lanes per row, the launch schedule.  The level table stays on the host.  UNIT and non-UNIT solves share the analysis; the
// smallest row whose diagonal is missing, zero or not finite is remembered and refuses every non-UNIT use.
//
// One right-hand side: solve<UNIT> of tri_levels.hpp, its kernels and its lane tree.
//
// k right-hand sides (1 .. 64), the hot path of this unit.  A group of T lanes owns a row, T the next power of two >= min(k, 16);
// lane t owns column t and walks the row's entries once per tile of 16 columns inside the same launch, so that the launch count
// does not grow with k and X[col * k + t] is one contiguous read across the group.  No lane shares a sum: for every column
//     acc = 0.0;  for the row's entries left to right: acc = fma(T_ij, x_j, acc);  x_i = b_i - acc  (UNIT)  or  (b_i - acc) / d_i
// whatever k and the tile, so column c of a k-column solve has the bits of a k = 1 solve of that column, and those of the one
// right-hand-side solve wherever that runs 1 lane per row.  The schedule is tri_levels.hpp's rule over the same level table with T
// in place of the lanes - a level of more than kSmallLevel lanes is a launch of its own, runs of smaller levels share one
// workgroup that steps through them with barriers - made on the host per T and cached.  Ordering between levels comes from kernel
// boundaries or from the barrier inside that one workgroup (same CU, same L1), never from one workgroup waiting for another.
// B and X may be the same array: a row reads B at its own index only, before it writes X there.
#include <climits>
#include <cmath>
#include <cstring>

#include "tri_levels.hpp"

namespace spmv
{
constexpr int kTrsvSlots = 4;   // (uplo, transpose) pairs: bit 0 upper, bit 1 transposed
constexpr int kTrsvWidths = 5;  // T = 1, 2, 4, 8, 16

struct trsv_state
{
    struct slot
    {
        bool     present = false;
        tri_part part;              // the working copy, its levels and the one right-hand-side schedule
        double*  diag    = nullptr; // [n] the diagonal, duplicates summed (0.0 where none is stored)
        int32_t  bad_row = -1;      // the smallest row whose diagonal is missing, zero or not finite; -1: none
        int64_t  bytes   = 0;
        std::vector<int32_t>           lvl_host;                    // [levels + 1] the level table
        std::vector<tri_part::segment> multi[kTrsvWidths];          // the k-column schedule per T = 1 << index
        bool                           multi_made[kTrsvWidths] = {};
    };
    slot    s[kTrsvSlots];
    int64_t multi_launches = 0, multi_level_launches = 0;  // of the last spmv_trsv_solve_multi: all, and those of the own-launch kernel
};

namespace
{
inline int  slot_of(uint32_t flags) { return ((flags & SPMV_TRSV_UPPER) ? 1 : 0) | ((flags & SPMV_TRSV_TRANSPOSE) ? 2 : 0); }
const char* slot_name(int idx)
{
    static const char* const names[kTrsvSlots] = {"lower", "upper", "transposed lower", "transposed upper"};
    return names[idx];
}

// ---- the working copy ---------------------------------------------------------------------------------------------------------
// entries of the selected triangle per row, the diagonal with its duplicates summed, the smallest row without a usable one
__global__ __launch_bounds__(kBlock) void trsv_count_kernel(int n, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                            const double* __restrict__ val, int upper, int32_t* __restrict__ cnt,
                                                            double* __restrict__ diag, int* __restrict__ bad)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i > n) return;
    if (i == n)
    {
        cnt[n] = 0;
        return;
    }
    int    k = 0;
    double d = 0.0;
    bool   has = false;
    for (int j = row_ptr[i]; j < row_ptr[i + 1]; ++j)
    {
        const int c = col[j];
        if (c == i)
        {
            d += val[j];
            has = true;
        }
        else if (upper ? c > i : c < i)
            ++k;
    }
    cnt[i]  = k;
    diag[i] = d;
    if (!has || !(d != 0.0) || !isfinite(d)) atomicMin(bad, i);
}

// the selected entries in stored order; row (transposed copies only): the row of every entry
__global__ __launch_bounds__(kBlock) void trsv_fill_kernel(int n, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                           const double* __restrict__ val, int upper, const int32_t* __restrict__ ptr,
                                                           int32_t* __restrict__ out_col, double* __restrict__ out_val,
                                                           int32_t* __restrict__ out_row)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    int p = ptr[i];
    for (int j = row_ptr[i]; j < row_ptr[i + 1]; ++j)  // the order inside the row is kept
    {
        const int c = col[j];
        if (c == i || (upper ? c < i : c > i)) continue;
        out_col[p] = c;
        out_val[p] = val[j];
        if (out_row) out_row[p] = i;
        ++p;
    }
}

// transposed copies: entries per column (cnt: n + 1 zeros)
__global__ __launch_bounds__(kBlock) void trsv_col_count_kernel(int64_t nnz, const int32_t* __restrict__ col, int32_t* __restrict__ cnt)
{
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < nnz; j += (int64_t)gridDim.x * kBlock) atomicAdd(cnt + col[j], 1);
}

// ---- k right-hand sides ---------------------------------------------------------------------------------------------------------
// row i by the group's lane t: columns t, t + T, ... (T < 16: T >= k, one trip; else tiles of 16 columns)
template <int T, bool UNIT>
__device__ __forceinline__ void trsv_multi_row(int i, int t, int k, const int32_t* __restrict__ ptr, const int32_t* __restrict__ col,
                                               const double* __restrict__ val, const double* __restrict__ diag, const double* B, double* X)
{
    const int b = ptr[i], e = ptr[i + 1];
    double    d = 1.0;
    if constexpr (!UNIT) d = diag[i];
    for (int c = t; c < k; c += T)
    {
        double acc = 0.0;
        for (int j = b; j < e; ++j) acc = fma(val[j], X[(int64_t)col[j] * k + c], acc);
        const int64_t at = (int64_t)i * k + c;
        const double  r  = B[at] - acc;
        if constexpr (UNIT)
            X[at] = r;
        else
            X[at] = r / d;
    }
}

// one level: rows order[first .. first + rows)
template <int T, bool UNIT>
__global__ __launch_bounds__(kBlock) void trsv_multi_level_kernel(int first, int rows, int k, const int32_t* __restrict__ order,
                                                                  const int32_t* __restrict__ ptr, const int32_t* __restrict__ col,
                                                                  const double* __restrict__ val, const double* __restrict__ diag,
                                                                  const double* B, double* X)
{
    const int64_t r = (int64_t)blockIdx.x * (kBlock / T) + threadIdx.x / T;
    if (r < rows) trsv_multi_row<T, UNIT>(order[first + r], threadIdx.x % T, k, ptr, col, val, diag, B, X);
}

// a run of small levels in one workgroup: what a level wrote is read by the next after the barrier (same CU, same L1)
template <int T, bool UNIT>
__global__ __launch_bounds__(kSolveThreads) void trsv_multi_run_kernel(int first_level, int nlevels, int k, const int32_t* __restrict__ lvl_ptr,
                                                                       const int32_t* __restrict__ order, const int32_t* __restrict__ ptr,
                                                                       const int32_t* __restrict__ col, const double* __restrict__ val,
                                                                       const double* __restrict__ diag, const double* B, double* X)
{
    const int r0 = threadIdx.x / T, t = threadIdx.x % T;
    for (int lv = first_level; lv < first_level + nlevels; ++lv)
    {
        const int first = lvl_ptr[lv], rows = lvl_ptr[lv + 1] - first;
        for (int r = r0; r < rows; r += kSolveThreads / T) trsv_multi_row<T, UNIT>(order[first + r], t, k, ptr, col, val, diag, B, X);
        __syncthreads();  // (outside the row loop: every lane reaches it)
    }
}

// tri_levels.hpp's schedule rule over the level table lp with T lanes per row
void make_schedule(const std::vector<int32_t>& lp, int T, std::vector<tri_part::segment>& out)
{
    out.clear();
    const int levels = (int)lp.size() - 1;
    for (int lv = 0; lv < levels;)
    {
        const int rows = lp[(size_t)lv + 1] - lp[(size_t)lv];
        if ((int64_t)rows * T > kSmallLevel)
        {
            out.push_back({lv, 1, lp[(size_t)lv], rows});
            ++lv;
            continue;
        }
        int end = lv;
        while (end < levels && (int64_t)(lp[(size_t)end + 1] - lp[(size_t)end]) * T <= kSmallLevel) ++end;
        out.push_back({lv, end - lv, lp[(size_t)lv], lp[(size_t)end] - lp[(size_t)lv]});
        lv = end;
    }
}

template <int T, bool UNIT>
void launch_multi(hipStream_t s, const trsv_state::slot& S, const std::vector<tri_part::segment>& sched, int k, const double* B, double* X,
                  int64_t* launches, int64_t* level_launches)
{
    const tri_part& p = S.part;
    for (const tri_part::segment& g : sched)
    {
        if (g.rows == 0) continue;
        ++*launches;
        if (g.nlevels > 1 || (int64_t)g.rows * T <= kSolveThreads)
            hipLaunchKernelGGL((trsv_multi_run_kernel<T, UNIT>), dim3(1), dim3(kSolveThreads), 0, s, g.first_level, g.nlevels, k, p.lvl_ptr, p.order,
                               p.ptr, p.col, p.val, S.diag, B, X);
        else
        {
            ++*level_launches;
            hipLaunchKernelGGL((trsv_multi_level_kernel<T, UNIT>), dim3((unsigned)ceil_div(g.rows, kBlock / T)), dim3(kBlock), 0, s, g.first_row,
                               g.rows, k, p.order, p.ptr, p.col, p.val, S.diag, B, X);
        }
    }
}

template <bool UNIT>
void launch_multi_width(int w, hipStream_t s, const trsv_state::slot& S, const std::vector<tri_part::segment>& sched, int k, const double* B,
                        double* X, int64_t* launches, int64_t* level_launches)
{
    switch (w)
    {
    case 0: launch_multi<1, UNIT>(s, S, sched, k, B, X, launches, level_launches); break;
    case 1: launch_multi<2, UNIT>(s, S, sched, k, B, X, launches, level_launches); break;
    case 2: launch_multi<4, UNIT>(s, S, sched, k, B, X, launches, level_launches); break;
    case 3: launch_multi<8, UNIT>(s, S, sched, k, B, X, launches, level_launches); break;
    default: launch_multi<16, UNIT>(s, S, sched, k, B, X, launches, level_launches); break;
    }
}

size_t launches_of(const std::vector<tri_part::segment>& sched)
{
    size_t k = 0;
    for (const tri_part::segment& g : sched) k += g.rows > 0;
    return k;
}

void free_slot(spmv_mat* m, trsv_state::slot& S)
{
    free_part(S.part);
    if (S.diag) (void)hipFree(S.diag);
    if (S.present) m->device_bytes -= S.bytes;
    S = trsv_state::slot();
}

// the working copy of slot idx and its analysis; on failure the slot holds nothing
int build_slot(spmv_mat* m, int idx, trsv_state::slot& S)
{
    const int   n = m->nrow;
    spmv_ctx*   ctx = m->ctx;
    hipStream_t s   = ctx->stream;
    const int   upper = idx & 1, transposed = idx & 2;
    SPMV_TRY(ensure_scratch(ctx, 64));
    int*      flag = (int*)ctx->scratch;
    tri_part& p    = S.part;
    int32_t * cnt = nullptr, *t_ptr = nullptr, *t_col = nullptr, *t_row = nullptr;
    double*   t_val = nullptr;
    int       rc = SPMV_OK;
    const unsigned grid1 = (unsigned)ceil_div((int64_t)n + 1, kBlock);
    do
    {
        if (hipMalloc(&cnt, sizeof(int32_t) * ((size_t)n + 1)) != hipSuccess || hipMalloc(&p.ptr, sizeof(int32_t) * ((size_t)n + 1)) != hipSuccess ||
            hipMalloc(&S.diag, sizeof(double) * (size_t)n) != hipSuccess)
        {
            rc = SPMV_ERR_ALLOC;
            break;
        }
        const int h_none = INT_MAX;
        if (hipMemcpyAsync(flag, &h_none, sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        {
            rc = SPMV_ERR_HIP;
            break;
        }
        hipLaunchKernelGGL(trsv_count_kernel, dim3(grid1), dim3(kBlock), 0, s, n, m->a, m->b, m->v, upper, cnt, S.diag, flag);
        int h_bad = INT_MAX;  // (read before the scan: it uses the context's scratch too)
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&h_bad, flag, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
        {
            rc = SPMV_ERR_HIP;
            break;
        }
        S.bad_row = h_bad == INT_MAX ? -1 : h_bad;
        if ((rc = exclusive_scan_i32(ctx, cnt, p.ptr, (int64_t)n + 1)) != SPMV_OK) break;
        int32_t h_nnz = 0;
        if (hipMemcpyAsync(&h_nnz, p.ptr + n, sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        {
            rc = SPMV_ERR_HIP;
            break;
        }
        if (h_nnz < 0 || (int64_t)h_nnz > m->nnz)
        {
            set_error("spmv_trsv_setup: selecting the %s triangle gave %d entries of %lld", slot_name(idx & 1), h_nnz, (long long)m->nnz);
            rc = SPMV_ERR_HIP;
            break;
        }
        p.nnz = h_nnz;
        const size_t nz = std::max<size_t>(1, (size_t)h_nnz);
        if (hipMalloc(&p.col, sizeof(int32_t) * nz) != hipSuccess || hipMalloc(&p.val, sizeof(double) * nz) != hipSuccess)
        {
            rc = SPMV_ERR_ALLOC;
            break;
        }
        if (!transposed)
            hipLaunchKernelGGL(trsv_fill_kernel, dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0, s, n, m->a, m->b, m->v, upper, p.ptr, p.col, p.val,
                               (int32_t*)nullptr);
        else
        {
            // the selected entries in stored order with their rows, then by column (stable): the transpose, a row's entries in
            // ascending column index
            if (hipMalloc(&t_col, sizeof(int32_t) * nz) != hipSuccess || hipMalloc(&t_row, sizeof(int32_t) * nz) != hipSuccess ||
                hipMalloc(&t_val, sizeof(double) * nz) != hipSuccess || hipMalloc(&t_ptr, sizeof(int32_t) * ((size_t)n + 1)) != hipSuccess)
            {
                rc = SPMV_ERR_ALLOC;
                break;
            }
            hipLaunchKernelGGL(trsv_fill_kernel, dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0, s, n, m->a, m->b, m->v, upper, p.ptr, t_col, t_val,
                               t_row);
            (void)hipMemsetAsync(cnt, 0, sizeof(int32_t) * ((size_t)n + 1), s);
            if (h_nnz > 0) hipLaunchKernelGGL(trsv_col_count_kernel, dim3(stream_grid(h_nnz)), dim3(kBlock), 0, s, (int64_t)h_nnz, t_col, cnt);
            if (hipGetLastError() != hipSuccess)
            {
                rc = SPMV_ERR_HIP;
                break;
            }
            if ((rc = exclusive_scan_i32(ctx, cnt, t_ptr, (int64_t)n + 1)) != SPMV_OK) break;
            if ((rc = coo_place_by_stable_sort(ctx, h_nnz, n, t_col, t_row, t_val, p.col, p.val)) != SPMV_OK) break;
            std::swap(p.ptr, t_ptr);
        }
        if (hipGetLastError() != hipSuccess)
        {
            rc = SPMV_ERR_HIP;
            break;
        }
        if ((rc = analyse_part(ctx, n, p, slot_name(idx), "spmv_trsv_setup")) != SPMV_OK) break;
        S.lvl_host.assign((size_t)p.levels + 1, 0);
        if (hipMemcpyAsync(S.lvl_host.data(), p.lvl_ptr, sizeof(int32_t) * S.lvl_host.size(), hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            rc = SPMV_ERR_HIP;
    } while (0);
    (void)hipStreamSynchronize(s);
    for (void* q : {(void*)cnt, (void*)t_ptr, (void*)t_col, (void*)t_row, (void*)t_val})
        if (q) (void)hipFree(q);
    if (rc != SPMV_OK)
    {
        free_slot(m, S);
        if (rc == SPMV_ERR_ALLOC) set_error("spmv_trsv_setup: out of device memory copying a triangle of a matrix of %lld entries", (long long)m->nnz);
        if (rc == SPMV_ERR_HIP && hipGetLastError() != hipSuccess) set_error("spmv_trsv_setup: set-up failed: %s", hipGetErrorString(hipGetLastError()));
        return rc;
    }
    // ptr, col + val, order, the level table, the diagonal
    S.bytes   = ((int64_t)n + 1) * 4 + p.nnz * 12 + (int64_t)n * 4 + ((int64_t)p.levels + 1) * 4 + (int64_t)n * 8;
    S.present = true;
    m->device_bytes += S.bytes;
    return SPMV_OK;
}

int refuse_diagonal(const trsv_state::slot& S, const char* who)
{
    SPMV_FAIL(SPMV_ERR_INVALID, "%s: the diagonal entry of row %d is missing, zero or not finite (SPMV_TRSV_UNIT solves without it)", who, S.bad_row);
}

void drop_if_empty(spmv_mat* m)
{
    for (const trsv_state::slot& S : m->trsv->s)
        if (S.present) return;
    delete m->trsv;
    m->trsv = nullptr;
}
}  // namespace

int trsv_check_flags(uint32_t flags, const char* who)
{
    constexpr uint32_t known = SPMV_TRSV_UPPER | SPMV_TRSV_UNIT | SPMV_TRSV_TRANSPOSE;
    SPMV_REQUIRE((flags & ~known) == 0, "%s: unknown flag bits 0x%x (SPMV_TRSV_LOWER / UPPER, UNIT, TRANSPOSE)", who, flags & ~known);
    return SPMV_OK;
}

int trsv_check_handle(const spmv_mat* m, const char* who) { return check_whole_square_csr(m, who, "a triangular solve"); }

void trsv_free(spmv_mat* m)
{
    if (!m->trsv) return;
    for (trsv_state::slot& S : m->trsv->s) free_slot(m, S);
    delete m->trsv;
    m->trsv = nullptr;
}

int trsv_setup(spmv_mat* m, uint32_t flags)
{
    SPMV_TRY(trsv_check_flags(flags, "spmv_trsv_setup"));
    SPMV_TRY(trsv_check_handle(m, "spmv_trsv_setup"));
    if (m->nrow == 0) return SPMV_OK;
    const int  idx  = slot_of(flags);
    const bool unit = (flags & SPMV_TRSV_UNIT) != 0;
    if (m->trsv && m->trsv->s[idx].present)
    {
        if (!unit && m->trsv->s[idx].bad_row >= 0) return refuse_diagonal(m->trsv->s[idx], "spmv_trsv_setup");
        return SPMV_OK;
    }
    if (!m->trsv) m->trsv = new trsv_state();
    trsv_state::slot& S  = m->trsv->s[idx];
    int               rc = build_slot(m, idx, S);
    if (rc == SPMV_OK && !unit && S.bad_row >= 0)
    {
        rc = refuse_diagonal(S, "spmv_trsv_setup");
        free_slot(m, S);  // a failed set-up leaves nothing behind
    }
    if (rc != SPMV_OK) drop_if_empty(m);
    return rc;
}

// x = op(T)^-1 b; the analysis of `flags` must be there
int trsv_apply(spmv_ctx* ctx, const spmv_mat* A, uint32_t flags, const double* b, double* x)
{
    if (A->nrow == 0) return SPMV_OK;
    if (!A->trsv || !A->trsv->s[slot_of(flags)].present) SPMV_FAIL(SPMV_ERR_INVALID, "spmv_trsv_solve: the handle was not set up");
    const trsv_state::slot& S = A->trsv->s[slot_of(flags)];
    if (flags & SPMV_TRSV_UNIT)
        solve<true>(ctx->stream, S.part, nullptr, b, x);
    else
        solve<false>(ctx->stream, S.part, S.diag, b, x);
    SPMV_HIP(hipGetLastError());
    return SPMV_OK;
}

int trsv_apply_multi(spmv_ctx* ctx, const spmv_mat* A, uint32_t flags, int32_t k, const double* B, double* X)
{
    if (A->nrow == 0) return SPMV_OK;
    if (!A->trsv || !A->trsv->s[slot_of(flags)].present) SPMV_FAIL(SPMV_ERR_INVALID, "spmv_trsv_solve_multi: the handle was not set up");
    trsv_state*       st = A->trsv;
    trsv_state::slot& S  = st->s[slot_of(flags)];
    int               w  = 0;
    while ((1 << w) < std::min(k, 16)) ++w;
    if (!S.multi_made[w])
    {
        make_schedule(S.lvl_host, 1 << w, S.multi[w]);
        S.multi_made[w] = true;
    }
    st->multi_launches = st->multi_level_launches = 0;
    if (flags & SPMV_TRSV_UNIT)
        launch_multi_width<true>(w, ctx->stream, S, S.multi[w], k, B, X, &st->multi_launches, &st->multi_level_launches);
    else
        launch_multi_width<false>(w, ctx->stream, S, S.multi[w], k, B, X, &st->multi_launches, &st->multi_level_launches);
    SPMV_HIP(hipGetLastError());
    return SPMV_OK;
}

int trsv_info(const spmv_mat* m, uint32_t flags, int32_t* levels, int32_t* lanes, int32_t* launches, int64_t* bytes)
{
    SPMV_TRY(trsv_check_flags(flags, "spmv_trsv_info"));
    if (!m->trsv || !m->trsv->s[slot_of(flags)].present)
        SPMV_FAIL(SPMV_ERR_INVALID, "spmv_trsv_info: the %s triangle of this handle was not set up (spmv_trsv_setup)", slot_name(slot_of(flags)));
    const trsv_state::slot& S = m->trsv->s[slot_of(flags)];
    if (levels) *levels = S.part.levels;
    if (lanes) *lanes = S.part.lanes;
    if (launches) *launches = (int32_t)launches_of(S.part.schedule);
    if (bytes) *bytes = S.bytes;
    return SPMV_OK;
}

bool trsv_get_param(const spmv_mat* m, const char* what, int64_t* value)
{
    const trsv_state* st = m->trsv;
    if (!strcmp(what, "trsv_ready"))  // bit (upper ? 1 : 0) | (transposed ? 2 : 0) of every analysis present
    {
        *value = 0;
        for (int i = 0; st && i < kTrsvSlots; ++i) *value |= st->s[i].present ? (int64_t)1 << i : 0;
    }
    else if (!strcmp(what, "trsv_bytes"))
    {
        *value = 0;
        for (int i = 0; st && i < kTrsvSlots; ++i) *value += st->s[i].present ? st->s[i].bytes : 0;
    }
    else if (!strcmp(what, "trsv_multi_launches"))  // of the last spmv_trsv_solve_multi
        *value = st ? st->multi_launches : 0;
    else if (!strcmp(what, "trsv_multi_level_launches"))  // of them: levels with a launch of their own
        *value = st ? st->multi_level_launches : 0;
    else
        return false;
    return true;
}
}  // namespace spmv
