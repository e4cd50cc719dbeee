// tri_levels.hpp — what the symmetric Gauss-Seidel sweep (symgs.hip) and the ILU(0) preconditioner (ilu0.hip) share: the
// multicolour order of the rows, the split of A into L + D + U by sweep position, the dependency levels of a triangle, the
// launch schedule over them and the level-solve kernels.  Both translation units include it; everything but tri_part sits in
// an unnamed namespace, so each unit has its own instances of the kernels.
//
// A triangular solve in a given order is only as parallel as the order lets it be.  Rows are put in LEVELS: level(i) = 1 + max
// level(j) over the entries j of row i in the triangle; the rows of one level depend on earlier levels only and are solved
// together.  Levels are found on the device by relaxing level(i) = max(level(j) + 1) to its fixed point, rows are ordered by
// level with a stable radix sort (ascending row index inside a level: neighbouring lanes read neighbouring rows), and the
// schedule — one launch per level, runs of small levels folded into one launch of a single workgroup that steps through them
// with barriers — is fixed at set-up.
#pragma once

#include <algorithm>
#include <vector>

#include "common.hpp"
#include "wave.hpp"

namespace spmv
{
struct tri_part
{
    int32_t* ptr     = nullptr;  // [n + 1]
    int32_t* col     = nullptr;  // [nnz]
    double*  val     = nullptr;  // [nnz]
    int32_t* order   = nullptr;  // [n] rows by level, ascending inside a level
    int32_t* lvl_ptr = nullptr;  // [levels + 1] into order
    int64_t  nnz     = 0;
    int32_t  levels  = 0;
    int32_t  lanes   = 1;  // lanes per row in the solve and product kernels
    struct segment
    {
        int32_t first_level, nlevels, first_row, rows;  // nlevels > 1: one workgroup steps through them
    };
    std::vector<segment> schedule;
};

namespace
{
constexpr int kSolveThreads = 1024;
constexpr int kSmallLevel   = 4096;  // lanes: levels up to this many (rows x lanes per row) are folded into one workgroup

// ---- split A = L + D + U ------------------------------------------------------------------------------------------
// pos: position of every row in the sweep (null: the row index itself); an entry belongs to L if its column comes
// earlier in the sweep than its row
__global__ __launch_bounds__(kBlock) void split_count_kernel(int n, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                             const double* __restrict__ val, const int32_t* __restrict__ pos,
                                                             int32_t* __restrict__ lo_cnt, int32_t* __restrict__ up_cnt,
                                                             double* __restrict__ diag, int* __restrict__ flag)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i > n) return;
    if (i == n)
    {
        lo_cnt[n] = 0;
        up_cnt[n] = 0;
        return;
    }
    int       nl = 0, nu = 0;
    double    d  = 0.0;
    const int pi = pos ? pos[i] : i;
    for (int j = row_ptr[i]; j < row_ptr[i + 1]; ++j)
    {
        const int c = col[j];
        if (c == i)
            d += val[j];  // duplicates of the diagonal entry are summed, as the product would
        else if ((pos ? pos[c] : c) < pi)
            ++nl;
        else
            ++nu;
    }
    lo_cnt[i] = nl;
    up_cnt[i] = nu;
    diag[i]   = d;
    if (d == 0.0) atomicOr(flag, 1);
}

__global__ __launch_bounds__(kBlock) void split_fill_kernel(int n, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                            const double* __restrict__ val, const int32_t* __restrict__ pos,
                                                            const int32_t* __restrict__ lo_ptr, const int32_t* __restrict__ up_ptr,
                                                            int32_t* __restrict__ lo_col, double* __restrict__ lo_val,
                                                            int32_t* __restrict__ up_col, double* __restrict__ up_val)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    int       pl = lo_ptr[i], pu = up_ptr[i];
    const int pi = pos ? pos[i] : i;
    for (int j = row_ptr[i]; j < row_ptr[i + 1]; ++j)  // the order inside the row is kept
    {
        const int c = col[j];
        if (c == i) continue;
        if ((pos ? pos[c] : c) < pi)
        {
            lo_col[pl] = c;
            lo_val[pl] = val[j];
            ++pl;
        }
        else
        {
            up_col[pu] = c;
            up_val[pu] = val[j];
            ++pu;
        }
    }
}

// ---- multicolour order ----------------------------------------------------------------------------------------------
// Greedy colouring in row order by relaxation: colour(i) = smallest colour none of the rows j < i coupled to i has.
// A row is final once the rows before it are (induction over the dependency levels), final rows never change again,
// and a pass that changes nothing is the fixed point — the same colours a sequential greedy pass would give.  Rows
// j > i coupled to i avoid colour(i) in their own turn when the pattern is symmetric; where it is not, two coupled
// rows may share a colour and the level analysis below simply keeps them apart.
__global__ __launch_bounds__(kBlock) void colour_relax_kernel(int n, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                              int32_t* colour, int* __restrict__ changed)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int b = row_ptr[i], e = row_ptr[i + 1];
    int       m = 0;
    for (int base = 0;; base += 64)  // (ends: a row has fewer coupled rows than colours tried)
    {
        unsigned long long used = 0ull;
        for (int j = b; j < e; ++j)
        {
            const int c = col[j];
            if (c >= i) continue;
            const int cj = __builtin_nontemporal_load(colour + c) - base;
            if (cj >= 0 && cj < 64) used |= 1ull << cj;
        }
        if (~used)
        {
            m = base + __builtin_ctzll(~used);
            break;
        }
    }
    if (m != colour[i])
    {
        colour[i] = m;
        *changed  = 1;
    }
}

__global__ __launch_bounds__(kBlock) void invert_order_kernel(int n, const int32_t* __restrict__ seq, int32_t* __restrict__ pos)
{
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k < n) pos[seq[k]] = k;
}

// ---- levels -----------------------------------------------------------------------------------------------------
// One relaxation pass, in place: values only grow and never pass the true level, so any interleaving of the lanes
// ends at the same fixed point; a pass that changes nothing has reached it.
__global__ __launch_bounds__(kBlock) void level_relax_kernel(int n, const int32_t* __restrict__ ptr, const int32_t* __restrict__ col,
                                                             int32_t* lev, int* __restrict__ changed)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    int m = 0;
    for (int j = ptr[i]; j < ptr[i + 1]; ++j) m = max(m, __builtin_nontemporal_load(lev + col[j]) + 1);
    if (m > lev[i])
    {
        lev[i]   = m;
        *changed = 1;
    }
}

__global__ __launch_bounds__(kBlock) void level_hist_kernel(int n, const int32_t* __restrict__ lev, int32_t* __restrict__ hist, int nlevels)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n && lev[i] < nlevels) atomicAdd(hist + lev[i], 1);
}

__global__ __launch_bounds__(kBlock) void level_max_kernel(int n, const int32_t* __restrict__ lev, int32_t* __restrict__ out)
{
    int m = 0;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) m = max(m, lev[i]);
    for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) atomicMax(out, m);
}

// ---- the level solve ------------------------------------------------------------------------------------------------
// x_i = (t_i - sum_j T_ij x_j) / d_i over the entries of row i in the triangle T; UNIT: the diagonal is 1 and is neither read
// nor divided by (the L of an LU factorisation).  LANES lanes share a row; their partial sums meet in a fixed tree (group_sum),
// so the result does not depend on the launch that solves the row.  t and x may be the same vector: a row reads t at its own
// index only, before it writes x there.
template <int LANES, bool UNIT = false>
__device__ __forceinline__ void solve_row(int i, int l, bool on, const int32_t* __restrict__ ptr, const int32_t* __restrict__ col,
                                          const double* __restrict__ val, const double* __restrict__ diag, const double* t, double* x)
{
    double acc = 0.0;
    if (on)
        for (int j = ptr[i] + l; j < ptr[i + 1]; j += LANES) acc = fma(val[j], x[col[j]], acc);
    acc = group_sum<LANES, true>(acc);
    if constexpr (UNIT)
    {
        if (on && l == 0) x[i] = t[i] - acc;
    }
    else
    {
        if (on && l == 0) x[i] = (t[i] - acc) / diag[i];
    }
}

// one level: rows order[first .. first + rows)
template <int LANES, bool UNIT = false>
__global__ __launch_bounds__(kBlock) void tri_solve_level_kernel(int first, int rows, const int32_t* __restrict__ order,
                                                                 const int32_t* __restrict__ ptr, const int32_t* __restrict__ col,
                                                                 const double* __restrict__ val, const double* __restrict__ diag,
                                                                 const double* t, double* x)
{
    const int  gid = blockIdx.x * kBlock + threadIdx.x;
    const int  r = gid / LANES, l = gid % LANES;
    const bool on = r < rows;
    solve_row<LANES, UNIT>(on ? order[first + r] : 0, l, on, ptr, col, val, diag, t, x);
}

// a run of small levels in one workgroup: what a level wrote is read by the next after the barrier (same CU, same L1)
template <int LANES, bool UNIT = false>
__global__ __launch_bounds__(kSolveThreads) void tri_solve_run_kernel(int first_level, int nlevels, const int32_t* __restrict__ lvl_ptr,
                                                                      const int32_t* __restrict__ order, const int32_t* __restrict__ ptr,
                                                                      const int32_t* __restrict__ col, const double* __restrict__ val,
                                                                      const double* __restrict__ diag, const double* t, double* x)
{
    const int r0 = threadIdx.x / LANES, l = threadIdx.x % LANES;
    for (int lv = first_level; lv < first_level + nlevels; ++lv)
    {
        const int first = lvl_ptr[lv], rows = lvl_ptr[lv + 1] - first;
        for (int base = 0; base < rows; base += kSolveThreads / LANES)  // (uniform bounds: every lane reaches the barrier)
        {
            const int  r  = base + r0;
            const bool on = r < rows;
            solve_row<LANES, UNIT>(on ? order[first + r] : 0, l, on, ptr, col, val, diag, t, x);
        }
        __syncthreads();
    }
}

void free_part(tri_part& p)
{
    for (void** q : {(void**)&p.ptr, (void**)&p.col, (void**)&p.val, (void**)&p.order, (void**)&p.lvl_ptr})
        if (*q)
        {
            (void)hipFree(*q);
            *q = nullptr;
        }
    p.schedule.clear();
}

// The multicolour order of a CSR handle's rows: colour (caller's scratch, [n]) by relaxation to the fixed point, seq ([n]) the
// rows by colour, ascending row index inside a colour, pos ([n]) its inverse.  `who` and `order_param` name the caller in messages.
int colour_order(spmv_ctx* ctx, const spmv_mat* m, const char* who, const char* order_param, int32_t* colour, int32_t* seq, int32_t* pos,
                 int32_t* colours)
{
    const int   n = m->nrow;
    hipStream_t s = ctx->stream;
    SPMV_TRY(ensure_scratch(ctx, 64));
    int* flag = (int*)ctx->scratch;
    (void)hipMemsetAsync(colour, 0, sizeof(int32_t) * (size_t)n, s);
    constexpr int kPasses = 8, kMaxRounds = 1 << 15;
    const unsigned grid = (unsigned)ceil_div(n, kBlock);
    int  h_changed = 1, round = 0;
    for (; round < kMaxRounds && h_changed; ++round)
    {
        (void)hipMemsetAsync(flag, 0, sizeof(int), s);
        for (int k = 0; k < kPasses; ++k) hipLaunchKernelGGL(colour_relax_kernel, dim3(grid), dim3(kBlock), 0, s, n, m->a, m->b, colour, flag);
        if (hipMemcpyAsync(&h_changed, flag, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
            return SPMV_ERR_HIP;
    }
    if (h_changed)
    {
        set_error("%s: colouring did not settle in %d passes (dependency chains that long); %s = 0 will not either", who, kPasses * kMaxRounds,
                  order_param);
        return SPMV_ERR_UNSUPPORTED;
    }
    int32_t h_max = 0;
    (void)hipMemsetAsync(flag, 0, sizeof(int), s);
    hipLaunchKernelGGL(level_max_kernel, dim3((unsigned)std::min<int64_t>(1024, grid)), dim3(kBlock), 0, s, n, colour, (int32_t*)flag);
    if (hipMemcpyAsync(&h_max, flag, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return SPMV_ERR_HIP;
    *colours = h_max + 1;
    int bits = 1;
    while (bits < 31 && (1LL << bits) < (long long)*colours) ++bits;
    SPMV_TRY(sort_ids_by_key(ctx, colour, n, bits, seq));  // by colour, ascending row inside
    hipLaunchKernelGGL(invert_order_kernel, dim3(grid), dim3(kBlock), 0, s, n, seq, pos);
    return SPMV_OK;
}

// levels of one triangle, rows by level, the launch schedule
int analyse_part(spmv_ctx* ctx, int n, tri_part& p, const char* which, const char* who)
{
    hipStream_t s    = ctx->stream;
    int32_t *   lev  = nullptr, *hist = nullptr;
    int         rc   = SPMV_OK;
    const unsigned grid = (unsigned)ceil_div(n, kBlock);
    SPMV_TRY(ensure_scratch(ctx, 64));
    int* flag = (int*)ctx->scratch;
    do
    {
        if (hipMalloc(&lev, sizeof(int32_t) * (size_t)n) != hipSuccess || hipMalloc(&p.order, sizeof(int32_t) * (size_t)n) != hipSuccess)
        {
            rc = SPMV_ERR_ALLOC;
            break;
        }
        if (hipMemsetAsync(lev, 0, sizeof(int32_t) * (size_t)n, s) != hipSuccess)
        {
            rc = SPMV_ERR_HIP;
            break;
        }
        // relax to the fixed point: `kPasses` passes between two looks at the flag; as many passes as the longest chain
        constexpr int kPasses = 8, kMaxRounds = 1 << 15;
        int  round = 0, h_flag = 1;
        for (; round < kMaxRounds && h_flag; ++round)
        {
            (void)hipMemsetAsync(flag, 0, sizeof(int), s);
            for (int k = 0; k < kPasses; ++k) hipLaunchKernelGGL(level_relax_kernel, dim3(grid), dim3(kBlock), 0, s, n, p.ptr, p.col, lev, flag);
            if (hipMemcpyAsync(&h_flag, flag, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
            {
                rc = SPMV_ERR_HIP;
                break;
            }
            // the flag of the LAST pass alone would do; any pass of the round is a safe over-estimate
        }
        if (rc != SPMV_OK) break;
        if (h_flag)
        {
            set_error("%s: the %s triangle has dependency chains longer than %d rows: a sweep in row order is sequential there", who, which,
                      kPasses * kMaxRounds);
            rc = SPMV_ERR_UNSUPPORTED;
            break;
        }
        int32_t h_max = 0;
        (void)hipMemsetAsync(flag, 0, sizeof(int), s);
        hipLaunchKernelGGL(level_max_kernel, dim3((unsigned)std::min<int64_t>(1024, grid)), dim3(kBlock), 0, s, n, lev, (int32_t*)flag);
        if (hipMemcpyAsync(&h_max, flag, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        {
            rc = SPMV_ERR_HIP;
            break;
        }
        const int levels = h_max + 1;
        p.levels         = levels;
        if (hipMalloc(&hist, sizeof(int32_t) * ((size_t)levels + 1)) != hipSuccess || hipMalloc(&p.lvl_ptr, sizeof(int32_t) * ((size_t)levels + 1)) != hipSuccess)
        {
            rc = SPMV_ERR_ALLOC;
            break;
        }
        (void)hipMemsetAsync(hist, 0, sizeof(int32_t) * ((size_t)levels + 1), s);
        hipLaunchKernelGGL(level_hist_kernel, dim3(grid), dim3(kBlock), 0, s, n, lev, hist, levels);
        if ((rc = exclusive_scan_i32(ctx, hist, p.lvl_ptr, (int64_t)levels + 1)) != SPMV_OK) break;
        int bits = 1;
        while (bits < 31 && (1LL << bits) < (long long)levels) ++bits;
        if ((rc = sort_ids_by_key(ctx, lev, n, bits, p.order)) != SPMV_OK) break;
        std::vector<int32_t> lp((size_t)levels + 1);
        if (hipMemcpyAsync(lp.data(), p.lvl_ptr, sizeof(int32_t) * lp.size(), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        {
            rc = SPMV_ERR_HIP;
            break;
        }
        if (lp[0] != 0 || lp[(size_t)levels] != n)
        {
            set_error("%s: the level table of the %s triangle does not cover the rows (%d of %d)", who, which, lp[(size_t)levels], n);
            rc = SPMV_ERR_HIP;
            break;
        }
        const double avg = n > 0 ? (double)p.nnz / n : 0.0;
        p.lanes          = avg <= 2.5 ? 1 : (avg <= 12.0 ? 4 : 16);
        // schedule: runs of small levels share one workgroup, every other level is a launch of its own
        p.schedule.clear();
        for (int lv = 0; lv < levels;)
        {
            const int rows = lp[(size_t)lv + 1] - lp[(size_t)lv];
            if ((int64_t)rows * p.lanes > kSmallLevel)
            {
                p.schedule.push_back({lv, 1, lp[(size_t)lv], rows});
                ++lv;
                continue;
            }
            int end = lv;
            while (end < levels && (int64_t)(lp[(size_t)end + 1] - lp[(size_t)end]) * p.lanes <= kSmallLevel) ++end;
            p.schedule.push_back({lv, end - lv, lp[(size_t)lv], lp[(size_t)end] - lp[(size_t)lv]});
            lv = end;
        }
    } while (0);
    (void)hipStreamSynchronize(s);
    if (lev) (void)hipFree(lev);
    if (hist) (void)hipFree(hist);
    return rc;
}

template <int LANES, bool UNIT>
void launch_solve(hipStream_t s, const tri_part& p, const double* diag, const double* t, double* x)
{
    for (const tri_part::segment& g : p.schedule)
    {
        if (g.rows == 0) continue;
        if (g.nlevels > 1 || (int64_t)g.rows * LANES <= kSolveThreads)
            hipLaunchKernelGGL((tri_solve_run_kernel<LANES, UNIT>), dim3(1), dim3(kSolveThreads), 0, s, g.first_level, g.nlevels, p.lvl_ptr, p.order,
                               p.ptr, p.col, p.val, diag, t, x);
        else
            hipLaunchKernelGGL((tri_solve_level_kernel<LANES, UNIT>), dim3((unsigned)ceil_div((int64_t)g.rows * LANES, kBlock)), dim3(kBlock), 0, s,
                               g.first_row, g.rows, p.order, p.ptr, p.col, p.val, diag, t, x);
    }
}
// (T + D) x = t through the levels of p; UNIT: (T + I) x = t, diag is not read
template <bool UNIT = false>
void solve(hipStream_t s, const tri_part& p, const double* diag, const double* t, double* x)
{
    if (p.lanes == 1)
        launch_solve<1, UNIT>(s, p, diag, t, x);
    else if (p.lanes == 4)
        launch_solve<4, UNIT>(s, p, diag, t, x);
    else
        launch_solve<16, UNIT>(s, p, diag, t, x);
}
}  // namespace
}  // namespace spmv
