// ilu0.hip — ILU(0) on a CSR handle: the incomplete LU factorisation without fill, computed on the device, and its application
// z = U^-1 L^-1 r by two level-scheduled triangular solves (what rocSPARSE and cuSPARSE call csrilu0 and csrsv).  The
// preconditioner of spmv_cg and spmv_bicgstab under SPMV_PRECOND_ILU0; spmv_ilu0_solve applies it on its own.
//
// Definition.  pos[i] is the position of row i in the sweep order ("ilu0_order": 1, the default, the multicolour order of the
// Gauss-Seidel sweep - colour by colour, ascending row index inside a colour; 0 the matrix's own row order, pos[i] = i).  The
// pattern P is the set of (i, j) with at least one stored entry; duplicates are summed first, in stored order.  ILU(0) in sweep
// order is the IKJ elimination restricted to P:
//
//   for i in sweep order:
//       for k in row i with pos[k] < pos[i], ascending pos[k]:
//           l_ik = a_ik / u_kk                                   (a true division)
//           for j in row k with pos[j] > pos[k]:
//               if (i, j) in P:  a_ij = fma(-l_ik, u_kj, a_ij)
//       u_ii = a_ii;  u_ij = a_ij for pos[j] > pos[i]
//
// L is unit lower triangular in sweep order, U upper triangular with the diagonal.  Every entry receives its subtractions in
// ascending pos[k]: one lane eliminates a row, so the order is the loop's.  Two set-ups of one matrix give the same bits.
//
// Set-up (ilu0_setup; synchronous, once per handle and order):
//   order     the colouring of tri_levels.hpp (shared with symgs.hip), or none
//   symbolic  a working copy of the matrix, row by row: the entries sorted by pos of their column (one lane per row, an insertion
//             sort in place: rows are short), duplicates merged, split into the strict lower part, the diagonal and the strict
//             upper part; and `map`, from every stored entry of the handle to its slot in the copy (spmv_ilu0_factors)
//   levels    analyse_part on both parts: rows by level, the launch schedule (tri_levels.hpp)
//   numeric   the elimination, level by level over the LOWER part's levels: row i depends exactly on the rows k of its lower
//             part, so the rows of a level are independent - each reads finished rows only and writes itself; (i, j) is looked
//             up in row i by binary search over pos.  No atomics on values.  A pivot that is zero or not finite: atomicMin on
//             its sweep position, SPMV_ERR_INVALID naming that row, nothing left in the handle.
// Application (ilu0_apply; asynchronous): L y = r forward through the levels of L (unit diagonal: no division; the first level
// is y = r), then U z = y backward through the levels of U, in place in z.  Vectors stay in the matrix's own numbering.  One
// launch per large level, one workgroup per run of small levels: the Gauss-Seidel schedule and its kernels, with a compile-time
// switch for the unit diagonal.  Where several lanes share a row their sums meet in solve_row's fixed tree: deterministic.
#include <climits>
#include <cmath>
#include <cstring>

#include "tri_levels.hpp"

namespace spmv
{
struct ilu0_plan
{
    tri_part lo, up;             // L without its unit diagonal, U without its diagonal; entries of a row ascending in pos of the column
    double*  diag  = nullptr;    // [n] u_ii
    int32_t* seq   = nullptr;    // [n] multicolour order: the k-th row of the sweep (null: the matrix's own order)
    int32_t* map   = nullptr;    // [nnz] slot of every stored entry: lo | up (+ lo.nnz) | diag (+ lo.nnz + up.nnz); -1: a later duplicate
    int32_t  mode    = 0;        // 0 the matrix's own order, 1 multicolour
    int32_t  colours = 0;
    int64_t  bytes   = 0;
};

namespace
{
// ---- symbolic ---------------------------------------------------------------------------------------------------------
// One lane per row: key[j] = pos of the column, src[j] = the stored entry, both sorted by key inside the row (stable: of a set
// of duplicates the first stored one comes first); the counts of distinct columns before and after the diagonal.
__global__ __launch_bounds__(kBlock) void ilu0_sort_count_kernel(int n, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                                 const int32_t* __restrict__ pos, int32_t* __restrict__ key,
                                                                 int32_t* __restrict__ src, int32_t* __restrict__ lo_cnt,
                                                                 int32_t* __restrict__ up_cnt, int* __restrict__ flag)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i > n) return;
    if (i == n)
    {
        lo_cnt[n] = 0;
        up_cnt[n] = 0;
        return;
    }
    const int b = row_ptr[i], e = row_ptr[i + 1], pi = pos ? pos[i] : i;
    for (int j = b; j < e; ++j)
    {
        const int c = col[j], k = pos ? pos[c] : c;
        int       t = j;
        for (; t > b && key[t - 1] > k; --t)
        {
            key[t] = key[t - 1];
            src[t] = src[t - 1];
        }
        key[t] = k;
        src[t] = j;
    }
    int  nl = 0, nu = 0, prev = -1;
    bool has_diag = false;
    for (int j = b; j < e; ++j)
    {
        const int k = key[j];
        if (k == prev) continue;
        prev = k;
        if (k < pi)
            ++nl;
        else if (k == pi)
            has_diag = true;
        else
            ++nu;
    }
    lo_cnt[i] = nl;
    up_cnt[i] = nu;
    if (!has_diag) atomicOr(flag, 1);
}

// the working copy from the sorted rows: duplicates summed in stored order, the map from stored entries to slots
__global__ __launch_bounds__(kBlock) void ilu0_fill_kernel(int n, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                           const double* __restrict__ val, const int32_t* __restrict__ pos,
                                                           const int32_t* __restrict__ key, const int32_t* __restrict__ src,
                                                           const int32_t* __restrict__ lo_ptr, const int32_t* __restrict__ up_ptr,
                                                           int32_t* __restrict__ lo_col, double* __restrict__ lo_val,
                                                           int32_t* __restrict__ up_col, double* __restrict__ up_val,
                                                           double* __restrict__ diag, int32_t* __restrict__ map)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int e = row_ptr[i + 1], pi = pos ? pos[i] : i;
    const int lo_nnz = lo_ptr[n], up_nnz = up_ptr[n];
    int       pl = lo_ptr[i], pu = up_ptr[i];
    for (int j = row_ptr[i]; j < e;)
    {
        const int k = key[j], first = src[j];
        double    v = 0.0;
        int       q = j;
        for (; q < e && key[q] == k; ++q)
        {
            v += val[src[q]];
            map[src[q]] = -1;
        }
        if (k < pi)
        {
            lo_col[pl] = col[first];
            lo_val[pl] = v;
            map[first] = pl++;
        }
        else if (k == pi)
        {
            diag[i]    = v;
            map[first] = lo_nnz + up_nnz + i;
        }
        else
        {
            up_col[pu] = col[first];
            up_val[pu] = v;
            map[first] = lo_nnz + pu++;
        }
        j = q;
    }
}

// ---- numeric ----------------------------------------------------------------------------------------------------------
// the slot in [b, e) whose column has sweep position `want` (the entries ascend in it), or -1
__device__ __forceinline__ int ilu0_find(const int32_t* __restrict__ col, const int32_t* __restrict__ pos, int b, int e, int want)
{
    while (b < e)
    {
        const int mid = b + ((e - b) >> 1), c = col[mid], pc = pos ? pos[c] : c;
        if (pc == want) return mid;
        if (pc < want)
            b = mid + 1;
        else
            e = mid;
    }
    return -1;
}

// The elimination of row i, by one lane.  It reads the upper parts and pivots of rows of earlier levels (finished; other lanes of
// this launch write their own rows only) and writes row i's values.  The value arrays are not __restrict__: in the folded kernel a
// level reads what the level before it wrote.
__device__ __forceinline__ void ilu0_row(int i, const int32_t* __restrict__ pos, const int32_t* __restrict__ lo_ptr,
                                         const int32_t* __restrict__ lo_col, double* lo_val, const int32_t* __restrict__ up_ptr,
                                         const int32_t* __restrict__ up_col, double* up_val, double* diag, int* bad_pos)
{
    const int pi = pos ? pos[i] : i;
    const int le = lo_ptr[i + 1], ub = up_ptr[i], ue = up_ptr[i + 1];
    double    d  = diag[i];
    for (int a = lo_ptr[i]; a < le; ++a)  // ascending pos[k]
    {
        const int    k = lo_col[a];
        const double l = lo_val[a] / diag[k];
        lo_val[a]      = l;
        for (int q = up_ptr[k]; q < up_ptr[k + 1]; ++q)
        {
            const int    j = up_col[q], pj = pos ? pos[j] : j;
            const double u = up_val[q];
            if (pj == pi)
                d = fma(-l, u, d);
            else if (pj < pi)  // (pos[j] > pos[k]: behind slot a)
            {
                const int s = ilu0_find(lo_col, pos, a + 1, le, pj);
                if (s >= 0) lo_val[s] = fma(-l, u, lo_val[s]);
            }
            else
            {
                const int s = ilu0_find(up_col, pos, ub, ue, pj);
                if (s >= 0) up_val[s] = fma(-l, u, up_val[s]);
            }
        }
    }
    diag[i] = d;
    if (!(d != 0.0) || !isfinite(d)) atomicMin(bad_pos, pi);
}

// one level of the lower part: rows order[first .. first + rows)
__global__ __launch_bounds__(kBlock) void ilu0_factor_level_kernel(int first, int rows, const int32_t* __restrict__ order,
                                                                   const int32_t* __restrict__ pos, const int32_t* __restrict__ lo_ptr,
                                                                   const int32_t* __restrict__ lo_col, double* lo_val,
                                                                   const int32_t* __restrict__ up_ptr, const int32_t* __restrict__ up_col,
                                                                   double* up_val, double* diag, int* bad_pos)
{
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r < rows) ilu0_row(order[first + r], pos, lo_ptr, lo_col, lo_val, up_ptr, up_col, up_val, diag, bad_pos);
}

// a run of small levels in one workgroup, as tri_solve_run_kernel steps through them
__global__ __launch_bounds__(kSolveThreads) void ilu0_factor_run_kernel(int first_level, int nlevels, const int32_t* __restrict__ lvl_ptr,
                                                                        const int32_t* __restrict__ order, const int32_t* __restrict__ pos,
                                                                        const int32_t* __restrict__ lo_ptr, const int32_t* __restrict__ lo_col,
                                                                        double* lo_val, const int32_t* __restrict__ up_ptr,
                                                                        const int32_t* __restrict__ up_col, double* up_val, double* diag,
                                                                        int* bad_pos)
{
    for (int lv = first_level; lv < first_level + nlevels; ++lv)
    {
        const int first = lvl_ptr[lv], rows = lvl_ptr[lv + 1] - first;
        for (int base = 0; base < rows; base += kSolveThreads)  // (uniform bounds: every lane reaches the barrier)
        {
            const int r = base + (int)threadIdx.x;
            if (r < rows) ilu0_row(order[first + r], pos, lo_ptr, lo_col, lo_val, up_ptr, up_col, up_val, diag, bad_pos);
        }
        __syncthreads();
    }
}

// the factor values in the order of the handle's own entries
__global__ __launch_bounds__(kBlock) void ilu0_gather_kernel(int64_t nnz, const int32_t* __restrict__ map, int32_t lo_nnz, int32_t up_nnz,
                                                             const double* __restrict__ lo_val, const double* __restrict__ up_val,
                                                             const double* __restrict__ diag, double* __restrict__ out)
{
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < nnz; j += (int64_t)gridDim.x * kBlock)
    {
        const int s = map[j];
        out[j]      = s < 0 ? 0.0 : (s < lo_nnz ? lo_val[s] : (s < lo_nnz + up_nnz ? up_val[s - lo_nnz] : diag[s - lo_nnz - up_nnz]));
    }
}

size_t launches_of(const tri_part& p)
{
    size_t k = 0;
    for (const tri_part::segment& g : p.schedule) k += g.rows > 0;
    return k;
}
}  // namespace

// the handles ILU(0) takes, checked on the host: a CSR handle that holds the whole square matrix and still has its arrays
int ilu0_check_handle(const spmv_mat* m, const char* who) { return check_whole_square_csr(m, who, "ILU(0)"); }

void ilu0_free(spmv_mat* m)
{
    if (!m->ilu) return;
    free_part(m->ilu->lo);
    free_part(m->ilu->up);
    for (void* q : {(void*)m->ilu->diag, (void*)m->ilu->seq, (void*)m->ilu->map})
        if (q) (void)hipFree(q);
    m->device_bytes -= m->ilu->bytes;
    delete m->ilu;
    m->ilu = nullptr;
}

int ilu0_setup(spmv_mat* m)
{
    const int32_t mode = m->ilu_order != 0 ? 1 : 0;
    if (m->ilu && m->ilu->mode == mode) return SPMV_OK;
    ilu0_free(m);  // (another order was asked for since)
    SPMV_TRY(ilu0_check_handle(m, "spmv_ilu0_setup"));
    const int n = m->nrow;
    SPMV_REQUIRE(m->nnz + (int64_t)n < INT32_MAX, "spmv_ilu0_setup: %lld entries and %d rows: the slots of the factors are 32-bit", (long long)m->nnz, n);
    spmv_ctx*   ctx = m->ctx;
    hipStream_t s   = ctx->stream;
    SPMV_TRY(ensure_scratch(ctx, 64));  // (before the plan is attached: a failure here leaves no half-built plan behind)
    ilu0_plan* g = new ilu0_plan();
    g->mode      = mode;
    m->ilu       = g;
    if (n == 0) return SPMV_OK;
    int32_t *lo_cnt = nullptr, *up_cnt = nullptr, *colour = nullptr, *pos = nullptr, *key = nullptr, *src = nullptr;
    int      rc      = SPMV_OK;
    int*     flag    = (int*)ctx->scratch;
    int      bad_row = -1;
    const size_t nz  = std::max<size_t>(1, (size_t)m->nnz);
    do
    {
        if (mode == 1)
        {
            if (hipMalloc(&colour, sizeof(int32_t) * (size_t)n) != hipSuccess || hipMalloc(&pos, sizeof(int32_t) * (size_t)n) != hipSuccess ||
                hipMalloc(&g->seq, sizeof(int32_t) * (size_t)n) != hipSuccess)
            {
                rc = SPMV_ERR_ALLOC;
                break;
            }
            if ((rc = colour_order(ctx, m, "spmv_ilu0_setup", "ilu0_order", colour, g->seq, pos, &g->colours)) != SPMV_OK) break;
        }
        if (hipMalloc(&lo_cnt, sizeof(int32_t) * ((size_t)n + 1)) != hipSuccess || hipMalloc(&up_cnt, sizeof(int32_t) * ((size_t)n + 1)) != hipSuccess ||
            hipMalloc(&g->lo.ptr, sizeof(int32_t) * ((size_t)n + 1)) != hipSuccess || hipMalloc(&g->up.ptr, sizeof(int32_t) * ((size_t)n + 1)) != hipSuccess ||
            hipMalloc(&g->diag, sizeof(double) * (size_t)n) != hipSuccess || hipMalloc(&key, sizeof(int32_t) * nz) != hipSuccess ||
            hipMalloc(&src, sizeof(int32_t) * nz) != hipSuccess || hipMalloc(&g->map, sizeof(int32_t) * nz) != hipSuccess)
        {
            rc = SPMV_ERR_ALLOC;
            break;
        }
        // symbolic: sorted rows and the counts of both parts
        (void)hipMemsetAsync(flag, 0, sizeof(int), s);
        hipLaunchKernelGGL(ilu0_sort_count_kernel, dim3((unsigned)ceil_div((int64_t)n + 1, kBlock)), dim3(kBlock), 0, s, n, m->a, m->b, pos, key, src,
                           lo_cnt, up_cnt, flag);
        int h_flag = 0;  // (read before the scans: they use the context's scratch too)
        if (hipMemcpyAsync(&h_flag, flag, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        {
            rc = SPMV_ERR_HIP;
            break;
        }
        if (h_flag)
        {
            set_error("spmv_ilu0_setup: the matrix has a row without a diagonal entry");
            rc = SPMV_ERR_INVALID;
            break;
        }
        if ((rc = exclusive_scan_i32(ctx, lo_cnt, g->lo.ptr, (int64_t)n + 1)) != SPMV_OK) break;
        if ((rc = exclusive_scan_i32(ctx, up_cnt, g->up.ptr, (int64_t)n + 1)) != SPMV_OK) break;
        int32_t h_lo = 0, h_up = 0;
        if (hipMemcpyAsync(&h_lo, g->lo.ptr + n, sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipMemcpyAsync(&h_up, g->up.ptr + n, sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        {
            rc = SPMV_ERR_HIP;
            break;
        }
        if (h_lo < 0 || h_up < 0 || (int64_t)h_lo + h_up + n > m->nnz)
        {
            set_error("spmv_ilu0_setup: splitting the matrix gave %d + %d + %d entries of %lld", h_lo, h_up, n, (long long)m->nnz);
            rc = SPMV_ERR_HIP;
            break;
        }
        g->lo.nnz = h_lo;
        g->up.nnz = h_up;
        if (hipMalloc(&g->lo.col, sizeof(int32_t) * std::max<size_t>(1, (size_t)h_lo)) != hipSuccess ||
            hipMalloc(&g->lo.val, sizeof(double) * std::max<size_t>(1, (size_t)h_lo)) != hipSuccess ||
            hipMalloc(&g->up.col, sizeof(int32_t) * std::max<size_t>(1, (size_t)h_up)) != hipSuccess ||
            hipMalloc(&g->up.val, sizeof(double) * std::max<size_t>(1, (size_t)h_up)) != hipSuccess)
        {
            rc = SPMV_ERR_ALLOC;
            break;
        }
        hipLaunchKernelGGL(ilu0_fill_kernel, dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0, s, n, m->a, m->b, m->v, pos, key, src, g->lo.ptr,
                           g->up.ptr, g->lo.col, g->lo.val, g->up.col, g->up.val, g->diag, g->map);
        if (hipGetLastError() != hipSuccess)
        {
            rc = SPMV_ERR_HIP;
            break;
        }
        if ((rc = analyse_part(ctx, n, g->lo, "lower", "spmv_ilu0_setup")) != SPMV_OK) break;
        if ((rc = analyse_part(ctx, n, g->up, "upper", "spmv_ilu0_setup")) != SPMV_OK) break;
        // numeric: the elimination through the lower part's schedule, one lane per row
        const int h_none = INT_MAX;
        if (hipMemcpyAsync(flag, &h_none, sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        {
            rc = SPMV_ERR_HIP;
            break;
        }
        for (const tri_part::segment& sg : g->lo.schedule)
        {
            if (sg.rows == 0) continue;
            if (sg.nlevels > 1 || sg.rows <= kSolveThreads)
                hipLaunchKernelGGL(ilu0_factor_run_kernel, dim3(1), dim3(kSolveThreads), 0, s, sg.first_level, sg.nlevels, g->lo.lvl_ptr, g->lo.order, pos,
                                   g->lo.ptr, g->lo.col, g->lo.val, g->up.ptr, g->up.col, g->up.val, g->diag, flag);
            else
                hipLaunchKernelGGL(ilu0_factor_level_kernel, dim3((unsigned)ceil_div(sg.rows, kBlock)), dim3(kBlock), 0, s, sg.first_row, sg.rows,
                                   g->lo.order, pos, g->lo.ptr, g->lo.col, g->lo.val, g->up.ptr, g->up.col, g->up.val, g->diag, flag);
        }
        int h_bad = INT_MAX;
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&h_bad, flag, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
        {
            rc = SPMV_ERR_HIP;
            break;
        }
        if (h_bad != INT_MAX)
        {
            // the offending row with the smallest sweep position: every later one may only be its consequence
            bad_row = h_bad;
            if (g->seq && (h_bad < 0 || h_bad >= n || hipMemcpy(&bad_row, g->seq + h_bad, sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess))
            {
                rc = SPMV_ERR_HIP;
                break;
            }
            set_error("spmv_ilu0_setup: the pivot of row %d (sweep position %d) is zero or not finite: ILU(0) does not exist in this order", bad_row,
                      h_bad);
            rc = SPMV_ERR_INVALID;
            break;
        }
    } while (0);
    (void)hipStreamSynchronize(s);
    for (int32_t* q : {lo_cnt, up_cnt, colour, pos, key, src})
        if (q) (void)hipFree(q);
    if (rc != SPMV_OK)
    {
        ilu0_free(m);
        if (rc == SPMV_ERR_ALLOC) set_error("spmv_ilu0_setup: out of device memory factorising a matrix of %lld entries", (long long)m->nnz);
        if (rc == SPMV_ERR_HIP && hipGetLastError() != hipSuccess) set_error("spmv_ilu0_setup: set-up failed: %s", hipGetErrorString(hipGetLastError()));
        return rc;
    }
    // col + val of both parts, ptr and order of both, diag, seq, map, the level tables
    g->bytes = (g->lo.nnz + g->up.nnz) * 12 + (int64_t)n * (4 + 4 + 4 + 4 + 8 + (g->seq ? 4 : 0)) + 8 + m->nnz * 4 +
               (int64_t)(g->lo.levels + g->up.levels + 2) * 4;
    m->device_bytes += g->bytes;
    return SPMV_OK;
}

// z = U^-1 L^-1 r; r and z must not overlap (the backward solve runs in place in z)
int ilu0_apply(spmv_ctx* ctx, const spmv_mat* A, const double* r, double* z)
{
    const ilu0_plan* g = A->ilu;
    if (!g) SPMV_FAIL(SPMV_ERR_INVALID, "spmv_ilu0_solve: the handle was not set up");
    if (A->nrow == 0) return SPMV_OK;
    if (!g->lo.ptr || !g->up.ptr || !g->lo.order || !g->up.order || !g->lo.lvl_ptr || !g->up.lvl_ptr || !g->diag || !r || !z)
        SPMV_FAIL(SPMV_ERR_INVALID, "spmv_ilu0_solve: the factorisation of this handle is incomplete");
    hipStream_t s = ctx->stream;
    solve<true>(s, g->lo, nullptr, r, z);   // L y = r, y into z
    solve<false>(s, g->up, g->diag, z, z);  // U z = y
    SPMV_HIP(hipGetLastError());
    return SPMV_OK;
}

// the factor values aligned to the handle's own entries, to the host
int ilu0_factor_values(const spmv_mat* m, double* out)
{
    const ilu0_plan* g = m->ilu;
    if (!g) SPMV_FAIL(SPMV_ERR_INVALID, "spmv_ilu0_factors: the handle was not set up (spmv_ilu0_setup)");
    if (m->nnz == 0 || m->nrow == 0) return SPMV_OK;
    hipStream_t s   = m->ctx->stream;
    double*     tmp = nullptr;
    if (hipMalloc(&tmp, sizeof(double) * (size_t)m->nnz) != hipSuccess)
        SPMV_FAIL(SPMV_ERR_ALLOC, "spmv_ilu0_factors: out of device memory for %lld values", (long long)m->nnz);
    hipLaunchKernelGGL(ilu0_gather_kernel, dim3(stream_grid(m->nnz)), dim3(kBlock), 0, s, m->nnz, g->map, (int32_t)g->lo.nnz, (int32_t)g->up.nnz,
                       g->lo.val, g->up.val, g->diag, tmp);
    const bool ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(out, tmp, sizeof(double) * (size_t)m->nnz, hipMemcpyDeviceToHost, s) == hipSuccess &&
                    hipStreamSynchronize(s) == hipSuccess;
    (void)hipFree(tmp);
    if (!ok) SPMV_FAIL(SPMV_ERR_HIP, "spmv_ilu0_factors: reading the factors failed: %s", hipGetErrorString(hipGetLastError()));
    return SPMV_OK;
}

// the k-th row of the sweep, to the host
int ilu0_sequence(const spmv_mat* m, int32_t* out)
{
    const ilu0_plan* g = m->ilu;
    if (!g) SPMV_FAIL(SPMV_ERR_INVALID, "spmv_ilu0_order: the handle was not set up (spmv_ilu0_setup)");
    if (!g->seq)
    {
        for (int32_t i = 0; i < m->nrow; ++i) out[i] = i;
        return SPMV_OK;
    }
    SPMV_HIP(hipMemcpyAsync(out, g->seq, sizeof(int32_t) * (size_t)m->nrow, hipMemcpyDeviceToHost, m->ctx->stream));
    SPMV_HIP(hipStreamSynchronize(m->ctx->stream));
    return SPMV_OK;
}

bool ilu0_get_param(const spmv_mat* m, const char* what, int64_t* value)
{
    const ilu0_plan* g = m->ilu;
    if (!strcmp(what, "ilu0_order"))
        *value = m->ilu_order != 0 ? 1 : 0;
    else if (!strcmp(what, "ilu0_ready"))  // 1: factorised in the order now asked for
        *value = g && g->mode == (m->ilu_order != 0 ? 1 : 0) ? 1 : 0;
    else if (!strcmp(what, "ilu0_colours"))  // 0: the matrix's own order
        *value = g ? g->colours : 0;
    else if (!strcmp(what, "ilu0_levels_forward"))
        *value = g ? g->lo.levels : 0;
    else if (!strcmp(what, "ilu0_levels_backward"))
        *value = g ? g->up.levels : 0;
    else if (!strcmp(what, "ilu0_launches"))  // per application: the two schedules
        *value = g ? (int64_t)(launches_of(g->lo) + launches_of(g->up)) : 0;
    else if (!strcmp(what, "ilu0_bytes"))
        *value = g ? g->bytes : 0;
    else
        return false;
    return true;
}

// "ilu0_order": 1 multicolour, 0 the matrix's own row order; takes effect at the next set-up / application
bool ilu0_set_param(spmv_mat* m, const char* name, int64_t value, int* rc)
{
    if (strcmp(name, "ilu0_order")) return false;
    *rc = value == 0 || value == 1 ? SPMV_OK : SPMV_ERR_INVALID;
    if (*rc == SPMV_OK)
        m->ilu_order = (int32_t)value;
    else
        set_error("ilu0_order: 0 (row order) or 1 (multicolour), got %lld", (long long)value);
    return true;
}
}  // namespace spmv
