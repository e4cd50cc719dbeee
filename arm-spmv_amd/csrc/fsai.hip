// fsai.hip — FSAI, the factorised sparse approximate inverse (Kolotilina-Yeremin) of a symmetric positive definite CSR handle: a
// sparse lower-triangular G with G A G^T ~ I, computed on the device, and its application z = G^T (G r) by two forward products.
// The preconditioner of spmv_cg, spmv_bicgstab, spmv_gmres and spmv_lobpcg under SPMV_PRECOND_FSAI; spmv_fsai_solve applies it on
// its own.  tests/fsai_ref.py is the NumPy twin of the definition below (include/spmv_abi.h states it as the contract).
//
// Definition.  The pattern S is the lower triangle, diagonal included, of the structural pattern of A^level (level 1, 2 or 3): every
// stored entry counts, zeros included; a row of S holds distinct columns in ascending order and ends at the row itself.  For row i
// with J = S_i and m = |J| <= kFsaiMaxRow, M = A[J, J], read from the LOWER triangle of A alone: entry (p, q), q <= p, is the sum
// of the stored entries (J_p, J_q) of row J_p of A, from 0.0 in stored order.  Symmetry is not checked.  M = C C^T by the
// right-looking Cholesky factorisation below (a true square root, true divisions, one fma per update); row i of G is the solution g
// of C^T g = e_m by back substitution from the last unknown up, so g_ii = 1 / c_mm.
//
//   for k = 0 .. m-1:   c_kk = sqrt(m_kk);   c_pk = m_pk / c_kk (p > k);   m_pq = fma(-c_pk, c_qk, m_pq)  (k < q <= p)
//   t = e_m;  for p = m-1 .. 0:   g_p = t_p / c_pp;   t_a = fma(-c_pa, g_p, t_a)  (a < p)
//
// Set-up (fsai_setup; synchronous, replaces earlier state):
//   pattern   level 1: A's own rows.  Level 2 and 3: spgemm's A A and (A A) A - their columns ascend already.  One lane per row
//             copies the columns <= i into a key buffer, sorts them (an insertion sort: linear on ascending input, and rows are
//             short), drops duplicates and counts; the scan of the counts is G's row_ptr, a second pass writes G's columns.  The
//             same launch finds the first row without a diagonal entry, the first row above the cap, the longest row and the rows per
//             lane class, with integer atomics.  No host round trip but those counters.
//   rows      the rows listed by lane class (fsai_settings.hpp; one stable pass of sort_ids_by_key), one launch per non-empty class:
//             fsai_rows_kernel below.  A pivot that is not positive or not finite: atomicMin on the row.
//   handles   G is a CSR handle of its own, analysed like any other (AUTO picks its kernel); G^T comes from csr_transpose.
// Application (fsai_apply; asynchronous): w = G r, z = G^T w, both through mat_apply_ex's overwrite path: two products, one work
// vector.  G holds the same bits after every set-up; the products are the engine's, deterministic for the kernels AUTO's model
// picks (a timing trial may pick another one on another day: "panel_trial" 0 on A is handed down to G and G^T).
#include <chrono>
#include <climits>
#include <cmath>

#include "fsai_settings.hpp"
#include "solver_host.hpp"
#include "sorted_runs.hpp"

namespace spmv
{
struct fsai_state
{
    spmv_mat* G  = nullptr;  // lower triangular, rows ascending in column, the diagonal last
    spmv_mat* Gt = nullptr;
    double*   w  = nullptr;  // [n] G r
    int32_t   level = 0, max_row = 0;
    int64_t   nnz = 0, bytes = 0;
    int64_t   us_pattern = 0, us_rows = 0, us_handles = 0;  // wall time of the last set-up by phase ("fsai_setup_us_*")
};

namespace
{
// the counters of one set-up (int32, on the device)
enum : int
{
    kFlagNoDiag = 0,  // the smallest row without a stored diagonal entry (INT_MAX: none)
    kFlagLong   = 1,  // the smallest row with more than kFsaiMaxRow pattern columns (INT_MAX: none)
    kFlagMax    = 2,  // the longest row of S
    kFlagClass  = 3,  // [kFsaiClasses] rows per lane class
    kFlagPivot  = 8,  // the smallest row whose factorisation met a pivot that is not positive or not finite (INT_MAX: none)
    kFlagCount  = 9
};
static_assert(kFlagClass + kFsaiClasses == kFlagPivot, "one counter per class");
static_assert(kFsaiMaxRow == SPMV_FSAI_MAX_ROW && fsai_lanes(kFsaiClasses - 1) == kFsaiMaxRow, "the cap of the contract is the widest group");

// One lane per row of the pattern's source: key[rp[i] ..) = its distinct columns <= i, ascending; cnt[i] how many; cls[i] the
// lane class; the counters.  cnt[n] = 0 for the scan.
__global__ __launch_bounds__(kBlock) void fsai_lower_count_kernel(int n, const int32_t* __restrict__ rp, const int32_t* __restrict__ col,
                                                                  int32_t* __restrict__ key, int32_t* __restrict__ cnt,
                                                                  int32_t* __restrict__ cls, int* __restrict__ flags)
{
    __shared__ int s_cls[kFsaiClasses];
    if (threadIdx.x < kFsaiClasses) s_cls[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i == n) cnt[n] = 0;
    if (i < n)
    {
        const int b = rp[i], e = rp[i + 1];
        int       t = b;
        for (int j = b; j < e; ++j)
        {
            const int c = col[j];
            if (c > i) continue;
            int s = t;  // (t <= j: the slot was read already)
            for (; s > b && key[s - 1] > c; --s) key[s] = key[s - 1];
            key[s] = c;
            ++t;
        }
        int m = 0, prev = -1;
        for (int j = b; j < t; ++j)
        {
            const int k = key[j];
            if (k == prev) continue;
            key[b + m++] = k;
            prev         = k;
        }
        cnt[i]      = m;
        const int c = fsai_class_of(m);
        cls[i]      = c < kFsaiClasses ? c : kFsaiClasses - 1;
        if (prev != i) atomicMin(flags + kFlagNoDiag, i);
        if (m > kFsaiMaxRow) atomicMin(flags + kFlagLong, i);
        atomicMax(flags + kFlagMax, m);
        if (c < kFsaiClasses) atomicAdd(&s_cls[c], 1);
    }
    __syncthreads();
    if (threadIdx.x < kFsaiClasses && s_cls[threadIdx.x]) atomicAdd(flags + kFlagClass + threadIdx.x, s_cls[threadIdx.x]);
}

// G's columns from the keys: one lane per row
__global__ __launch_bounds__(kBlock) void fsai_lower_fill_kernel(int n, const int32_t* __restrict__ rp, const int32_t* __restrict__ key,
                                                                 const int32_t* __restrict__ g_rp, int32_t* __restrict__ g_col)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int b = rp[i], gb = g_rp[i], m = g_rp[i + 1] - gb;
    for (int q = 0; q < m; ++q) g_col[gb + q] = key[b + q];
}

// The lanes of a group are lanes of one wavefront, whose LDS accesses complete in the order they were issued: what a lane wrote
// before this point, the group's other lanes read behind it.  The fence keeps the compiler from moving accesses across.
__device__ __forceinline__ void fsai_group_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// One group of L lanes per listed row (every listed row has 1 <= m <= L pattern columns).  No workgroup barrier: the groups of a
// workgroup go their own ways.  Lane a owns row a of M: it alone adds into it, so the sums are those of the stored order.
template <int L>
__global__ __launch_bounds__(fsai_block_lanes(L)) void fsai_rows_kernel(int64_t nlist, const int32_t* __restrict__ rows,
                                                                        const int32_t* __restrict__ a_rp, const int32_t* __restrict__ a_col,
                                                                        const double* __restrict__ a_val, const int32_t* __restrict__ g_rp,
                                                                        const int32_t* __restrict__ g_col, double* __restrict__ g_val,
                                                                        int* __restrict__ bad_row)
{
    constexpr int GROUPS = fsai_groups_per_block(L), TRI = (int)fsai_tri(L);
    static_assert(GROUPS * (TRI * 8 + L * 8 + L * 4) == fsai_block_lds_bytes(L) && fsai_block_lds_bytes(L) <= kFsaiLdsPerBlock, "the settings' LDS");
    static_assert(L <= kFsaiWave && kFsaiWave % L == 0, "a group lies inside a wavefront");
    __shared__ double  s_m[GROUPS * TRI];
    __shared__ double  s_g[GROUPS * L];
    __shared__ int32_t s_j[GROUPS * L];
    const int      grp = threadIdx.x / L, a = threadIdx.x % L;
    double* const  M   = s_m + grp * TRI;
    double* const  gv  = s_g + grp * L;
    int32_t* const J   = s_j + grp * L;
    double* const  Ma  = M + (int)fsai_tri(a);  // lane a's row of M
    const int64_t  nblocks = (nlist + GROUPS - 1) / GROUPS;
    for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x)
    {
        const int64_t k = blk * GROUPS + grp;
        if (k >= nlist) continue;  // (the whole group)
        const int i  = rows[k];
        const int gb = g_rp[i], m = g_rp[i + 1] - gb;
        const int tm = (int)fsai_tri(m);
        fsai_group_sync();  // (the row before this one is read out)
        if (a < m) J[a] = g_col[gb + a];
        for (int t = a; t < tm; t += L) M[t] = 0.0;
        fsai_group_sync();
        // M = A[J, J], the lower triangle: lane a walks row J[a] of A and places the columns it finds in J[0 .. a]
        if (a < m)
        {
            const int p = J[a], end = a_rp[p + 1];
            for (int e = a_rp[p]; e < end; ++e)
            {
                const int c = a_col[e];
                if (c > p) continue;
                int lo = 0, hi = a + 1;
                while (lo < hi)
                {
                    const int mid = (lo + hi) >> 1;
                    if (J[mid] < c)
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                if (lo <= a && J[lo] == c) Ma[lo] += a_val[e];
            }
        }
        fsai_group_sync();
        // right-looking Cholesky: the lanes across column k, then lane a across its row of the trailing matrix
        bool ok = true;
        for (int kk = 0; kk < m; ++kk)
        {
            const double d = M[(int)fsai_tri(kk) + kk];  // (the same word for the whole group)
            if (!(d > 0.0) || !isfinite(d))
            {
                ok = false;
                break;
            }
            const double c  = sqrt(d);
            double       lk = 0.0;
            fsai_group_sync();  // (every lane has read d)
            if (a == kk) Ma[kk] = c;
            if (a > kk && a < m)
            {
                lk     = Ma[kk] / c;
                Ma[kk] = lk;
            }
            fsai_group_sync();
            if (a > kk && a < m)
                for (int q = kk + 1; q <= a; ++q) Ma[q] = fma(-lk, M[(int)fsai_tri(q) + kk], Ma[q]);
            fsai_group_sync();
        }
        if (!ok)
        {
            if (a == 0) atomicMin(bad_row, i);
            continue;
        }
        // C^T g = e_m from the last unknown up: lane a keeps t_a, lane p publishes g_p
        double t = a == m - 1 ? 1.0 : 0.0;
        for (int p = m - 1; p >= 0; --p)
        {
            if (a == p) gv[p] = t / Ma[p];
            fsai_group_sync();
            if (a < p) t = fma(-M[(int)fsai_tri(p) + a], gv[p], t);
        }
        if (a < m) g_val[gb + a] = gv[a];  // (its own word)
    }
}

template <int L>
void launch_rows(hipStream_t s, int64_t nlist, const int32_t* rows, const spmv_mat* A, const spmv_mat* G, int* bad_row)
{
    const int64_t nblocks = ceil_div(nlist, fsai_groups_per_block(L));
    hipLaunchKernelGGL((fsai_rows_kernel<L>), dim3((unsigned)std::min<int64_t>(kMaxGrid, nblocks)), dim3(fsai_block_lanes(L)), 0, s, nlist, rows, A->a,
                       A->b, A->v, G->a, G->b, const_cast<double*>(G->v), bad_row);
}

void state_free(fsai_state* st)
{
    if (!st) return;
    if (st->G) mat_free(st->G);
    if (st->Gt) mat_free(st->Gt);
    if (st->w) (void)hipFree(st->w);
    delete st;
}
}  // namespace

// the handles FSAI takes, checked on the host: a CSR handle that holds the whole square matrix and still has its arrays
int fsai_check_handle(const spmv_mat* m, const char* who) { return check_whole_square_csr(m, who, "FSAI"); }

int fsai_check_level(int32_t level, const char* who)
{
    SPMV_REQUIRE(level >= 0 && level <= 3, "%s: level=%d, must be 1 .. 3 (0: the handle's \"fsai_level\")", who, level);
    return SPMV_OK;
}

void fsai_free(spmv_mat* m)
{
    state_free(m->fsai);
    m->fsai = nullptr;
}

int fsai_setup(spmv_ctx* ctx, spmv_mat* m, int32_t level)
{
    const char* const who = "spmv_fsai_setup";
    SPMV_TRY(fsai_check_level(level, who));
    SPMV_TRY(fsai_check_handle(m, who));
    const int lvl = level == 0 ? m->fsai_level : level;
    const int n   = m->nrow;
    if (n == 0)
    {
        fsai_free(m);
        m->fsai        = new fsai_state();
        m->fsai->level = lvl;
        return SPMV_OK;
    }
    hipStream_t s = ctx->stream;
    using clock   = std::chrono::steady_clock;
    auto us_since = [](clock::time_point t) { return (int64_t)std::chrono::duration_cast<std::chrono::microseconds>(clock::now() - t).count(); };
    const clock::time_point t_begin = clock::now();
    int64_t                 us_pattern = 0, us_rows = 0;
    // the pattern's source: A, A A or (A A) A; the products' handles run the row-parallel kernel (nothing is multiplied with them)
    spmv_mat* P = nullptr;
    if (lvl >= 2) SPMV_TRY(spgemm(ctx, m, m, SPMV_SPGEMM_AUTO, &P, SPMV_CSR_VECTOR));
    if (lvl == 3)
    {
        spmv_mat* P3 = nullptr;
        const int rc = spgemm(ctx, P, m, SPMV_SPGEMM_AUTO, &P3, SPMV_CSR_VECTOR);
        mat_free(P);
        SPMV_TRY(rc);
        P = P3;
    }
    const spmv_mat* src = P ? P : m;
    fsai_state*     st  = nullptr;
    int             rc  = SPMV_OK;
    bool            keep_old = false;  // a refusal that leaves the state of an earlier set-up in the handle
    {
        device_pool pool(ctx, who);
        int32_t *   key = nullptr, *cnt = nullptr, *cls = nullptr, *ids = nullptr, *g_rp = nullptr;
        int*        flags = nullptr;
        int         h[kFlagCount];
        do
        {
            if ((rc = pool.get(key, (size_t)src->nnz)) != SPMV_OK || (rc = pool.get(cnt, (size_t)n + 1)) != SPMV_OK ||
                (rc = pool.get(cls, (size_t)n)) != SPMV_OK || (rc = pool.get(ids, (size_t)n)) != SPMV_OK ||
                (rc = pool.get(g_rp, (size_t)n + 1)) != SPMV_OK || (rc = pool.get(flags, (size_t)kFlagCount)) != SPMV_OK)
                break;
            for (int f = 0; f < kFlagCount; ++f) h[f] = 0;
            h[kFlagNoDiag] = h[kFlagLong] = h[kFlagPivot] = INT_MAX;
            if ((rc = write_scalars(ctx, flags, h, sizeof(h), who, "writing the counters")) != SPMV_OK) break;
            hipLaunchKernelGGL(fsai_lower_count_kernel, dim3((unsigned)ceil_div((int64_t)n + 1, kBlock)), dim3(kBlock), 0, s, n, src->a, src->b, key, cnt,
                               cls, flags);
            if ((rc = hip_step(hipGetLastError(), who, "the pattern's launch")) != SPMV_OK) break;
            if ((rc = read_scalars(ctx, h, flags, sizeof(h), who)) != SPMV_OK) break;
            if (h[kFlagNoDiag] != INT_MAX)
            {
                set_error("%s: row %d has no stored diagonal entry", who, h[kFlagNoDiag]);
                rc = SPMV_ERR_INVALID;
                break;
            }
            if (h[kFlagLong] != INT_MAX)
            {
                int32_t len = 0;
                if ((rc = read_scalars(ctx, &len, cnt + h[kFlagLong], sizeof(len), who)) != SPMV_OK) break;
                set_error("%s: row %d has m = %d pattern columns at level %d, the cap is %d (the longest row has %d)", who, h[kFlagLong], len, lvl,
                          kFsaiMaxRow, h[kFlagMax]);
                rc       = SPMV_ERR_UNSUPPORTED;
                keep_old = true;
                break;
            }
            if ((rc = exclusive_scan_i32(ctx, cnt, g_rp, (int64_t)n + 1)) != SPMV_OK) break;
            int32_t g_nnz = 0;
            if ((rc = read_scalars(ctx, &g_nnz, g_rp + n, sizeof(g_nnz), who)) != SPMV_OK) break;
            if (g_nnz < n || (int64_t)g_nnz > src->nnz)
            {
                set_error("%s: the pattern came to %d entries of %lld for %d rows", who, g_nnz, (long long)src->nnz, n);
                rc = SPMV_ERR_HIP;
                break;
            }
            st        = new fsai_state();
            st->level = lvl;
            st->nnz   = g_nnz;
            st->max_row = h[kFlagMax];
            if ((rc = mat_alloc(ctx, SPMV_FMT_CSR, n, n, g_nnz, 0, (size_t)n + 1, (size_t)g_nnz, (size_t)g_nnz, &st->G)) != SPMV_OK) break;
            spmv_mat* G = st->G;
            if ((rc = hip_step(hipMemcpyAsync(const_cast<int32_t*>(G->a), g_rp, sizeof(int32_t) * ((size_t)n + 1), hipMemcpyDeviceToDevice, s), who,
                               "copying the row offsets")) != SPMV_OK)
                break;
            hipLaunchKernelGGL(fsai_lower_fill_kernel, dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0, s, n, src->a, (const int32_t*)key, G->a,
                               const_cast<int32_t*>(G->b));
            if ((rc = hip_step(hipGetLastError(), who, "the columns' launch")) != SPMV_OK) break;
            // the rows by lane class, ascending inside a class
            if ((rc = sort_ids_by_key(ctx, cls, n, key_bits(kFsaiClasses), ids)) != SPMV_OK) break;
            if ((rc = hip_step(hipStreamSynchronize(s), who, "waiting for the pattern")) != SPMV_OK) break;
            us_pattern = us_since(t_begin);
            int64_t first = 0;
            for (int c = 0; c < kFsaiClasses; ++c)
            {
                const int64_t rows = h[kFlagClass + c];
                if (rows > 0)
                {
                    int* const bad = flags + kFlagPivot;
                    switch (c)
                    {
                        case 0: launch_rows<4>(s, rows, ids + first, m, G, bad); break;
                        case 1: launch_rows<8>(s, rows, ids + first, m, G, bad); break;
                        case 2: launch_rows<16>(s, rows, ids + first, m, G, bad); break;
                        case 3: launch_rows<32>(s, rows, ids + first, m, G, bad); break;
                        default: launch_rows<64>(s, rows, ids + first, m, G, bad); break;
                    }
                }
                first += rows;
            }
            if (first != n)
            {
                set_error("%s: the lane classes hold %lld rows of %d", who, (long long)first, n);
                rc = SPMV_ERR_HIP;
                break;
            }
            if ((rc = hip_step(hipGetLastError(), who, "a launch of the row kernel")) != SPMV_OK) break;
            int h_bad = INT_MAX;
            if ((rc = read_scalars(ctx, &h_bad, flags + kFlagPivot, sizeof(h_bad), who)) != SPMV_OK) break;
            us_rows = us_since(t_begin) - us_pattern;
            if (h_bad != INT_MAX)
            {
                set_error("%s: a pivot of row %d is not positive or not finite: its local matrix is not positive definite", who, h_bad);
                rc = SPMV_ERR_INVALID;
                break;
            }
        } while (0);
    }  // (the pool waits for the stream and frees)
    if (P) mat_free(P);
    if (rc == SPMV_OK)
    {
        // the two handles: G like any uploaded CSR handle, G^T by the engine's transpose; "panel_trial" of A holds for both
        st->G->pb_trial = m->pb_trial;
        rc              = csr_analyse(st->G);
        if (rc == SPMV_OK) rc = csr_transpose(ctx, st->G, &st->Gt);
        if (rc == SPMV_OK && hipMalloc(&st->w, sizeof(double) * (size_t)n) != hipSuccess)
        {
            (void)hipGetLastError();
            set_error("%s: out of device memory for the work vector of %d entries", who, n);
            rc = SPMV_ERR_ALLOC;
        }
    }
    if (rc != SPMV_OK)
    {
        state_free(st);
        if (!keep_old) fsai_free(m);
        return rc;
    }
    st->us_pattern = us_pattern;
    st->us_rows    = us_rows;
    st->us_handles = us_since(t_begin) - us_pattern - us_rows;
    st->bytes      = st->G->device_bytes + st->Gt->device_bytes + (int64_t)sizeof(double) * n;
    fsai_free(m);
    m->fsai = st;
    return SPMV_OK;
}

// z = G^T (G r); r and z must not overlap
int fsai_apply(spmv_ctx* ctx, const spmv_mat* A, const double* r, double* z)
{
    const fsai_state* st = A->fsai;
    if (!st) SPMV_FAIL(SPMV_ERR_INVALID, "spmv_fsai_solve: the handle was not set up (spmv_fsai_setup)");
    if (A->nrow == 0) return SPMV_OK;
    if (!st->G || !st->Gt || !st->w || !r || !z) SPMV_FAIL(SPMV_ERR_INVALID, "spmv_fsai_solve: the factor of this handle is incomplete");
    apply_extra over;
    over.overwrite = true;
    SPMV_TRY(mat_apply_ex(ctx, st->G, r, st->w, over));
    return mat_apply_ex(ctx, st->Gt, st->w, z, over);
}

int fsai_info(const spmv_mat* m, int32_t* level, int64_t* nnz, int32_t* max_row)
{
    const fsai_state* st = m->fsai;
    if (!st) SPMV_FAIL(SPMV_ERR_INVALID, "spmv_fsai_info: the handle was not set up (spmv_fsai_setup)");
    if (level) *level = st->level;
    if (nnz) *nnz = st->nnz;
    if (max_row) *max_row = st->max_row;
    return SPMV_OK;
}

// G as host CSR; null arrays: the size alone
int fsai_factor_download(spmv_ctx* ctx, const spmv_mat* m, int64_t* nnz, int32_t* row_ptr, int32_t* col, double* val)
{
    const char* const who = "spmv_fsai_factor";
    const fsai_state* st  = m->fsai;
    if (!st) SPMV_FAIL(SPMV_ERR_INVALID, "%s: the handle was not set up (spmv_fsai_setup)", who);
    *nnz = st->nnz;
    if (!st->G)  // (no rows)
    {
        if (row_ptr) row_ptr[0] = 0;
        return SPMV_OK;
    }
    hipStream_t s = ctx->stream;
    hipError_t  e = hipSuccess;
    if (row_ptr) e = hipMemcpyAsync(row_ptr, st->G->a, sizeof(int32_t) * ((size_t)m->nrow + 1), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && col && st->nnz) e = hipMemcpyAsync(col, st->G->b, sizeof(int32_t) * (size_t)st->nnz, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && val && st->nnz) e = hipMemcpyAsync(val, st->G->v, sizeof(double) * (size_t)st->nnz, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return hip_step(e, who, "downloading the factor");
}

bool fsai_get_param(const spmv_mat* m, const char* name, int64_t* value)
{
    const fsai_state* st = m->fsai;
    if (!strcmp(name, "fsai_level"))
        *value = m->fsai_level;
    else if (!strcmp(name, "fsai_ready"))
        *value = st ? 1 : 0;
    else if (!strcmp(name, "fsai_bytes"))
        *value = st ? st->bytes : 0;
    else if (!strcmp(name, "fsai_max_row"))
        *value = st ? st->max_row : 0;
    else if (!strcmp(name, "fsai_setup_us_pattern"))  // the last set-up's wall time: the products, the cut, the scan, the columns, the classes
        *value = st ? st->us_pattern : 0;
    else if (!strcmp(name, "fsai_setup_us_rows"))  // the row kernel's launches
        *value = st ? st->us_rows : 0;
    else if (!strcmp(name, "fsai_setup_us_handles"))  // the analysis of G, the transpose and its analysis
        *value = st ? st->us_handles : 0;
    else
        return false;
    return true;
}

bool fsai_set_param(spmv_mat* m, const char* name, int64_t value, int* rc)
{
    if (strcmp(name, "fsai_level")) return false;
    if (value < 1 || value > 3)
    {
        set_error("fsai_level: 1 .. 3, got %lld", (long long)value);
        *rc = SPMV_ERR_INVALID;
        return true;
    }
    m->fsai_level = (int32_t)value;
    *rc           = SPMV_OK;
    return true;
}
}  // namespace spmv
