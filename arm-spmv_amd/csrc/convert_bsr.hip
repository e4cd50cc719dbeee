// convert_bsr.hip - block CSR set-up on the device: CSR -> BSR, BSR -> CSR and the transposed BSR handle.  Integer work and copies
// off the hot path; set-up memory comes from a device_pool (sorted_runs.hpp) and is gone when the call returns.  tests/bsr_ref.py
// is the NumPy twin of the orders defined here.
//
// csr_to_bsr.  Entry e of row i, column j gets the key (i / bs, j / bs); runs_by_key_pair (sorted_runs.hip) orders the entry ids
// stably by that pair and cuts the runs of equal keys: a run IS a block, the runs come out by block row with block columns
// ascending, so run s is block s and the scan of the runs per block row is the block row pointer.  One lane per block clears its
// bs^2 values and adds its entries in that order - the stored order - with plain additions from 0.0: a position's value is the
// sum of the entries that fall on it (a single entry v comes through as 0.0 + v), a position without an entry is 0.0.
//
// bsr_to_csr.  One lane per scalar row walks its block row's blocks - in stable block-column order, through a sorted id list
// where the handle's block columns do not ascend already - and counts, then writes, the positions inside nrow x ncol (with
// drop_zeros: those whose value is not equal to 0.0); a scan of the counts in between is the row pointer.
//
// bsr_transpose.  Block ids ordered stably by block column (sort_ids_by_key, convert_sort.hip): the k-th of them is block k of
// A^T, its block column the block row it came from, its values the block's transposed as they are copied (bs^2 lanes per block).
#include "bsr_settings.hpp"
#include "common.hpp"
#include "solver_host.hpp"
#include "sorted_runs.hpp"

namespace spmv
{
namespace
{
// owner[e] = the row r with ptr[r] <= e < ptr[r + 1], e < total (ptr has n + 1 entries, ptr[n] = total)
__global__ __launch_bounds__(kBlock) void owner_of_entry_kernel(int64_t total, int32_t n, const int32_t* __restrict__ ptr, int32_t* __restrict__ owner)
{
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock)
    {
        int32_t lo = 0, hi = n;  // the answer lies in [lo, hi)
        while (hi - lo > 1)
        {
            const int32_t mid = lo + (hi - lo) / 2;
            if (ptr[mid] <= e)
                lo = mid;
            else
                hi = mid;
        }
        owner[e] = lo;
    }
}

__global__ __launch_bounds__(kBlock) void block_keys_kernel(int64_t nnz, int32_t bs, const int32_t* __restrict__ row, const int32_t* __restrict__ col,
                                                           int32_t* __restrict__ key_i, int32_t* __restrict__ key_j)
{
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * kBlock)
    {
        key_i[e] = row[e] / bs;
        key_j[e] = col[e] / bs;
    }
}

// one lane per block (run) s: its column, and its values from 0.0 in stored order
__global__ __launch_bounds__(kBlock) void block_fill_kernel(int64_t nnzb, int32_t bs, const int32_t* __restrict__ seg_start, const int32_t* __restrict__ order,
                                                           const int32_t* __restrict__ run_j, const int32_t* __restrict__ row, const int32_t* __restrict__ col,
                                                           const double* __restrict__ val, int32_t* __restrict__ bcol, double* __restrict__ bval)
{
    const int bs2 = bs * bs;
    for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < nnzb; s += (int64_t)gridDim.x * kBlock)
    {
        double* blk = bval + s * bs2;
        for (int p = 0; p < bs2; ++p) blk[p] = 0.0;
        const int end = seg_start[s + 1];
        for (int k = seg_start[s]; k < end; ++k)
        {
            const int32_t e = order[k];
            const int     p = (row[e] % bs) * bs + col[e] % bs;
            blk[p]          = __dadd_rn(blk[p], val[e]);
        }
        bcol[s] = run_j[s];
    }
}

// flag = 1 where a block row's block columns do not ascend strictly
__global__ __launch_bounds__(kBlock) void block_order_check_kernel(int64_t nnzb, const int32_t* __restrict__ brow, const int32_t* __restrict__ bcol,
                                                                  int32_t* __restrict__ flag)
{
    bool bad = false;
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x + 1; k < nnzb; k += (int64_t)gridDim.x * kBlock)
        bad |= brow[k] == brow[k - 1] && bcol[k] <= bcol[k - 1];
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

__global__ __launch_bounds__(kBlock) void gather_i32_kernel(int64_t n, const int32_t* __restrict__ src, const int32_t* __restrict__ idx, int32_t* __restrict__ out)
{
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += (int64_t)gridDim.x * kBlock) out[k] = src[idx[k]];
}

// one lane per scalar row i: WRITE false: count[i] = its positions (count[nrow] = 0); true: columns and values at row_ptr[i]
template <bool WRITE>
__global__ __launch_bounds__(kBlock) void bsr_rows_kernel(int32_t nrow, int32_t ncol, int32_t bs, int32_t drop_zeros, const int32_t* __restrict__ brow_ptr,
                                                         const int32_t* __restrict__ order, const int32_t* __restrict__ bcol, const double* __restrict__ bval,
                                                         int32_t* __restrict__ count, const int32_t* __restrict__ row_ptr, int32_t* __restrict__ col,
                                                         double* __restrict__ val)
{
    const int bs2 = bs * bs;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i <= nrow; i += (int64_t)gridDim.x * kBlock)
    {
        if (i == nrow)
        {
            if (!WRITE) count[i] = 0;
            continue;
        }
        const int br = (int)(i / bs), r = (int)(i % bs);
        int64_t   at  = WRITE ? row_ptr[i] : 0;
        int32_t   n   = 0;
        const int end = brow_ptr[br + 1];
        for (int k = brow_ptr[br]; k < end; ++k)
        {
            const int64_t b  = order ? order[k] : k;
            const int64_t j0 = (int64_t)bcol[b] * bs;
            for (int c = 0; c < bs; ++c)
            {
                if (j0 + c >= ncol) break;
                const double v = bval[b * bs2 + r * bs + c];
                if (drop_zeros && v == 0.0) continue;
                if (WRITE)
                {
                    col[at] = (int32_t)(j0 + c);
                    val[at] = v;
                    ++at;
                }
                ++n;
            }
        }
        if (!WRITE) count[i] = n;
    }
}

__global__ __launch_bounds__(kBlock) void histogram_kernel(int64_t n, const int32_t* __restrict__ key, int32_t* __restrict__ count)
{
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += (int64_t)gridDim.x * kBlock) atomicAdd(count + key[k], 1);  // (an integer sum)
}

// bs^2 lanes per block k of A^T: out[k][c][r] = in[order[k]][r][c], and the block's column = the block row it came from
__global__ __launch_bounds__(kBlock) void block_transpose_kernel(int64_t nnzb, int32_t bs, const int32_t* __restrict__ order, const int32_t* __restrict__ brow,
                                                                const double* __restrict__ in, int32_t* __restrict__ out_col, double* __restrict__ out)
{
    const int     bs2   = bs * bs;
    const int64_t total = nnzb * bs2;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kBlock)
    {
        const int64_t k = t / bs2;
        const int     p = (int)(t % bs2), r = p / bs, c = p % bs;  // position (r, c) of the OUTPUT block
        const int64_t b = order[k];
        out[t]          = in[b * bs2 + c * bs + r];
        if (p == 0) out_col[k] = brow[b];
    }
}

// the ids of a BSR handle's blocks in stable (block row, block column) order, or null where they are in that order already
int blocks_in_column_order(spmv_ctx* ctx, device_pool& pool, const char* who, const spmv_mat* A, int64_t nnzb, int32_t mb, int32_t nbc, const int32_t* brow,
                           int32_t** order)
{
    *order        = nullptr;
    hipStream_t s = ctx->stream;
    SPMV_TRY(ensure_scratch(ctx, 64));
    int32_t* flag = (int32_t*)ctx->scratch;
    int32_t  h    = 0;
    SPMV_TRY(hip_step(hipMemsetAsync(flag, 0, sizeof(int32_t), s), who, "clearing the order flag"));
    hipLaunchKernelGGL(block_order_check_kernel, dim3(stream_grid(nnzb)), dim3(kBlock), 0, s, nnzb, brow, A->b, flag);
    SPMV_TRY(hip_step(hipGetLastError(), who, "the order check's launch"));
    SPMV_TRY(read_scalars(ctx, &h, flag, sizeof(h), who));
    if (!h) return SPMV_OK;
    int32_t *ids1, *brow1, *ids2, *ord;
    SPMV_TRY(pool.get(ids1, (size_t)nnzb));
    SPMV_TRY(pool.get(brow1, (size_t)nnzb));
    SPMV_TRY(pool.get(ids2, (size_t)nnzb));
    SPMV_TRY(pool.get(ord, (size_t)nnzb));
    SPMV_TRY(sort_ids_by_key(ctx, A->b, nnzb, key_bits(nbc), ids1));
    hipLaunchKernelGGL(gather_i32_kernel, dim3(stream_grid(nnzb)), dim3(kBlock), 0, s, nnzb, brow, (const int32_t*)ids1, brow1);
    SPMV_TRY(sort_ids_by_key(ctx, brow1, nnzb, key_bits(mb), ids2));
    hipLaunchKernelGGL(gather_i32_kernel, dim3(stream_grid(nnzb)), dim3(kBlock), 0, s, nnzb, (const int32_t*)ids1, (const int32_t*)ids2, ord);
    SPMV_TRY(hip_step(hipGetLastError(), who, "the block order's launches"));
    *order = ord;
    return SPMV_OK;
}
}  // namespace

// ---- the refusals, on the host ---------------------------------------------------------------------------------------------------
int bsr_check_bs(int32_t bs, const char* who)
{
    if (!bsr_bs_valid(bs)) SPMV_FAIL(SPMV_ERR_UNSUPPORTED, "%s: square blocks of 2 .. 8, got bs = %d", who, bs);
    return SPMV_OK;
}

int csr_to_bsr_check(const spmv_ctx* ctx, const spmv_mat* csr, int32_t bs, const char* who)
{
    if (csr->format != SPMV_FMT_CSR) SPMV_FAIL(SPMV_ERR_UNSUPPORTED, "%s: the input must be a CSR handle (format %d)", who, csr->format);
    SPMV_TRY(bsr_check_bs(bs, who));
    SPMV_REQUIRE(csr->ctx == ctx, "%s: the matrix belongs to another context", who);
    SPMV_REQUIRE(csr->row_begin == 0, "%s: the matrix is a row shard (it starts at row %lld)", who, (long long)csr->row_begin);
    SPMV_REQUIRE(csr->a && (csr->nnz == 0 || (csr->b && csr->v)), "%s: the handle's CSR arrays are gone (panel_keep_csr = 0)", who);
    return SPMV_OK;
}

int bsr_to_csr_check(const spmv_ctx* ctx, const spmv_mat* bsr, const char* who)
{
    if (bsr->format != SPMV_FMT_BSR) SPMV_FAIL(SPMV_ERR_UNSUPPORTED, "%s: the input must be a BSR handle (format %d)", who, bsr->format);
    SPMV_REQUIRE(bsr->ctx == ctx, "%s: the matrix belongs to another context", who);
    if (bsr->nnz > (int64_t)INT32_MAX - 65536)
        SPMV_FAIL(SPMV_ERR_UNSUPPORTED, "%s: %lld stored values do not fit a CSR handle's int32 offsets", who, (long long)bsr->nnz);
    return SPMV_OK;
}

// ---- CSR -> BSR --------------------------------------------------------------------------------------------------------------------
int csr_to_bsr(spmv_ctx* ctx, const spmv_mat* csr, int32_t bs, spmv_mat** out)
{
    const char*   who = "spmv_csr_to_bsr";
    hipStream_t   s   = ctx->stream;
    const int64_t nnz = csr->nnz;
    const int32_t mb = (int32_t)ceil_div(csr->nrow, bs), nbc = (int32_t)ceil_div(csr->ncol, bs), bs2 = bs * bs;
    spmv_mat*     B  = nullptr;
    if (nnz == 0 || mb == 0)
    {
        SPMV_TRY(mat_alloc(ctx, SPMV_FMT_BSR, csr->nrow, csr->ncol, 0, bs, (size_t)mb + 1, 0, 0, &B));
        const int rc = hip_step(hipMemsetAsync(const_cast<int32_t*>(B->a), 0, sizeof(int32_t) * ((size_t)mb + 1), s), who, "clearing the block row pointer");
        if (rc != SPMV_OK) mat_free(B);
        else *out = B;
        return rc;
    }
    device_pool pool(ctx, who);
    int32_t *   row, *key_i, *key_j;
    SPMV_TRY(pool.get(row, (size_t)nnz));
    SPMV_TRY(pool.get(key_i, (size_t)nnz));
    SPMV_TRY(pool.get(key_j, (size_t)nnz));
    hipLaunchKernelGGL(owner_of_entry_kernel, dim3(stream_grid(nnz)), dim3(kBlock), 0, s, nnz, csr->nrow, csr->a, row);
    hipLaunchKernelGGL(block_keys_kernel, dim3(stream_grid(nnz)), dim3(kBlock), 0, s, nnz, bs, (const int32_t*)row, csr->b, key_i, key_j);
    SPMV_TRY(hip_step(hipGetLastError(), who, "the block keys' launches"));
    key_runs kr;
    SPMV_TRY(runs_by_key_pair(ctx, pool, who, key_i, mb, key_j, nbc, nnz, &kr));
    const int64_t nnzb = kr.runs;
    SPMV_TRY(mat_alloc(ctx, SPMV_FMT_BSR, csr->nrow, csr->ncol, nnzb * bs2, bs, (size_t)mb + 1, (size_t)nnzb, (size_t)(nnzb * bs2), &B));
    int rc = exclusive_scan_i32(ctx, kr.count_i, const_cast<int32_t*>(B->a), (int64_t)mb + 1);
    if (rc == SPMV_OK)
    {
        hipLaunchKernelGGL(block_fill_kernel, dim3(stream_grid(nnzb)), dim3(kBlock), 0, s, nnzb, bs, (const int32_t*)kr.seg_start, (const int32_t*)kr.order,
                           (const int32_t*)kr.run_j, (const int32_t*)row, csr->b, csr->v, const_cast<int32_t*>(B->b), const_cast<double*>(B->v));
        rc = hip_step(hipGetLastError(), who, "the block fill's launch");
    }
    if (rc == SPMV_OK) rc = hip_step(hipStreamSynchronize(s), who, "the set-up's kernels");
    if (rc != SPMV_OK)
    {
        mat_free(B);
        return rc;
    }
    *out = B;
    return SPMV_OK;
}

// ---- BSR -> CSR --------------------------------------------------------------------------------------------------------------------
int bsr_to_csr(spmv_ctx* ctx, const spmv_mat* bsr, int32_t drop_zeros, spmv_mat** out)
{
    const char*   who = "spmv_bsr_to_csr";
    hipStream_t   s   = ctx->stream;
    const int32_t bs = bsr->k, nrow = bsr->nrow, ncol = bsr->ncol;
    const int32_t mb = (int32_t)ceil_div(nrow, bs), nbc = (int32_t)ceil_div(ncol, bs);
    const int64_t nnzb = bsr->nnz / (bs * bs);
    device_pool   pool(ctx, who);
    int32_t *     order = nullptr, *count;
    if (nnzb > 1)
    {
        int32_t* brow;
        SPMV_TRY(pool.get(brow, (size_t)nnzb));
        hipLaunchKernelGGL(owner_of_entry_kernel, dim3(stream_grid(nnzb)), dim3(kBlock), 0, s, nnzb, mb, bsr->a, brow);
        SPMV_TRY(hip_step(hipGetLastError(), who, "the block rows' launch"));
        SPMV_TRY(blocks_in_column_order(ctx, pool, who, bsr, nnzb, mb, nbc, brow, &order));
    }
    SPMV_TRY(pool.get(count, (size_t)nrow + 1));
    const int grid = stream_grid((int64_t)nrow + 1);
    hipLaunchKernelGGL(bsr_rows_kernel<false>, dim3(grid), dim3(kBlock), 0, s, nrow, ncol, bs, drop_zeros, bsr->a, (const int32_t*)order, bsr->b, bsr->v, count,
                       (const int32_t*)nullptr, (int32_t*)nullptr, (double*)nullptr);
    SPMV_TRY(hip_step(hipGetLastError(), who, "the count's launch"));
    SPMV_TRY(exclusive_scan_i32(ctx, count, count, (int64_t)nrow + 1));
    int32_t nnz = 0;
    SPMV_TRY(read_scalars(ctx, &nnz, count + nrow, sizeof(nnz), who));
    SPMV_REQUIRE(nnz >= 0 && nnz <= bsr->nnz, "%s: %d positions from %lld stored values", who, nnz, (long long)bsr->nnz);
    spmv_mat* C = nullptr;
    SPMV_TRY(mat_alloc(ctx, SPMV_FMT_CSR, nrow, ncol, nnz, 0, (size_t)nrow + 1, (size_t)nnz, (size_t)nnz, &C));
    int rc = hip_step(hipMemcpyAsync(const_cast<int32_t*>(C->a), count, sizeof(int32_t) * ((size_t)nrow + 1), hipMemcpyDeviceToDevice, s), who, "copying the row pointer");
    if (rc == SPMV_OK && nnz > 0)
    {
        hipLaunchKernelGGL(bsr_rows_kernel<true>, dim3(grid), dim3(kBlock), 0, s, nrow, ncol, bs, drop_zeros, bsr->a, (const int32_t*)order, bsr->b, bsr->v,
                           (int32_t*)nullptr, (const int32_t*)count, const_cast<int32_t*>(C->b), const_cast<double*>(C->v));
        rc = hip_step(hipGetLastError(), who, "the fill's launch");
    }
    if (rc == SPMV_OK) rc = hip_step(hipStreamSynchronize(s), who, "the set-up's kernels");
    if (rc != SPMV_OK)
    {
        mat_free(C);
        return rc;
    }
    *out = C;
    return SPMV_OK;
}

// ---- the BSR handle of A^T (transpose.hip: the companion of a BSR handle); owns its arrays, analysed like an uploaded one -------------
int bsr_transpose(spmv_ctx* ctx, const spmv_mat* A, spmv_mat** out)
{
    const char*   who = "spmv_mat_transpose_setup";
    hipStream_t   s   = ctx->stream;
    const int32_t bs = A->k, bs2 = bs * bs;
    const int32_t mb = (int32_t)ceil_div(A->nrow, bs), nbc = (int32_t)ceil_div(A->ncol, bs);
    const int64_t nnzb = A->nnz / bs2;
    spmv_mat*     T    = nullptr;
    SPMV_TRY(mat_alloc(ctx, SPMV_FMT_BSR, A->ncol, A->nrow, A->nnz, bs, (size_t)nbc + 1, (size_t)nnzb, (size_t)A->nnz, &T));
    int rc = SPMV_OK;
    {
        device_pool pool(ctx, who);
        int32_t *   brow = nullptr, *order = nullptr, *count = nullptr;
        rc = pool.get(count, (size_t)nbc + 1);
        if (rc == SPMV_OK) rc = hip_step(hipMemsetAsync(count, 0, sizeof(int32_t) * ((size_t)nbc + 1), s), who, "clearing the column counts");
        if (rc == SPMV_OK && nnzb > 0)
        {
            rc = pool.get(brow, (size_t)nnzb);
            if (rc == SPMV_OK) rc = pool.get(order, (size_t)nnzb);
            if (rc == SPMV_OK)
            {
                hipLaunchKernelGGL(owner_of_entry_kernel, dim3(stream_grid(nnzb)), dim3(kBlock), 0, s, nnzb, mb, A->a, brow);
                hipLaunchKernelGGL(histogram_kernel, dim3(stream_grid(nnzb)), dim3(kBlock), 0, s, nnzb, A->b, count);
                rc = hip_step(hipGetLastError(), who, "the column counts' launches");
            }
            if (rc == SPMV_OK) rc = sort_ids_by_key(ctx, A->b, nnzb, key_bits(nbc), order);
        }
        if (rc == SPMV_OK) rc = exclusive_scan_i32(ctx, count, const_cast<int32_t*>(T->a), (int64_t)nbc + 1);
        if (rc == SPMV_OK && nnzb > 0)
        {
            hipLaunchKernelGGL(block_transpose_kernel, dim3(stream_grid(A->nnz)), dim3(kBlock), 0, s, nnzb, bs, (const int32_t*)order, (const int32_t*)brow, A->v,
                               const_cast<int32_t*>(T->b), const_cast<double*>(T->v));
            rc = hip_step(hipGetLastError(), who, "the block transpose's launch");
        }
        if (rc == SPMV_OK) rc = hip_step(hipStreamSynchronize(s), who, "the set-up's kernels");
    }
    if (rc == SPMV_OK) rc = bsr_analyse(T);
    if (rc != SPMV_OK)
    {
        mat_free(T);
        return rc;
    }
    *out = T;
    return SPMV_OK;
}
}  // namespace spmv
