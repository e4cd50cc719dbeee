// convert_f32.hip - set-up of CSR handles with single-precision value storage (SPMV_FMT_CSR_F32), on the device: CSR -> format 6,
// host arrays -> format 6, format 6 -> CSR, and the format-6 handle of A^T.  Copies off the hot path; set-up memory comes from a
// device_pool (sorted_runs.hpp) and is gone when the call returns.  tests/csr_f32_ref.py is the NumPy twin of the rounding and of
// the statistics defined in csr_f32_settings.hpp.
//
// f32_pack_kernel.  One lane per entry, grid-stride: the value is classified and rounded (f32_classify), the word is packed and
// stored, and the pass gathers in the same sweep the values that changed, the nonzero values that became zero or subnormal, the
// largest relative change among the changed ones that did not underflow, the values that cannot be stored (not finite, or rounding
// to +-inf) and the first row that holds one of those.  The counts are integer atomics, the largest change a maximum over the bits
// of non-negative doubles (which order as the doubles do) and the first row a minimum: the same bits after every call.  A value
// that cannot be stored ends the conversion on the host; the word written for it (0.0f) is never multiplied.
#include "common.hpp"
#include "csr_f32_settings.hpp"
#include "solver_host.hpp"
#include "sorted_runs.hpp"

namespace spmv
{
namespace
{
struct f32_stats  // on the device: the context's scratch; every field an integer for the atomics
{
    unsigned long long inexact, underflow, max_rel_bits, overflow, first_row;
};

template <typename T>
__global__ __launch_bounds__(kBlock) void f32_pack_kernel(int64_t nnz, int32_t nrow, const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                         const T* __restrict__ val, uint64_t* __restrict__ ent, f32_stats* __restrict__ st)
{
    unsigned           inexact = 0, underflow = 0, overflow = 0;
    unsigned long long worst = 0, first = ~0ull;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * kBlock)
    {
        const double    v = (double)val[e];
        float           f;
        const f32_class c = f32_classify(v, &f);
        ent[e]            = f32_pack(col[e], f);
        if (c == kF32Overflow)
        {
            ++overflow;
            int32_t lo = 0, hi = nrow;  // the row r with row_ptr[r] <= e < row_ptr[r + 1] lies in [lo, hi)
            while (hi - lo > 1)
            {
                const int32_t mid = lo + (hi - lo) / 2;
                if (row_ptr[mid] <= e)
                    lo = mid;
                else
                    hi = mid;
            }
            first = min(first, (unsigned long long)lo);
            continue;
        }
        if (f32_changed(v, f)) ++inexact;
        if (c == kF32Underflow) ++underflow;
        if (c == kF32Inexact) worst = max(worst, (unsigned long long)__double_as_longlong(f32_rel_change(v, f)));
    }
    for (int off = 32; off > 0; off >>= 1)
    {
        inexact += __shfl_xor(inexact, off);
        underflow += __shfl_xor(underflow, off);
        overflow += __shfl_xor(overflow, off);
        worst = max(worst, (unsigned long long)__shfl_xor(worst, off));
        first = min(first, (unsigned long long)__shfl_xor(first, off));
    }
    if ((threadIdx.x & 63) == 0)
    {
        if (inexact) atomicAdd(&st->inexact, (unsigned long long)inexact);
        if (underflow) atomicAdd(&st->underflow, (unsigned long long)underflow);
        if (worst) atomicMax(&st->max_rel_bits, worst);
        if (overflow)
        {
            atomicAdd(&st->overflow, (unsigned long long)overflow);
            atomicMin(&st->first_row, first);
        }
    }
}

__global__ __launch_bounds__(kBlock) void f32_widen_kernel(int64_t nnz, const uint64_t* __restrict__ ent, int32_t* __restrict__ col, double* __restrict__ val)
{
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * kBlock)
    {
        const uint64_t w = ent[e];
        if (col) col[e] = f32_entry_col(w);
        if (val) val[e] = (double)f32_entry_value(w);
    }
}

// a format-6 handle with its row pointer and stream allocated (the stream holds at least one word: kernels never see nullptr)
int f32_alloc(spmv_ctx* ctx, int32_t nrow, int32_t ncol, int64_t nnz, const char* who, spmv_mat** out)
{
    spmv_mat* m = nullptr;
    SPMV_TRY(mat_alloc(ctx, SPMV_FMT_CSR_F32, nrow, ncol, nnz, 0, (size_t)nrow + 1, 0, 0, &m));
    if (hipMalloc((void**)&m->f32_ent, sizeof(uint64_t) * (size_t)std::max<int64_t>(nnz, 1)) != hipSuccess)
    {
        (void)hipGetLastError();
        mat_free(m);
        SPMV_FAIL(SPMV_ERR_ALLOC, "%s: out of device memory for a stream of %lld packed entries", who, (long long)nnz);
    }
    m->device_bytes += (int64_t)sizeof(uint64_t) * nnz;
    *out = m;
    return SPMV_OK;
}

// packs `nnz` entries of (col, val) under row_ptr (all on the device) into m's stream; synchronous; fills *h
template <typename T>
int f32_pack_into(spmv_ctx* ctx, spmv_mat* m, const int32_t* row_ptr, const int32_t* col, const T* val, const char* who, f32_stats* h)
{
    hipStream_t s = ctx->stream;
    SPMV_TRY(ensure_scratch(ctx, sizeof(f32_stats)));
    f32_stats* d = (f32_stats*)ctx->scratch;
    *h           = f32_stats{0, 0, 0, 0, ~0ull};
    SPMV_TRY(hip_step(hipMemcpyAsync(d, h, sizeof(*h), hipMemcpyHostToDevice, s), who, "clearing the statistics"));
    if (m->nnz > 0)
    {
        hipLaunchKernelGGL((f32_pack_kernel<T>), dim3(stream_grid(m->nnz)), dim3(kBlock), 0, s, m->nnz, m->nrow, row_ptr, col, val, m->f32_ent, d);
        SPMV_TRY(hip_step(hipGetLastError(), who, "the packing pass's launch"));
    }
    SPMV_TRY(read_scalars(ctx, h, d, sizeof(*h), who));
    if (h->overflow)
        SPMV_FAIL(SPMV_ERR_INVALID, "%s: %llu values are not finite or round to +-inf in single precision (the first in row %llu)", who, h->overflow, h->first_row);
    return SPMV_OK;
}
}  // namespace

// ---- the refusals, on the host ---------------------------------------------------------------------------------------------------
int csr_to_f32_check(const spmv_ctx* ctx, const spmv_mat* csr, const char* who)
{
    if (csr->format != SPMV_FMT_CSR) SPMV_FAIL(SPMV_ERR_UNSUPPORTED, "%s: the input must be a CSR handle (format %d)", who, csr->format);
    SPMV_REQUIRE(csr->ctx == ctx, "%s: the matrix belongs to another context", who);
    SPMV_REQUIRE(csr->row_begin == 0, "%s: the matrix is a row shard (it starts at row %lld)", who, (long long)csr->row_begin);
    SPMV_REQUIRE(csr->a && (csr->nnz == 0 || (csr->b && csr->v)), "%s: the handle's CSR arrays are gone (panel_keep_csr = 0)", who);
    return SPMV_OK;
}

int f32_to_csr_check(const spmv_ctx* ctx, const spmv_mat* f32, const char* who)
{
    if (f32->format != SPMV_FMT_CSR_F32) SPMV_FAIL(SPMV_ERR_UNSUPPORTED, "%s: the input must be a handle of format 6 (format %d)", who, f32->format);
    SPMV_REQUIRE(f32->ctx == ctx, "%s: the matrix belongs to another context", who);
    return SPMV_OK;
}

// ---- CSR -> format 6; synchronous, analysed by the caller ----------------------------------------------------------------------------
int csr_to_f32(spmv_ctx* ctx, const spmv_mat* csr, const char* who, spmv_mat** out)
{
    spmv_mat* m = nullptr;
    SPMV_TRY(f32_alloc(ctx, csr->nrow, csr->ncol, csr->nnz, who, &m));
    f32_stats h;
    int       rc = hip_step(hipMemcpyAsync(const_cast<int32_t*>(m->a), csr->a, sizeof(int32_t) * ((size_t)csr->nrow + 1), hipMemcpyDeviceToDevice, ctx->stream), who,
                            "copying the row pointer");
    if (rc == SPMV_OK) rc = f32_pack_into(ctx, m, csr->a, csr->b, csr->v, who, &h);
    if (rc != SPMV_OK)
    {
        (void)hipStreamSynchronize(ctx->stream);
        mat_free(m);
        return rc;
    }
    m->f32_inexact   = (int64_t)h.inexact;
    m->f32_underflow = (int64_t)h.underflow;
    m->f32_max_rel   = __builtin_bit_cast(double, h.max_rel_bits);
    *out             = m;
    return SPMV_OK;
}

// ---- host arrays -> format 6; synchronous, analysed by the caller (the statistics of an uploaded handle are zero) ---------------------
int csr_f32_from_host(spmv_ctx* ctx, int32_t nrow, int32_t ncol, int64_t nnz, const int32_t* row_ptr, const int32_t* col, const float* val, spmv_mat** out)
{
    const char* who = "spmv_csr_f32_upload";
    spmv_mat*   m   = nullptr;
    SPMV_TRY(f32_alloc(ctx, nrow, ncol, nnz, who, &m));
    int rc = SPMV_OK;
    {
        device_pool pool(ctx, who);
        int32_t*    d_col = nullptr;
        float*      d_val = nullptr;
        f32_stats   h;
        rc = pool.get(d_col, (size_t)nnz);
        if (rc == SPMV_OK) rc = pool.get(d_val, (size_t)nnz);
        if (rc == SPMV_OK) rc = hip_step(hipMemcpyAsync(const_cast<int32_t*>(m->a), row_ptr, sizeof(int32_t) * ((size_t)nrow + 1), hipMemcpyHostToDevice, ctx->stream), who, "uploading the row pointer");
        if (rc == SPMV_OK && nnz > 0) rc = hip_step(hipMemcpyAsync(d_col, col, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, ctx->stream), who, "uploading the columns");
        if (rc == SPMV_OK && nnz > 0) rc = hip_step(hipMemcpyAsync(d_val, val, sizeof(float) * (size_t)nnz, hipMemcpyHostToDevice, ctx->stream), who, "uploading the values");
        if (rc == SPMV_OK) rc = hip_step(hipStreamSynchronize(ctx->stream), who, "the uploads");  // pageable host memory: the caller may free it on return
        if (rc == SPMV_OK) rc = f32_pack_into(ctx, m, m->a, (const int32_t*)d_col, (const float*)d_val, who, &h);
    }
    if (rc != SPMV_OK)
    {
        mat_free(m);
        return rc;
    }
    *out = m;
    return SPMV_OK;
}

// ---- format 6 -> CSR (exact); synchronous, analysed by the caller --------------------------------------------------------------------
int f32_to_csr(spmv_ctx* ctx, const spmv_mat* f32, const char* who, spmv_mat** out)
{
    spmv_mat* C = nullptr;
    SPMV_TRY(mat_alloc(ctx, SPMV_FMT_CSR, f32->nrow, f32->ncol, f32->nnz, 0, (size_t)f32->nrow + 1, (size_t)f32->nnz, (size_t)f32->nnz, &C));
    hipStream_t s  = ctx->stream;
    int         rc = hip_step(hipMemcpyAsync(const_cast<int32_t*>(C->a), f32->a, sizeof(int32_t) * ((size_t)f32->nrow + 1), hipMemcpyDeviceToDevice, s), who, "copying the row pointer");
    if (rc == SPMV_OK && f32->nnz > 0)
    {
        hipLaunchKernelGGL(f32_widen_kernel, dim3(stream_grid(f32->nnz)), dim3(kBlock), 0, s, f32->nnz, (const uint64_t*)f32->f32_ent, const_cast<int32_t*>(C->b),
                           const_cast<double*>(C->v));
        rc = hip_step(hipGetLastError(), who, "the widening pass's launch");
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

// columns and widened values of a format-6 handle into device arrays of the caller's (either may be null); asynchronous
int f32_widen_arrays(spmv_ctx* ctx, const spmv_mat* f32, int32_t* d_col, double* d_val)
{
    if (f32->nnz == 0) return SPMV_OK;
    hipLaunchKernelGGL(f32_widen_kernel, dim3(stream_grid(f32->nnz)), dim3(kBlock), 0, ctx->stream, f32->nnz, (const uint64_t*)f32->f32_ent, d_col, d_val);
    SPMV_HIP(hipGetLastError());
    return SPMV_OK;
}

// ---- the format-6 handle of A^T (transpose.hip: the companion of a format-6 handle); owns its arrays, analysed ----------------------
// Widen into an fp64 CSR copy, run the device transpose on it (spgemm.hip: csr_transpose), pack the result again (exact: every value is
// a float already).  Both fp64 intermediates - 12 nnz bytes each, plus the transpose's own set-up memory - are freed before this returns.
int f32_transpose(spmv_ctx* ctx, const spmv_mat* A, spmv_mat** out)
{
    const char* who = "spmv_mat_transpose_setup";
    spmv_mat *  W = nullptr, *T = nullptr, *R = nullptr;
    if (A->nnz == 0)  // nothing to transpose: ncol empty rows
    {
        SPMV_TRY(f32_alloc(ctx, A->ncol, A->nrow, 0, who, &R));
        int rc0 = hip_step(hipMemsetAsync(const_cast<int32_t*>(R->a), 0, sizeof(int32_t) * ((size_t)A->ncol + 1), ctx->stream), who, "clearing the row pointer");
        if (rc0 == SPMV_OK) rc0 = hip_step(hipStreamSynchronize(ctx->stream), who, "the set-up's kernels");
        if (rc0 == SPMV_OK) rc0 = csr_f32_analyse(R);
        if (rc0 != SPMV_OK)
        {
            mat_free(R);
            return rc0;
        }
        *out = R;
        return SPMV_OK;
    }
    SPMV_TRY(f32_to_csr(ctx, A, who, &W));  // (never analysed: csr_transpose reads its arrays alone)
    int rc = csr_transpose(ctx, W, &T, SPMV_CSR_VECTOR);  // (the intermediate selects nothing: forced to the kernel that needs no layout)
    mat_free(W);
    if (rc != SPMV_OK) return rc;
    rc = csr_to_f32(ctx, T, who, &R);
    (void)hipStreamSynchronize(ctx->stream);
    mat_free(T);
    if (rc == SPMV_OK) rc = csr_f32_analyse(R);
    if (rc != SPMV_OK)
    {
        if (R) mat_free(R);
        return rc;
    }
    *out = R;
    return SPMV_OK;
}
}  // namespace spmv
