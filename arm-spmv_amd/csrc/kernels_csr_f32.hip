// kernels_csr_f32.hip - y += A*x for CSR with single-precision value storage (SPMV_FMT_CSR_F32) on CDNA4 (gfx950).
//
// Bytes per stored entry: 8 - one packed word, the column in its low half, the float value's bits in its high half
// (csr_f32_settings.hpp) - against the 12 of CSR.  x is gathered, the sums are accumulated and y is written in fp64.  The product
// is memory-bound; what the narrower stream buys where is DESIGN.md 26.
//
// csr_f32_kernel<LPR> is the row-parallel CSR kernel's arrangement (kernels_csr.hip: csr_vector_kernel) over that stream: LPR = 2^k
// lanes cooperate on one row, lane l of the group walks entries l, l + LPR, ...; ONE 8-byte nontemporal load per entry takes the
// place of that kernel's two (4 and 8 bytes); four entries are in flight per lane, then their four gathers of x, then
// sum = fma((double)v, x, sum) in the same order; group_sum<LPR, false> (wave.hpp) joins the lanes - no atomics touch y; the
// write-back is that kernel's, apply_extra's overwrite and fused dot included.  Entry offsets are 64-bit.
//
// THE CONTRACT.  Because the order of operations is csr_vector_kernel<LPR, false, false>'s, a product of a format-6 handle returns
// the same bits as the product of the fp64 CSR handle that holds the widened values, forced to SPMV_CSR_VECTOR at the same lanes
// per row with default flags (tests/test_gpu_csr_f32.py holds it to that at every lane count).
#include "common.hpp"
#include "csr_f32_settings.hpp"
#include "wave.hpp"

namespace spmv
{
namespace
{
static_assert(kCsrF32Workgroup == kBlock && kCsrF32MaxLanes == kWave, "csr_f32_settings.hpp describes this chip's workgroup and wavefront");

template <int LPR>
__global__ __launch_bounds__(kCsrF32Workgroup) void csr_f32_kernel(int nrow, const int32_t* __restrict__ row_ptr, const uint64_t* __restrict__ ent,
                                                                   const double* __restrict__ x, double* __restrict__ y, int overwrite,
                                                                   const double* __restrict__ dot_w, double* __restrict__ dot_out)
{
    static_assert(csr_f32_lanes_valid(LPR) && kCsrF32InFlight == 4, "the loop below keeps four entries in flight");
    constexpr int ROWS = csr_f32_rows_per_workgroup(LPR);
    const int     row  = blockIdx.x * ROWS + threadIdx.x / LPR;
    const int     sub  = threadIdx.x % LPR;

    double sum = 0.0;
    if (row < nrow)
    {
        int64_t       j   = (int64_t)row_ptr[row] + sub;
        const int64_t end = row_ptr[row + 1];
        for (; j + 3 * LPR < end; j += 4 * LPR)
        {
            const uint64_t e0 = load_stream(ent + j);
            const uint64_t e1 = load_stream(ent + j + LPR);
            const uint64_t e2 = load_stream(ent + j + 2 * LPR);
            const uint64_t e3 = load_stream(ent + j + 3 * LPR);
            const double   x0 = x[f32_entry_col(e0)];
            const double   x1 = x[f32_entry_col(e1)];
            const double   x2 = x[f32_entry_col(e2)];
            const double   x3 = x[f32_entry_col(e3)];
            sum = fma((double)f32_entry_value(e0), x0, sum);
            sum = fma((double)f32_entry_value(e1), x1, sum);
            sum = fma((double)f32_entry_value(e2), x2, sum);
            sum = fma((double)f32_entry_value(e3), x3, sum);
        }
        for (; j < end; j += LPR)
        {
            const uint64_t e = load_stream(ent + j);
            sum              = fma((double)f32_entry_value(e), x[f32_entry_col(e)], sum);
        }
    }
    // every lane of the wave takes part in the cross-lane step (no early exit above)
    sum = group_sum<LPR, false>(sum);
    // y += sum, or y = sum; the solver's dot product w . y_new rides along (spmv_apply_dot): the row-parallel CSR kernel's write-back
    double part = 0.0;
    if (row < nrow && sub == 0)
    {
        const double yn = overwrite ? sum : y[row] + sum;
        y[row]          = yn;
        if (dot_w) part = dot_w[row] * yn;
    }
    if (dot_w)  // uniform over the grid
    {
        part = wave_sum(part);
        if ((threadIdx.x & 63) == 0) slot_add(dot_out, part);
    }
}

// the longest row
__global__ __launch_bounds__(kBlock) void csr_f32_row_max_kernel(int nrow, const int32_t* __restrict__ row_ptr, int32_t* __restrict__ out)
{
    int most = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nrow; i += (int64_t)gridDim.x * kBlock) most = max(most, row_ptr[i + 1] - row_ptr[i]);
    for (int off = 32; off > 0; off >>= 1) most = max(most, __shfl_xor(most, off));
    if ((threadIdx.x & 63) == 0 && most > 0) atomicMax(out, most);
}

template <int LPR>
void launch_f32(spmv_ctx* ctx, const spmv_mat* A, const double* x, double* y, const apply_extra& ex)
{
    hipLaunchKernelGGL((csr_f32_kernel<LPR>), dim3((unsigned)csr_f32_grid(A->nrow, LPR)), dim3(kCsrF32Workgroup), 0, ctx->stream, A->nrow, A->a,
                       (const uint64_t*)A->f32_ent, x, y, ex.overwrite ? 1 : 0, ex.dot_w, ex.dot_out);
}
}  // namespace

// The product of a format-6 handle; takes apply_extra into its write-back (kernels_csr.hip: fuses_extras).
int csr_f32_apply(spmv_ctx* ctx, const spmv_mat* A, const double* x, double* y, const apply_extra& ex)
{
    if (A->nrow == 0) return SPMV_OK;
    if (!csr_f32_lanes_valid(A->lanes_per_row)) SPMV_FAIL(SPMV_ERR_INVALID, "format 6 product: lanes_per_row must be a power of two in 1..64, got %d", A->lanes_per_row);
    switch (csr_f32_lanes_that_fit(A->nrow, A->lanes_per_row))
    {
        case 1: launch_f32<1>(ctx, A, x, y, ex); break;
        case 2: launch_f32<2>(ctx, A, x, y, ex); break;
        case 4: launch_f32<4>(ctx, A, x, y, ex); break;
        case 8: launch_f32<8>(ctx, A, x, y, ex); break;
        case 16: launch_f32<16>(ctx, A, x, y, ex); break;
        case 32: launch_f32<32>(ctx, A, x, y, ex); break;
        default: launch_f32<64>(ctx, A, x, y, ex); break;
    }
    SPMV_HIP(hipGetLastError());
    return SPMV_OK;
}

// Row statistics and the lanes per row.  Runs once when a format-6 handle is created; no plan, no trial: the format has one kernel.
int csr_f32_analyse(spmv_mat* m)
{
    spmv_ctx* ctx  = m->ctx;
    int32_t   most = 0;
    if (m->nrow > 0 && m->nnz > 0)
    {
        SPMV_TRY(ensure_scratch(ctx, 64));
        int32_t* d = (int32_t*)ctx->scratch;
        SPMV_HIP(hipMemsetAsync(d, 0, sizeof(int32_t), ctx->stream));
        hipLaunchKernelGGL(csr_f32_row_max_kernel, dim3(stream_grid(m->nrow)), dim3(kBlock), 0, ctx->stream, m->nrow, m->a, d);
        SPMV_HIP(hipGetLastError());
        SPMV_HIP(hipMemcpyAsync(&most, d, sizeof(most), hipMemcpyDeviceToHost, ctx->stream));
        SPMV_HIP(hipStreamSynchronize(ctx->stream));
    }
    m->max_row_nnz   = most;
    m->kernel        = SPMV_CSR_VECTOR;
    m->lanes_per_row = csr_pick_lanes(m->nrow > 0 ? (double)m->nnz / (double)m->nrow : 0.0);
    return SPMV_OK;
}

// spmv_mat_set_kernel on a format-6 handle: one kernel (AUTO picks the lanes again, VECTOR takes the caller's or keeps what is there).
// Every refusal comes before the handle is written.
int csr_f32_set_kernel(spmv_mat* m, int32_t kernel, int32_t lanes)
{
    if (kernel != SPMV_CSR_AUTO && kernel != SPMV_CSR_VECTOR)
        SPMV_FAIL(SPMV_ERR_UNSUPPORTED, "spmv_mat_set_kernel: a handle of format 6 has one kernel: AUTO (0) or VECTOR (1), got %d", kernel);
    if (lanes != 0 && !csr_f32_lanes_valid(lanes))
        SPMV_FAIL(SPMV_ERR_UNSUPPORTED, "spmv_mat_set_kernel: a row of a format 6 handle takes 0 (keep / choose) or a power of two up to 64 lanes, got %d", lanes);
    if (lanes > 0)
        m->lanes_per_row = lanes;
    else if (kernel == SPMV_CSR_AUTO)
        m->lanes_per_row = csr_pick_lanes(m->nrow > 0 ? (double)m->nnz / (double)m->nrow : 0.0);
    m->kernel        = SPMV_CSR_VECTOR;
    m->kernel_forced = kernel != SPMV_CSR_AUTO;
    return SPMV_OK;
}
}  // namespace spmv
