// kernels_bsr.hip - y += A*x for block CSR (square blocks of bs x bs values, row-major, bs in 2 .. 8) on CDNA4 (gfx950).
//
// Bytes per stored value: 8 of the value and 4 / bs^2 of the block's column, against 12 in CSR; one gathered stretch of x (bs
// contiguous doubles) serves the bs rows of a block.  The product is memory-bound: no MFMA.
//
// bsr_vector_kernel<BS, G, EDGE>.  The lane map, the lanes per block row, the reduction's partners and the grid are those of
// bsr_settings.hpp.  A block row's values are one contiguous run: a group of G * BS^2 lanes reads G whole blocks of it per step
// with consecutive lanes on consecutive doubles, every lane on the (r, c) position it keeps for the whole loop, four steps in flight,
// one accumulator per lane.  The sums of a scalar row meet in a fixed shift-down tree over ds_bpermute (wave.hpp): no atomics, and
// the same bits at every launch.  Value offsets are 64-bit.
//
// Positions of a stored block outside nrow x ncol are absent.  Rows: a lane whose scalar row is >= nrow adds into no lane that
// stores (its partners hold the same r) and stores nothing, so the loop knows nothing of the last block row.  Columns: only where
// ncol is no multiple of BS (EDGE) does a lane compare its block's column with the first block column that is out of range for
// its c - a compare and two selects, the same for every block, no branch; x is then read at a clamped index and neither it nor the
// stored value reaches the sum.  Where ncol is a multiple of BS the loop has none of it.
#include "bsr_settings.hpp"
#include "common.hpp"
#include "wave.hpp"

namespace spmv
{
namespace
{
// the shift-down tree of bsr_settings.hpp over W positions UNIT lanes apart; `pos` is this lane's position
template <int W, int UNIT>
__device__ __forceinline__ double bsr_tree_sum(double v, int pos)
{
    if constexpr (W > 1)
    {
        constexpr int H = bsr_half(W);
        const double  t = bpermute(v, (lane_id() + H * UNIT) & (kWave - 1));
        if (pos + H < W) v += t;
        return bsr_tree_sum<H, UNIT>(v, pos);
    }
    else
        return v;
}

template <int BS, int G, bool EDGE>
__global__ __launch_bounds__(kBsrWorkgroup) void bsr_vector_kernel(int mb, int nrow, int ncol, const int32_t* __restrict__ brow_ptr,
                                                                   const int32_t* __restrict__ bcol, const double* __restrict__ val,
                                                                   const double* __restrict__ x, double* __restrict__ y)
{
    constexpr int  BS2 = BS * BS, LANES = G * BS2;
    const bsr_lane L    = bsr_lane_map(BS, LANES, (int)threadIdx.x & (kWave - 1));
    const int64_t  brow = bsr_first_row(blockIdx.x, (int)threadIdx.x / kWave, BS, LANES) + L.row;
    const bool     mine = L.active && brow < mb;

    double sum = 0.0;
    if (mine)
    {
        int           b   = brow_ptr[brow] + L.block;
        const int     end = brow_ptr[brow + 1];
        const double* v   = val + bsr_value_offset(0, BS, L.r, L.c);
        const double* xc  = x + L.c;
        // EDGE: block columns >= lim hold a column >= ncol at this lane's c (bc * BS + c < ncol  <=>  bc < ceil((ncol - c) / BS))
        const int lim  = EDGE ? (ncol - L.c + BS - 1) / BS : 0;
        const int last = ncol - 1;  // (EDGE: x is read at min(column, last); a handle with blocks has ncol >= 1)
        // one term: the block's column, the lane's value of it and its x; EDGE: both selected away beyond the last column
        auto load = [&](int at, double& vv, double& xx) {
            const int bc = load_stream(bcol + at);
            vv           = load_stream(v + (int64_t)at * BS2);
            if constexpr (EDGE)
            {
                xx = x[min(bc * BS + L.c, last)];
                xx = bc < lim ? xx : 0.0;
                vv = bc < lim ? vv : 0.0;
            }
            else
                xx = xc[bc * BS];
        };
        for (; b + 3 * G < end; b += 4 * G)  // four steps in flight before the first fma
        {
            double v0, v1, v2, v3, x0, x1, x2, x3;
            load(b, v0, x0);
            load(b + G, v1, x1);
            load(b + 2 * G, v2, x2);
            load(b + 3 * G, v3, x3);
            sum = fma(v0, x0, sum);
            sum = fma(v1, x1, sum);
            sum = fma(v2, x2, sum);
            sum = fma(v3, x3, sum);
        }
        for (; b < end; b += G)
        {
            double v0, x0;
            load(b, v0, x0);
            sum = fma(v0, x0, sum);
        }
    }
    // every lane of the wavefront takes part in the cross-lane steps (no early exit above)
    sum = bsr_tree_sum<BS, 1>(sum, L.c);
    sum = bsr_tree_sum<G, BS2>(sum, L.block);
    if (mine && L.block == 0 && L.c == 0)
    {
        const int64_t row = brow * BS + L.r;
        if (row < nrow) y[row] += sum;
    }
}

// the most blocks in a block row
__global__ __launch_bounds__(kBlock) void bsr_row_max_kernel(int mb, const int32_t* __restrict__ brow_ptr, int32_t* __restrict__ out)
{
    int most = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < mb; i += (int64_t)gridDim.x * kBlock) most = max(most, brow_ptr[i + 1] - brow_ptr[i]);
    for (int off = 32; off > 0; off >>= 1) most = max(most, __shfl_xor(most, off));
    if ((threadIdx.x & 63) == 0 && most > 0) atomicMax(out, most);
}

template <int BS, int G>
int launch_bsr(spmv_ctx* ctx, const spmv_mat* A, const double* x, double* y)
{
    const int    mb   = (int)ceil_div(A->nrow, BS);
    const auto   grid = dim3((unsigned)bsr_grid(mb, BS, G * BS * BS));
    if (A->ncol % BS)
        hipLaunchKernelGGL((bsr_vector_kernel<BS, G, true>), grid, dim3(kBsrWorkgroup), 0, ctx->stream, mb, A->nrow, A->ncol, A->a, A->b, A->v, x, y);
    else
        hipLaunchKernelGGL((bsr_vector_kernel<BS, G, false>), grid, dim3(kBsrWorkgroup), 0, ctx->stream, mb, A->nrow, A->ncol, A->a, A->b, A->v, x, y);
    SPMV_HIP(hipGetLastError());
    return SPMV_OK;
}
}  // namespace

int bsr_apply(spmv_ctx* ctx, const spmv_mat* A, const double* x, double* y)
{
    if (A->nrow == 0 || A->nnz == 0) return SPMV_OK;
    const int bs = A->k, g = A->lanes_per_row / (bs * bs);
    if (!bsr_lanes_valid(bs, A->lanes_per_row)) SPMV_FAIL(SPMV_ERR_INVALID, "BSR product: %d lanes per block row of %d x %d blocks", A->lanes_per_row, bs, bs);
    switch (bs * 100 + g)
    {
        case 201: return launch_bsr<2, 1>(ctx, A, x, y);
        case 202: return launch_bsr<2, 2>(ctx, A, x, y);
        case 204: return launch_bsr<2, 4>(ctx, A, x, y);
        case 208: return launch_bsr<2, 8>(ctx, A, x, y);
        case 216: return launch_bsr<2, 16>(ctx, A, x, y);
        case 301: return launch_bsr<3, 1>(ctx, A, x, y);
        case 307: return launch_bsr<3, 7>(ctx, A, x, y);
        case 401: return launch_bsr<4, 1>(ctx, A, x, y);
        case 402: return launch_bsr<4, 2>(ctx, A, x, y);
        case 404: return launch_bsr<4, 4>(ctx, A, x, y);
        case 501: return launch_bsr<5, 1>(ctx, A, x, y);
        case 502: return launch_bsr<5, 2>(ctx, A, x, y);
        case 601: return launch_bsr<6, 1>(ctx, A, x, y);
        case 701: return launch_bsr<7, 1>(ctx, A, x, y);
        case 801: return launch_bsr<8, 1>(ctx, A, x, y);
        default: SPMV_FAIL(SPMV_ERR_INVALID, "BSR product: no kernel for %d lanes per block row of %d x %d blocks", A->lanes_per_row, bs, bs);
    }
}

// Block-row statistics and the lanes per block row.  Runs once when a BSR handle is created.
int bsr_analyse(spmv_mat* m)
{
    spmv_ctx*     ctx  = m->ctx;
    const int     bs   = m->k;
    const int64_t nnzb = m->nnz / (bs * bs);
    const int     mb   = (int)ceil_div(m->nrow, bs);
    // the kernel steps its block index in int32 (b + 4 G): keep clear of the wrap
    SPMV_REQUIRE(nnzb <= (int64_t)INT32_MAX - 65536, "BSR handle with %lld blocks (int32 block offsets)", (long long)nnzb);
    int32_t most = 0;
    if (mb > 0 && nnzb > 0)
    {
        SPMV_TRY(ensure_scratch(ctx, 64));
        int32_t* d = (int32_t*)ctx->scratch;
        SPMV_HIP(hipMemsetAsync(d, 0, sizeof(int32_t), ctx->stream));
        hipLaunchKernelGGL(bsr_row_max_kernel, dim3(stream_grid(mb)), dim3(kBlock), 0, ctx->stream, mb, m->a, d);
        SPMV_HIP(hipGetLastError());
        SPMV_HIP(hipMemcpyAsync(&most, d, sizeof(most), hipMemcpyDeviceToHost, ctx->stream));
        SPMV_HIP(hipStreamSynchronize(ctx->stream));
    }
    m->max_row_nnz   = (int32_t)std::min<int64_t>((int64_t)most * bs, INT32_MAX);
    m->kernel        = SPMV_CSR_VECTOR;
    m->lanes_per_row = bsr_pick_lanes(bs, mb > 0 ? (double)nnzb / (double)mb : 0.0);
    int rc;
    if (plan_analyse(m, &rc)) return rc;  // the plan's lanes per block row
    return SPMV_OK;
}

// spmv_mat_set_kernel on a BSR handle: one kernel (AUTO picks the lanes again, VECTOR takes the caller's or keeps what is there)
int bsr_set_kernel(spmv_mat* m, int32_t kernel, int32_t lanes)
{
    SPMV_REQUIRE(kernel == SPMV_CSR_AUTO || kernel == SPMV_CSR_VECTOR, "spmv_mat_set_kernel: a BSR handle has one kernel: AUTO (0) or VECTOR (1), got %d", kernel);
    SPMV_REQUIRE(lanes == 0 || bsr_lanes_valid(m->k, lanes),
                 "spmv_mat_set_kernel: a block row of %d x %d blocks takes %d times a divisor of %d lanes, got %d", m->k, m->k, m->k * m->k, bsr_slots(m->k), lanes);
    const int     bs = m->k;
    const int64_t mb = ceil_div(m->nrow, bs);
    if (lanes > 0)
        m->lanes_per_row = lanes;
    else if (kernel == SPMV_CSR_AUTO)
        m->lanes_per_row = bsr_pick_lanes(bs, mb > 0 ? (double)(m->nnz / (bs * bs)) / (double)mb : 0.0);
    m->kernel        = SPMV_CSR_VECTOR;
    m->kernel_forced = kernel != SPMV_CSR_AUTO;
    return SPMV_OK;
}

int bsr_apply_plan(spmv_mat* m)
{
    const plan_node* p = plan_of(m);
    SPMV_REQUIRE(p->kernel == SPMV_CSR_VECTOR, "plan: a BSR handle runs kernel VECTOR (1), the plan names %d", p->kernel);
    SPMV_REQUIRE(bsr_lanes_valid(m->k, p->lanes_per_row), "plan: %d lanes per block row do not fit blocks of %d x %d", p->lanes_per_row, m->k, m->k);
    m->kernel        = SPMV_CSR_VECTOR;
    m->lanes_per_row = p->lanes_per_row;
    return SPMV_OK;
}
}  // namespace spmv
