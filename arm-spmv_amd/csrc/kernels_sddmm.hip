// kernels_sddmm.hip — the sampled dense-dense product (spmv_sddmm) on CDNA4 (gfx950):
//     out[e] = alpha * sum_{c < k} U[row(e), c] * V[col(e), c] + beta * out[e]        for every stored entry e of a CSR pattern.
//
// U (nrow x k) and V (ncol x k) are ROW-MAJOR as in spmv_apply_multi (kernels_spmm.hip); out has nnz entries in the handle's entry
// order.  The pattern's values are never read.  Algorithmic bytes per call: 4*nnz (columns) + 4*(nrow+1) + 8*nnz (16*nnz with
// beta != 0) + 8*nrow*k + 8*ncol*k.
//
// Work is divided by ENTRIES (sddmm_settings.hpp): a wavefront takes a run of kSddmmRun entries wherever they lie, finds the rows of
// the run's first and last entry (wave_row_of: all 64 lanes probe row_ptr at once, 64-ary, 4 steps for 16M rows), and walks the run in
// chunks of 64: lane l loads the column of entry chunk + l, its old value where beta != 0 (both ahead of the gathers), and finds the
// entry's row by a binary search between the run's two rows (no step at all inside one long row).  A row of 1M entries is 2048 runs
// like any others.
//   sddmm_kernel<L>     L = 2 .. 64 lanes make an entry, lane t column t, lanes t >= k masked ON THEIR LOADS; group g of a wavefront makes
//                       the entries chunk + g L + i one after the other: column and row come along the group by ds_bpermute, U's row is
//                       loaded only where the row differs from the group's previous entry (held in a register across a row segment),
//                       the gathers V[col * k + t] of sddmm_batch(L) entries (8 k contiguous bytes per entry and group) are issued
//                       before their multiplies, the products are summed by the xor butterfly of wave.hpp (ds_swizzle, no LDS
//                       memory), which leaves the sum in every lane: lane i keeps step i's, the sum of the entry it stores.
//   sddmm_k1_kernel     k = 1 (the gradient of y = A x in A's values): a lane an entry, no reduction, kSddmmK1Depth chunks in flight.
//
// Order of the additions (the contract of spmv_sddmm): each product U[i, c] * V[j, c] is rounded on its own (no fma); with
// L = the next power of two >= k and p_c = 0.0 for k <= c < L, s = the pairwise tree p_c + p_(c xor 1), then + the sum at
// (c xor 2), (c xor 4), ... (both partners of a pair compute the same sum: addition is commutative); then out = alpha * s where
// beta == 0.0 (out is not read), else fma(alpha, s, beta * out).  The order depends on k alone.
#include "common.hpp"
#include "sddmm_settings.hpp"
#include "wave.hpp"

namespace spmv
{
namespace
{
// the row r with row_ptr[r] <= e < row_ptr[r + 1], found by a whole wavefront (every lane active, e uniform and below row_ptr[nrow]):
// lane l probes the l-th of 64 evenly spaced rows of [lo, hi], the number of probes at or below e narrows the range 64-fold
__device__ __forceinline__ int wave_row_of(const int32_t* __restrict__ row_ptr, int nrow, int64_t e)
{
    int       lo = 0, hi = nrow;  // row_ptr[lo] <= e < row_ptr[hi]
    const int lane = lane_id();
    while (hi - lo > 1)
    {
        const int64_t step = ((int64_t)hi - lo + kSddmmWave - 1) / kSddmmWave;
        const int64_t p    = std::min<int64_t>(lo + lane * step, hi);
        const int     n    = __popcll(__ballot(row_ptr[p] <= e));  // >= 1: lane 0 probes lo
        hi                 = (int)std::min<int64_t>(lo + n * step, hi);
        lo                 = (int)(lo + (n - 1) * step);
    }
    return lo;
}

// the same for one lane's entry between the rows of its run's first and last entry: row_ptr[lo] <= e < row_ptr[hi + 1]
__device__ __forceinline__ int lane_row_of(const int32_t* __restrict__ row_ptr, int lo, int hi, int64_t e)
{
    ++hi;
    while (hi - lo > 1)
    {
        const int mid = lo + (hi - lo) / 2;
        if (row_ptr[mid] <= e)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

template <int L>
__global__ __launch_bounds__(kSddmmBlock) void sddmm_kernel(int nrow, int k, int64_t nnz, int64_t nruns,
                                                            const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                            const double* __restrict__ U, const double* __restrict__ V, double alpha,
                                                            double beta, double* __restrict__ out)
{
    constexpr int B     = sddmm_batch(L);
    const int     lane  = lane_id();
    const int     t     = sddmm_column_of_lane(lane, L);
    const int     first = lane - t;  // the group's first lane: the entries chunk + first + i are the group's
    const bool    live  = t < k;
    const int64_t waves = (int64_t)gridDim.x * sddmm_waves_per_block();
    for (int64_t run = (int64_t)blockIdx.x * sddmm_waves_per_block() + threadIdx.x / kSddmmWave; run < nruns; run += waves)
    {
        const int64_t e0 = sddmm_run_begin(run), e1 = sddmm_run_end(run, nnz);
        const int     r0 = wave_row_of(row_ptr, nrow, e0);
        const int     r1 = wave_row_of(row_ptr, nrow, e1 - 1);
        int           held = -1;  // the row whose U[row, t] the lane holds in u
        double        u    = 0.0;
        for (int64_t c0 = e0; c0 < e1; c0 += kSddmmChunk)
        {
            const int64_t e    = c0 + lane;
            const bool    mine = e < e1;
            const int     n    = (int)std::min<int64_t>(kSddmmChunk, e1 - c0);  // uniform: the chunk's entries
            const double  o0   = (mine && beta != 0.0) ? out[e] : 0.0;          // ahead of the gathers
            const int     cj   = mine ? load_stream(col + e) : 0;
            const int     ri   = mine ? lane_row_of(row_ptr, r0, r1, e) : 0;
            double        res  = 0.0;
#pragma unroll 1
            for (int b = 0; b < L; b += B)  // (one trip for L <= 16)
            {
                int    rr[B], cc[B];
                double ul[B], vg[B];
                int    ahead = held;  // the row held once the loads below have landed
#pragma unroll
                for (int i = 0; i < B; ++i)
                {
                    const int src = first + b + i;  // the lane that loaded this entry's column and row
                    rr[i]         = bpermute(ri, src);
                    cc[i]         = bpermute(cj, src);
                    const bool ok = live && src < n;
                    ul[i]         = (ok && rr[i] != ahead) ? U[(int64_t)rr[i] * k + t] : 0.0;
                    if (ok) ahead = rr[i];
                }
#pragma unroll
                for (int i = 0; i < B; ++i) vg[i] = (live && first + b + i < n) ? V[(int64_t)cc[i] * k + t] : 0.0;
#pragma unroll
                for (int i = 0; i < B; ++i)
                {
                    const bool ok = live && first + b + i < n;
                    if (ok && rr[i] != held)
                    {
                        u    = ul[i];
                        held = rr[i];
                    }
                    const double p = ok ? u * vg[i] : 0.0;
                    const double s = group_sum_swizzle<L>(p);
                    if (t == b + i) res = s;
                }
            }
            if (mine) out[e] = beta != 0.0 ? fma(alpha, res, beta * o0) : alpha * res;
        }
    }
}

__global__ __launch_bounds__(kSddmmBlock) void sddmm_k1_kernel(int nrow, int64_t nnz, int64_t nruns,
                                                               const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                               const double* __restrict__ U, const double* __restrict__ V, double alpha,
                                                               double beta, double* __restrict__ out)
{
    constexpr int D     = kSddmmK1Depth;
    const int     lane  = lane_id();
    const int64_t waves = (int64_t)gridDim.x * sddmm_waves_per_block();
    for (int64_t run = (int64_t)blockIdx.x * sddmm_waves_per_block() + threadIdx.x / kSddmmWave; run < nruns; run += waves)
    {
        const int64_t e0 = sddmm_run_begin(run), e1 = sddmm_run_end(run, nnz);
        const int     r0 = wave_row_of(row_ptr, nrow, e0);
        const int     r1 = wave_row_of(row_ptr, nrow, e1 - 1);
        for (int64_t c0 = e0; c0 < e1; c0 += D * kSddmmChunk)
        {
            double o0[D], ug[D], vg[D];
            int    cj[D];
#pragma unroll
            for (int q = 0; q < D; ++q)
            {
                const int64_t e = c0 + q * kSddmmChunk + lane;
                o0[q]           = (e < e1 && beta != 0.0) ? out[e] : 0.0;
                cj[q]           = e < e1 ? load_stream(col + e) : 0;
            }
#pragma unroll
            for (int q = 0; q < D; ++q)
            {
                const int64_t e = c0 + q * kSddmmChunk + lane;
                ug[q]           = e < e1 ? U[lane_row_of(row_ptr, r0, r1, e)] : 0.0;
                vg[q]           = e < e1 ? V[cj[q]] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < D; ++q)
            {
                const int64_t e = c0 + q * kSddmmChunk + lane;
                const double  s = ug[q] * vg[q];
                if (e < e1) out[e] = beta != 0.0 ? fma(alpha, s, beta * o0[q]) : alpha * s;
            }
        }
    }
}

template <int L>
int launch(spmv_ctx* ctx, const spmv_mat* A, int32_t k, double alpha, const double* U, const double* V, double beta, double* out)
{
    const int64_t nruns = sddmm_runs(A->nnz);
    const dim3    grid((unsigned)sddmm_grid(nruns, kSddmmMaxGrid));
    if constexpr (L == 1)
        hipLaunchKernelGGL(sddmm_k1_kernel, grid, dim3(kSddmmBlock), 0, ctx->stream, A->nrow, A->nnz, nruns, A->a, A->b, U, V, alpha, beta,
                           out);
    else
        hipLaunchKernelGGL((sddmm_kernel<L>), grid, dim3(kSddmmBlock), 0, ctx->stream, A->nrow, k, A->nnz, nruns, A->a, A->b, U, V, alpha,
                           beta, out);
    SPMV_HIP(hipGetLastError());
    return SPMV_OK;
}
}  // namespace

// a CSR handle with its index arrays; U nrow x k, V ncol x k, out nnz entries (checked by the caller: abi.hip)
int sddmm_apply(spmv_ctx* ctx, const spmv_mat* A, int32_t k, double alpha, const double* U, const double* V, double beta, double* out)
{
    if (A->nnz == 0 || A->nrow == 0 || A->ncol == 0) return SPMV_OK;
    switch (sddmm_lanes(k))
    {
        case 1: return launch<1>(ctx, A, k, alpha, U, V, beta, out);
        case 2: return launch<2>(ctx, A, k, alpha, U, V, beta, out);
        case 4: return launch<4>(ctx, A, k, alpha, U, V, beta, out);
        case 8: return launch<8>(ctx, A, k, alpha, U, V, beta, out);
        case 16: return launch<16>(ctx, A, k, alpha, U, V, beta, out);
        case 32: return launch<32>(ctx, A, k, alpha, U, V, beta, out);
        default: return launch<64>(ctx, A, k, alpha, U, V, beta, out);
    }
}
}  // namespace spmv
