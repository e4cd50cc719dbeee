// sorted_runs.hip — from values keyed by a pair (i, j) to CSR with the values of equal keys added up, on the device, on CDNA4
// (gfx950): the one pipeline behind AMG's coarse operator (amg.hip) and SpGEMM's sort path (spgemm.hip).  tests/amg_ref.py and
// tests/spgemm_ref.py are the NumPy twins of the order defined here.
//
// runs_by_key_pair.  Value ids are ordered stably by (i, j) with two passes of sort_ids_by_key, j first (key_bits(n_j) bits, then
// key_bits(n_i)); the heads of runs of equal keys are marked (head[total] = 0, so that the scan of total + 1 flags ends on the
// number of runs, which the host reads); every head then writes its run's start, i and j and counts itself into count_i.
// 24 bytes of transient memory per value beside the sort's own buffers, 12 per run, 4 per i.
//
// runs_sum_into_csr.  One lane per run adds its values from 0.0, left to right in that order, in plain additions - there is no
// product here, so nothing can contract - and writes column and sum at the run's place in its row of C.
#include "common.hpp"
#include "solver_host.hpp"
#include "sorted_runs.hpp"

namespace spmv
{
namespace
{
// out[k] = src[idx[k]]
__global__ __launch_bounds__(kBlock) void runs_gather_kernel(int64_t n, const int32_t* __restrict__ src, const int32_t* __restrict__ idx,
                                                            int32_t* __restrict__ out)
{
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += (int64_t)gridDim.x * kBlock) out[k] = src[idx[k]];
}

// head[k] = 1 where the k-th value in (i, j) order starts a run, k < total;  head[total] = 0
__global__ __launch_bounds__(kBlock) void runs_head_kernel(int64_t total, const int32_t* __restrict__ order, const int32_t* __restrict__ key_i,
                                                          const int32_t* __restrict__ key_j, int32_t* __restrict__ head)
{
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k <= total; k += (int64_t)gridDim.x * kBlock)
    {
        int32_t h = 0;
        if (k < total)
        {
            const int32_t e = order[k];
            h               = 1;
            if (k > 0)
            {
                const int32_t p = order[k - 1];
                h               = (key_i[e] != key_i[p] || key_j[e] != key_j[p]) ? 1 : 0;
            }
        }
        head[k] = h;
    }
}

// every run's start, i and j: seg_start[s] (and seg_start[runs] = total), run_i[s], run_j[s], and the runs per i
__global__ __launch_bounds__(kBlock) void runs_segment_kernel(int64_t total, const int32_t* __restrict__ order, const int32_t* __restrict__ key_i,
                                                             const int32_t* __restrict__ key_j, const int32_t* __restrict__ head,
                                                             const int32_t* __restrict__ run_of, int32_t* __restrict__ seg_start,
                                                             int32_t* __restrict__ run_i, int32_t* __restrict__ run_j, int32_t* __restrict__ count_i)
{
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k <= total; k += (int64_t)gridDim.x * kBlock)
    {
        if (k == total)
            seg_start[run_of[k]] = (int32_t)total;
        else if (head[k])
        {
            const int32_t s = run_of[k], e = order[k];
            seg_start[s]    = (int32_t)k;
            run_i[s]        = key_i[e];
            run_j[s]        = key_j[e];
            atomicAdd(count_i + key_i[e], 1);  // (an integer sum)
        }
    }
}

// one lane per run: its place in C, its column, and its values from 0.0, left to right, plain additions
__global__ __launch_bounds__(kBlock) void runs_sum_kernel(int64_t runs, const int32_t* __restrict__ seg_start, const int32_t* __restrict__ order,
                                                         const double* __restrict__ t, const int32_t* __restrict__ run_i,
                                                         const int32_t* __restrict__ run_j, const int32_t* __restrict__ run_first,
                                                         const int32_t* __restrict__ rows, const int32_t* __restrict__ c_rp,
                                                         int32_t* __restrict__ c_col, double* __restrict__ c_val)
{
    for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < runs; s += (int64_t)gridDim.x * kBlock)
    {
        double    acc = 0.0;
        const int end = seg_start[s + 1];
        for (int k = seg_start[s]; k < end; ++k) acc = __dadd_rn(acc, t[order[k]]);
        const int32_t i  = run_i[s];
        const int64_t at = (int64_t)c_rp[rows ? rows[i] : i] + (s - run_first[i]);
        c_col[at]        = run_j[s];
        c_val[at]        = acc;
    }
}
}  // namespace

int runs_by_key_pair(spmv_ctx* ctx, device_pool& pool, const char* who, const int32_t* key_i, int64_t n_i, const int32_t* key_j, int64_t n_j,
                     int64_t total, key_runs* out)
{
    hipStream_t s    = ctx->stream;
    const int   grid = stream_grid(total + 1);
    int32_t *   ids1, *key_i1, *ids2, *order, *head, *run_of;
    SPMV_TRY(pool.get(ids1, (size_t)total));
    SPMV_TRY(pool.get(key_i1, (size_t)total));
    SPMV_TRY(pool.get(ids2, (size_t)total));
    SPMV_TRY(pool.get(order, (size_t)total));
    SPMV_TRY(sort_ids_by_key(ctx, key_j, total, key_bits(n_j), ids1));
    hipLaunchKernelGGL(runs_gather_kernel, dim3(grid), dim3(kBlock), 0, s, total, key_i, (const int32_t*)ids1, key_i1);
    SPMV_TRY(sort_ids_by_key(ctx, key_i1, total, key_bits(n_i), ids2));
    hipLaunchKernelGGL(runs_gather_kernel, dim3(grid), dim3(kBlock), 0, s, total, (const int32_t*)ids1, (const int32_t*)ids2, order);
    SPMV_TRY(pool.get(head, (size_t)total + 1));
    SPMV_TRY(pool.get(run_of, (size_t)total + 1));
    hipLaunchKernelGGL(runs_head_kernel, dim3(grid), dim3(kBlock), 0, s, total, (const int32_t*)order, key_i, key_j, head);
    SPMV_TRY(hip_step(hipGetLastError(), who, "the head marking's launch"));
    SPMV_TRY(exclusive_scan_i32(ctx, head, run_of, total + 1));
    int32_t runs = 0;
    SPMV_TRY(read_scalars(ctx, &runs, run_of + total, sizeof(runs), who));
    SPMV_REQUIRE(runs >= 1 && runs <= total, "%s: %d runs of equal keys from %lld values", who, runs, (long long)total);
    SPMV_TRY(pool.get(out->seg_start, (size_t)runs + 1));
    SPMV_TRY(pool.get(out->run_i, (size_t)runs));
    SPMV_TRY(pool.get(out->run_j, (size_t)runs));
    SPMV_TRY(pool.get(out->count_i, (size_t)n_i + 1));
    SPMV_TRY(hip_step(hipMemsetAsync(out->count_i, 0, sizeof(int32_t) * ((size_t)n_i + 1), s), who, "clearing the runs' counts"));
    hipLaunchKernelGGL(runs_segment_kernel, dim3(grid), dim3(kBlock), 0, s, total, (const int32_t*)order, key_i, key_j, (const int32_t*)head,
                       (const int32_t*)run_of, out->seg_start, out->run_i, out->run_j, out->count_i);
    SPMV_TRY(hip_step(hipGetLastError(), who, "the segment kernel's launch"));
    out->runs  = runs;
    out->order = order;
    return SPMV_OK;
}

int runs_sum_into_csr(spmv_ctx* ctx, const char* who, const key_runs& kr, const double* t, const int32_t* run_first, const int32_t* rows,
                      const int32_t* c_rp, int32_t* c_col, double* c_val)
{
    hipLaunchKernelGGL(runs_sum_kernel, dim3(stream_grid(kr.runs)), dim3(kBlock), 0, ctx->stream, (int64_t)kr.runs, (const int32_t*)kr.seg_start,
                       (const int32_t*)kr.order, t, (const int32_t*)kr.run_i, (const int32_t*)kr.run_j, run_first, rows, c_rp, c_col, c_val);
    return hip_step(hipGetLastError(), who, "the run sum's launch");
}
}  // namespace spmv
