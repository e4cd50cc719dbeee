// solver_common.hpp — the device side of what the solvers share (spmv_cg in solver.hip, spmv_cg_multi in solver_multi.hip,
// spmv_cgls in solver_cgls.hip, spmv_bicgstab in solver_bicgstab.hip, spmv_gmres in solver_gmres.hip, spmv_minres in
// solver_minres.hip): the sums over a workgroup
// and the deterministic sum over a grid (the last-ticket pattern).  The host side they share is solver_host.hpp.
#pragma once

#include "common.hpp"
#include "wave.hpp"

namespace spmv
{
// ---- sums over the workgroup ---------------------------------------------------------------------------------------------------
// Both add in the same order: xor butterfly inside a wavefront (wave_sum), then the four wavefronts in order.  They differ in who
// holds the result and in whose LDS they use, and so in their barriers: neither is written through the other.

// valid in thread 0; its own LDS array (two calls in one kernel: a __syncthreads() between them)
static __device__ __forceinline__ double block_sum(double v)
{
    __shared__ double s_part[kBlock / kWave];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    double total = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < kBlock / kWave; ++w) total += s_part[w];
    return total;
}

// valid in every thread; the caller's LDS array (kBlock / kWave doubles)
static __device__ __forceinline__ double block_sum_all(double v, double* s_part)
{
    v = wave_sum(v);
    __syncthreads();  // the previous call's readers are done with s_part
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < kBlock / kWave; ++w) t += s_part[w];
    return t;
}

// ---- the deterministic sum over the grid: the last-ticket pattern --------------------------------------------------------------
// Every workgroup stores its partial sums in a buffer and takes a ticket from one atomic counter; the workgroup that takes the last
// ticket of the launch adds the buffer up in buffer order and writes the scalars the next launch reads (and the ticket back to 0).
// No atomic adds in arrival order: which workgroup comes last changes nothing, the order of the additions belongs to the buffer.

// True (in every thread) for the workgroup that stored its partial sums last: all the others' are visible to it.  Thread 0 alone
// fences, before its ticket and - if it was last - behind it: a fence by all 256 threads costs two to four times one lane's, in
// every workgroup of every launch.  One lane's fence is enough because
//   - a workgroup's partial sums are stored by threads of wavefront 0, thread 0's own: thread 0 alone in grid_totals below, the
//     threads < KP <= 64 in spmv_cg_multi's store_partials;
//   - the leading __syncthreads() orders those stores (and every thread's reads of the launch's scalars, which the last workgroup
//     is about to overwrite) ahead of the fence;
//   - the last workgroup reads the partial sums with agent-scope atomic loads (partial_sum_load) behind the trailing barrier.
// (What the launch writes into the vectors needs no fence: its readers are later launches.)
static __device__ __forceinline__ bool took_last_ticket(uint32_t* ticket)
{
    __shared__ uint32_t s_last;
    __syncthreads();  // every thread of the workgroup has read the launch's scalars: the last workgroup may write them
    if (threadIdx.x == 0)
    {
        __threadfence();  // this workgroup's partial sums before its ticket
        const bool last = atomicAdd(ticket, 1u) == gridDim.x - 1;
        if (last) __threadfence();  // the ticket before the others' partial sums (which are read with atomic loads besides)
        s_last = last ? 1u : 0u;
    }
    __syncthreads();
    return s_last != 0;
}

// another workgroup's partial sum, by an atomic load: straight from memory, whatever an earlier launch left in this CU's caches
static __device__ __forceinline__ double partial_sum_load(const double* p)
{
    return __longlong_as_double((long long)__hip_atomic_load((const unsigned long long*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// The launch's totals of NQ per-thread sums: part[q * gridDim.x + workgroup] takes the workgroups' sums, and the workgroup with
// the last ticket adds each plane up - lane t the workgroups t, t + 256, ... in that order, then block_sum_all - and returns true
// with the totals in every thread.  The order of the additions belongs to (n, grid), not to the workgroup that comes last.
template <int NQ>
static __device__ __forceinline__ bool grid_totals(const double (&val)[NQ], double* __restrict__ part, uint32_t* ticket, double (&total)[NQ])
{
    __shared__ double s_part[kBlock / kWave];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
    {
        const double t = block_sum_all(val[q], s_part);
        if (threadIdx.x == 0) part[(int64_t)q * gridDim.x + blockIdx.x] = t;
    }
    if (!took_last_ticket(ticket)) return false;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
    {
        double acc = 0.0;
        for (int g = threadIdx.x; g < (int)gridDim.x; g += kBlock) acc += partial_sum_load(part + (int64_t)q * gridDim.x + g);
        total[q] = block_sum_all(acc, s_part);
    }
    return true;
}
}  // namespace spmv
