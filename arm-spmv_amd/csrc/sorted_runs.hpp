// sorted_runs.hpp - what the set-up steps that order entries by a key pair and add up runs of equal keys share (amg.hip: the
// coarse operator; spgemm.hip: the sort path): the scoped owner of a step's device memory, the width of a key, the gather of the
// second stable pass and the marking of run heads.  Device code; every unit that includes it gets kernels of its own.
#pragma once

#include <algorithm>
#include <vector>

#include "common.hpp"

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

// head[k] = 1 where the k-th entry in (I, J) order starts a run, k < nnz;  head[nnz] = 0
__global__ __launch_bounds__(kBlock) void runs_head_kernel(int64_t nnz, const int32_t* __restrict__ order, const int32_t* __restrict__ key_i,
                                                          const int32_t* __restrict__ key_j, int32_t* __restrict__ head)
{
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k <= nnz; k += (int64_t)gridDim.x * kBlock)
    {
        int32_t h = 0;
        if (k < nnz)
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

// device memory of a set-up step: freed, behind the stream, when the step returns however it returns
struct device_pool
{
    spmv_ctx*          ctx;
    const char*        who;
    std::vector<void*> held;
    size_t             bytes = 0;  // asked for so far
    device_pool(spmv_ctx* c, const char* w) : ctx(c), who(w) {}
    device_pool(const device_pool&)            = delete;
    device_pool& operator=(const device_pool&) = delete;
    ~device_pool()
    {
        (void)hipStreamSynchronize(ctx->stream);
        for (void* p : held) (void)hipFree(p);
    }
    template <typename T>
    int get(T*& out, size_t count)
    {
        void* p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess)
        {
            (void)hipGetLastError();
            SPMV_FAIL(SPMV_ERR_ALLOC, "%s: out of device memory for %zu bytes of set-up memory", who, count * sizeof(T));
        }
        held.push_back(p);
        bytes += count * sizeof(T);
        out = (T*)p;
        return SPMV_OK;
    }
    void keep(void* p) { held.erase(std::remove(held.begin(), held.end(), p), held.end()); }  // the caller owns p from here on
};

inline int key_bits(int64_t values)
{
    int bits = 1;
    while (bits < 31 && ((int64_t)1 << bits) < values) ++bits;
    return bits;
}

}  // namespace
}  // namespace spmv
