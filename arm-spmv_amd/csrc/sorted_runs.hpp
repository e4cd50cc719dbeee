// sorted_runs.hpp - what set-up steps share: the scoped owner of a step's device memory, the width of a sort key, and the
// pipeline of sorted_runs.hip from values keyed by a pair (i, j) to CSR with the values of equal keys added up (amg.hip: the
// coarse operator; spgemm.hip: the sort path).  Host declarations only; the kernels live in sorted_runs.hip, once.
#pragma once

#include <algorithm>
#include <vector>

#include "common.hpp"

namespace spmv
{
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

// the runs of equal (i, j) among `total` keyed values; every pointer is device memory of the caller's pool
struct key_runs
{
    int32_t  runs      = 0;        // distinct (i, j)
    int32_t* order     = nullptr;  // [total]    value ids in stable (i, j) order
    int32_t* seg_start = nullptr;  // [runs + 1] where every run starts in `order`; seg_start[runs] = total
    int32_t *run_i = nullptr, *run_j = nullptr;  // [runs]
    int32_t* count_i = nullptr;    // [n_i + 1]  runs per i, count_i[n_i] = 0: ready for exclusive_scan_i32
};

// key_i[total] < n_i, key_j[total] < n_j, 1 <= total <= INT32_MAX.  Asynchronous but for one read of the number of runs.
int runs_by_key_pair(spmv_ctx* ctx, device_pool& pool, const char* who, const int32_t* key_i, int64_t n_i, const int32_t* key_j, int64_t n_j,
                     int64_t total, key_runs* out);

// One lane per run s with i = run_i[s]: at = c_rp[rows ? rows[i] : i] + (s - run_first[i]), c_col[at] = run_j[s], c_val[at] = the sum
// of t[order[k]] over the run, from 0.0, left to right (__dadd_rn).  run_first is the exclusive scan of count_i.  Asynchronous.
int runs_sum_into_csr(spmv_ctx* ctx, const char* who, const key_runs& kr, const double* t, const int32_t* run_first, const int32_t* rows,
                      const int32_t* c_rp, int32_t* c_col, double* c_val);
}  // namespace spmv
