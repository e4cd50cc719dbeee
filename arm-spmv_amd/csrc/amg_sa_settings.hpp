// Pure host arithmetic of the smoothed-aggregation cycle's two fused kernels (amg.hip: amg_restrict_csr_kernel,
// amg_prolong_csr_kernel): no HIP, no state, so that tests/test_amg_sa_settings.py can compile it with g++
// (tests/amg_sa_settings_check.cpp).
//
// A group of g = 2^k lanes, 1 <= g <= 64, serves one row of R or P.  g is chosen per level and per operator at set-up from the
// operator's mean row length: the largest power of two not above HALF the mean, so that every lane of a group has about two
// entries or more to stream before the reduction tree, clamped to 1 .. 64.  In integers: the largest g with 2 g nrow <= nnz.
// DESIGN.md 20 holds the measurement behind the rule.
#pragma once
#include <cstdint>

namespace spmv
{
constexpr int kAmgSaMaxLanes = 64;

// nnz >= 0 stored entries in nrow >= 0 rows; an empty operator takes one lane a row
constexpr int amg_sa_group_lanes(int64_t nnz, int64_t nrow)
{
    int g = 1;
    while (g < kAmgSaMaxLanes && nrow > 0 && 4 * (int64_t)g * nrow <= nnz) g <<= 1;  // (2 g is the candidate: 2 (2 g) nrow <= nnz)
    return g;
}

// rows a workgroup of `block` lanes serves at once
constexpr int amg_sa_rows_per_block(int block, int g) { return block / g; }
}  // namespace spmv
