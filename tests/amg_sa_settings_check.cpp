// Properties of arm-spmv_amd/csrc/amg_sa_settings.hpp (the lanes a row of R or P takes in the smoothed-aggregation cycle).
// Compiled and run by tests/test_amg_sa_settings.py; prints one summary line.
//   * for every nrow in 1 .. 300 and every nnz in 0 .. 140 nrow, and for the same ratios at rows in the millions and at the
//     largest int32 sizes: g is a power of two in 1 .. 64, it is the LARGEST power of two with 2 g nrow <= nnz (half the mean row
//     length) or 1 where there is none, it does not decrease in nnz, and it depends on the ratio alone (k nnz, k nrow);
//   * nrow = 0 and nnz = 0 take one lane;
//   * the row lengths DESIGN.md 20 names land where it says: R of 23 - 25 entries a row 8 lanes, 57 entries 16, 68 - 75 entries 32,
//     371 - 453 entries 64; P of 4 - 7 entries 2 lanes, 8 - 11 entries 4;
//   * a workgroup of 256 lanes serves a whole number of rows under every g.
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include "amg_sa_settings.hpp"

static bool is_rule(int g, int64_t nnz, int64_t nrow)
{
    if (g < 1 || g > spmv::kAmgSaMaxLanes || (g & (g - 1))) return false;
    const bool fits = g == 1 || 2 * (int64_t)g * nrow <= nnz;                                // g itself is not above half the mean
    const bool last = g == spmv::kAmgSaMaxLanes || nrow == 0 || 2 * (int64_t)(2 * g) * nrow > nnz;  // and 2 g is
    return fits && last;
}

int main()
{
    using namespace spmv;
    long long bad = 0, checked = 0;
    for (int64_t nrow = 1; nrow <= 300; ++nrow)
    {
        int prev = 1;
        for (int64_t nnz = 0; nnz <= 140 * nrow; ++nnz)
        {
            const int g = amg_sa_group_lanes(nnz, nrow);
            ++checked;
            if (!is_rule(g, nnz, nrow) || g < prev) ++bad;
            for (int64_t k : {(int64_t)7, (int64_t)4096, (int64_t)51001})
                if (amg_sa_group_lanes(k * nnz, k * nrow) != g) ++bad;
            prev = g;
        }
    }
    for (int64_t nrow : {(int64_t)1, (int64_t)1048579, (int64_t)INT32_MAX})
        for (int64_t nnz : {(int64_t)0, (int64_t)1, (int64_t)INT32_MAX - 65536, (int64_t)INT32_MAX})
        {
            ++checked;
            if (!is_rule(amg_sa_group_lanes(nnz, nrow), nnz, nrow)) ++bad;
        }
    if (amg_sa_group_lanes(0, 0) != 1 || amg_sa_group_lanes(100, 0) != 1 || amg_sa_group_lanes(0, 100) != 1) ++bad;
    int named = 0;
    const int64_t rows = 1000;
    for (int64_t len = 23; len <= 25; ++len, ++named)
        if (amg_sa_group_lanes(len * rows, rows) != 8) ++bad;
    if (++named, amg_sa_group_lanes(57 * rows, rows) != 16) ++bad;
    for (int64_t len = 68; len <= 75; ++len, ++named)
        if (amg_sa_group_lanes(len * rows, rows) != 32) ++bad;
    for (int64_t len = 371; len <= 453; ++len, ++named)
        if (amg_sa_group_lanes(len * rows, rows) != 64) ++bad;
    for (int64_t len = 4; len <= 11; ++len, ++named)
        if (amg_sa_group_lanes(len * rows, rows) != (len < 8 ? 2 : 4)) ++bad;
    for (int g = 1; g <= kAmgSaMaxLanes; g <<= 1)
        if (amg_sa_rows_per_block(256, g) * g != 256) ++bad;
    std::printf("amg_sa_settings: %lld pairs (nnz, nrow), %d named row lengths, %lld violations\n", checked, named, bad);
    return bad ? 1 : 0;
}
