// Properties of arm-spmv_amd/csrc/fsai_settings.hpp (spmv_fsai_setup: the lanes, the LDS and the packed-triangle offsets of the row
// kernel).  Compiled and run by tests/test_fsai_settings.py; prints one summary line.
//   * the class of m is total and monotone; for 1 <= m <= 64 its lanes L are the smallest of 4, 8, 16, 32, 64 with L >= m, and
//     every m beyond the cap gets no class;
//   * L divides a wavefront, so a group never straddles one; a workgroup's lanes are a whole number of wavefronts, at most 256;
//   * a group's LDS holds the packed triangle of L rows, L doubles and L int32; at most 2080 doubles of triangle go to a 64-lane
//     group; a workgroup's LDS fits the 64 KiB it may declare and at least two workgroups fit the CU's 160 KiB;
//   * the packed offsets are those of rows laid end to end: (p, q) -> p (p + 1) / 2 + q is a bijection from the lower triangle of
//     m rows onto 0 .. m (m + 1) / 2 - 1, checked by enumeration for every m up to the cap, and they are 64-bit: no wrap for any
//     int32 p.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "fsai_settings.hpp"

int main()
{
    using namespace spmv;
    long long bad = 0, checked = 0;
    int       prev = 0, edges = 0;
    for (int64_t m = -3; m <= 4 * kFsaiMaxRow; ++m)
    {
        const int c = fsai_class_of(m);
        ++checked;
        if (c < 0 || c > kFsaiClasses || c < prev) ++bad;
        if ((c == kFsaiClasses) != (m > kFsaiMaxRow)) ++bad;
        if (c < kFsaiClasses)
        {
            const int L = fsai_lanes(c);
            if (L < m || (c > 0 && fsai_lanes(c - 1) >= m) || L < kFsaiMinLanes || L > kFsaiMaxRow) ++bad;
        }
        if (c != prev) ++edges;
        prev = c;
    }
    for (int64_t m : {(int64_t)1 << 31, (int64_t)1 << 40, INT64_MAX})
        if (fsai_class_of(m) != kFsaiClasses) ++bad;
    if (fsai_class_of(INT64_MIN) != 0 || fsai_class_of(1) != 0 || fsai_class_of(4) != 0 || fsai_class_of(5) != 1 || fsai_class_of(64) != 4) ++bad;
    if (fsai_lanes(kFsaiClasses - 1) != kFsaiMaxRow || kFsaiMaxRow != kFsaiWave) ++bad;
    for (int c = 0; c < kFsaiClasses; ++c)
    {
        const int L = fsai_lanes(c), G = fsai_groups_per_block(L);
        if (kFsaiWave % L || (L & (L - 1))) ++bad;
        if (G < 1 || G * L > kFsaiBlockLanes || (G * L) % kFsaiWave || fsai_block_lanes(L) != G * L) ++bad;
        if (fsai_group_doubles(L) != L * (L + 1) / 2 + L + L / 2 || fsai_tri(L) > 2080) ++bad;
        if (fsai_block_lds_bytes(L) != G * fsai_group_doubles(L) * 8 || fsai_block_lds_bytes(L) > kFsaiLdsPerBlock) ++bad;
        if (fsai_blocks_per_cu(L) < 2 || fsai_blocks_per_cu(L) * fsai_block_lds_bytes(L) > kFsaiLdsPerCu) ++bad;
        // (one group more would not fit, or would not be whole wavefronts, or would pass 256 lanes)
        const int more = G + 1;
        if (more * L <= kFsaiBlockLanes && (more * L) % kFsaiWave == 0 && more * fsai_group_doubles(L) * 8 <= kFsaiLdsPerBlock) ++bad;
    }
    if (fsai_tri(kFsaiMaxRow) != 2080 || fsai_groups_per_block(64) != 3 || fsai_groups_per_block(4) != 64) ++bad;
    // the packed triangle, by enumeration
    for (int m = 1; m <= kFsaiMaxRow; ++m)
    {
        std::vector<int> seen((size_t)fsai_tri(m), 0);
        for (int p = 0; p < m; ++p)
            for (int q = 0; q <= p; ++q)
            {
                const int64_t at = fsai_tri_at(p, q);
                ++checked;
                if (at < 0 || at >= fsai_tri(m) || seen[(size_t)at]++) ++bad;
            }
        for (int v : seen)
            if (v != 1) ++bad;
    }
    if (fsai_tri(INT32_MAX) != (int64_t)INT32_MAX * ((int64_t)INT32_MAX + 1) / 2 || fsai_tri_at(INT32_MAX, INT32_MAX) <= fsai_tri(INT32_MAX)) ++bad;
    std::printf("fsai_settings: %lld values checked, %d class edges, cap %d, %lld violations\n", checked, edges, kFsaiMaxRow, bad);
    return bad ? 1 : 0;
}
