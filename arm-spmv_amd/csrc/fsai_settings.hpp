// Pure host arithmetic of the FSAI row kernel (fsai.hip): no HIP, no state, so that tests/test_fsai_settings.py can compile it with
// g++ (tests/fsai_settings_check.cpp).
//
// Row i of G comes from the dense system of its m pattern columns, m <= kFsaiMaxRow.  A row is owned by a group of L lanes, L the
// smallest of 4, 8, 16, 32, 64 with L >= m; a group never straddles a wavefront.  In LDS a group keeps the packed lower triangle of
// its matrix (row p at p (p + 1) / 2, room for L rows), the solution vector (L doubles) and the L pattern columns (int32: L / 2
// doubles).  A workgroup holds as many groups as 256 lanes give, but no more than fit kFsaiLdsPerBlock, the 64 KiB a workgroup may
// declare statically; its lanes stay a whole number of wavefronts.  fsai_blocks_per_cu is what the CU's 160 KiB then hold.
#pragma once
#include <cstdint>

namespace spmv
{
constexpr int kFsaiMaxRow      = 64;  // the cap on m: a wavefront's lanes
constexpr int kFsaiClasses     = 5;   // L = 4 << class
constexpr int kFsaiMinLanes    = 4;
constexpr int kFsaiBlockLanes  = 256;
constexpr int kFsaiWave        = 64;
constexpr int kFsaiLdsPerCu    = 160 * 1024;
constexpr int kFsaiLdsPerBlock = 64 * 1024;

// the class of a row of m pattern columns: 0 .. 4 for 1 <= m <= 64, kFsaiClasses (no kernel) beyond the cap; m <= 0 counts as 1
constexpr int fsai_class_of(int64_t m)
{
    int c = 0;
    while (c < kFsaiClasses && ((int64_t)kFsaiMinLanes << c) < m) ++c;
    return c;
}
constexpr int fsai_lanes(int cls) { return kFsaiMinLanes << cls; }
// packed lower triangle, rows first: where row p starts, and entry (p, q), q <= p; 64-bit, so that no caller's index wraps
constexpr int64_t fsai_tri(int64_t p) { return p * (p + 1) / 2; }
constexpr int64_t fsai_tri_at(int64_t p, int64_t q) { return fsai_tri(p) + q; }
// doubles of LDS a group of L lanes takes: triangle, solution, columns
constexpr int fsai_group_doubles(int lanes) { return (int)fsai_tri(lanes) + lanes + lanes / 2; }
constexpr int fsai_groups_per_block(int lanes)
{
    int g = kFsaiBlockLanes / lanes;
    while (g > 1 && g * fsai_group_doubles(lanes) * 8 > kFsaiLdsPerBlock) --g;
    while (g > 1 && (g * lanes) % kFsaiWave) --g;  // (a whole number of wavefronts)
    return g;
}
constexpr int fsai_block_lanes(int lanes) { return fsai_groups_per_block(lanes) * lanes; }
constexpr int fsai_block_lds_bytes(int lanes) { return fsai_groups_per_block(lanes) * fsai_group_doubles(lanes) * 8; }
constexpr int fsai_blocks_per_cu(int lanes) { return kFsaiLdsPerCu / fsai_block_lds_bytes(lanes); }
}  // namespace spmv
