// bsr_settings.hpp - the arithmetic of the block CSR product (kernels_bsr.hip) as plain functions that a host compiler takes too:
// how many lanes a block row gets, how many block rows a wavefront and a workgroup hold, which stored value a lane multiplies,
// whom it adds to in the reduction, and the size of the grid.  tests/bsr_settings_check.cpp walks every one of them with g++.
//
// A block holds bs x bs values, row-major, bs in 2 .. 8.  A wavefront of 64 lanes holds slots = 64 / bs^2 whole blocks at a time
// (16, 7, 4, 2, 1, 1, 1); its first slots * bs^2 lanes are active (64, 63, 64, 50, 36, 49, 64), the others idle.  A block row gets
// g of the slots, g a divisor of `slots`, so lanes = g * bs^2 and a wavefront holds slots / g block rows.  Inside its group lane
// t = q * bs^2 + r * bs + c starts on the block row's q-th block and steps g blocks at a time; it keeps (r, c) for the whole loop:
// the values of one step of a group are lanes * 8 contiguous bytes, read by consecutive lanes.
//
// The reduction is a fixed shift-down tree, first over the bs positions c of a row of the block (lanes 1 apart), then over the g
// blocks of the group (lanes bs^2 apart): at a step of a width w, half h = bsr_half(w), the position p adds the one at p + h where
// p + h < w, and w becomes h.  Every partner holds the same r; the sum of scalar row r ends in the lane with q = 0, c = 0.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SPMV_BSR_HD __host__ __device__
#else
#define SPMV_BSR_HD
#endif

namespace spmv
{
constexpr int kBsrMinBs     = 2;
constexpr int kBsrMaxBs     = 8;
constexpr int kBsrWave      = 64;
constexpr int kBsrWorkgroup = 256;  // four wavefronts

SPMV_BSR_HD constexpr bool bsr_bs_valid(int bs) { return bs >= kBsrMinBs && bs <= kBsrMaxBs; }
SPMV_BSR_HD constexpr int  bsr_slots(int bs) { return kBsrWave / (bs * bs); }              // whole blocks a wavefront holds at a time
SPMV_BSR_HD constexpr int  bsr_active_lanes(int bs) { return bsr_slots(bs) * bs * bs; }    // a multiple of bs^2

// may a block row of blocks of bs get this many lanes?
SPMV_BSR_HD constexpr bool bsr_lanes_valid(int bs, int lanes)
{
    if (!bsr_bs_valid(bs) || lanes <= 0 || lanes % (bs * bs) != 0) return false;
    const int g = lanes / (bs * bs);
    return g <= bsr_slots(bs) && bsr_slots(bs) % g == 0;
}

// The lanes a block row gets, from the mean number of blocks per block row, as the CSR row-parallel kernel picks its lanes per row
// from the mean row: the fewest slots that leave a lane at most kBsrBlocksPerLane blocks of a mean row.  Measured on MI355X
// (tools/bench_bsr.py, "ms_by_lanes"): at 5, 8 and 27 blocks per block row one slot is as fast as any or faster (more block rows
// per wavefront: more independent pointer -> column -> x chains in flight), so only long block rows are shared out further.
constexpr int kBsrStepsInFlight = 4;   // steps a lane has in flight before its first fma (kernels_bsr.hip)
constexpr int kBsrBlocksPerLane = 32;
inline int bsr_pick_lanes(int bs, double mean_blocks)
{
    const int slots = bsr_slots(bs);
    for (int g = 1; g < slots; ++g)
        if (slots % g == 0 && (double)(g * kBsrBlocksPerLane) >= mean_blocks) return g * bs * bs;
    return slots * bs * bs;
}

SPMV_BSR_HD constexpr int bsr_rows_per_wave(int bs, int lanes) { return bsr_slots(bs) / (lanes / (bs * bs)); }
SPMV_BSR_HD constexpr int bsr_rows_per_workgroup(int bs, int lanes) { return (kBsrWorkgroup / kBsrWave) * bsr_rows_per_wave(bs, lanes); }
// workgroups of a product over mb block rows (0: nothing to launch)
inline int64_t bsr_grid(int64_t mb, int bs, int lanes)
{
    const int64_t per = bsr_rows_per_workgroup(bs, lanes);
    return (mb + per - 1) / per;
}

// what lane `lane` (0 .. 63) of a wavefront does
struct bsr_lane
{
    int active;  // 0: the lane idles (64 is no multiple of bs^2)
    int row;     // block row inside the wavefront, 0 .. bsr_rows_per_wave - 1
    int block;   // q: first block inside the block row; the lane then steps lanes / bs^2 blocks at a time
    int r, c;    // position inside the block, for the whole loop
};
SPMV_BSR_HD constexpr bsr_lane bsr_lane_map(int bs, int lanes, int lane)
{
    const int bs2 = bs * bs, g = lanes / bs2, slot = lane / bs2, p = lane % bs2;
    return bsr_lane{slot < bsr_slots(bs) ? 1 : 0, slot / g, slot % g, p / bs, p % bs};
}
// the first block row of wavefront `wave` (0 .. 3) of workgroup `workgroup`
SPMV_BSR_HD constexpr int64_t bsr_first_row(int64_t workgroup, int wave, int bs, int lanes)
{
    return (workgroup * (kBsrWorkgroup / kBsrWave) + wave) * bsr_rows_per_wave(bs, lanes);
}
// offset of the value a lane multiplies at block `b` (64-bit: nnzb * bs^2 may pass INT32_MAX)
SPMV_BSR_HD constexpr int64_t bsr_value_offset(int64_t b, int bs, int r, int c) { return b * (bs * bs) + r * bs + c; }

// ---- the reduction ---------------------------------------------------------------------------------------------------------------
SPMV_BSR_HD constexpr int bsr_half(int w) { return (w + 1) / 2; }
SPMV_BSR_HD constexpr int bsr_tree_steps(int w)
{
    int n = 0;
    for (; w > 1; w = bsr_half(w)) ++n;
    return n;
}
SPMV_BSR_HD constexpr int bsr_reduce_steps(int bs, int lanes) { return bsr_tree_steps(bs) + bsr_tree_steps(lanes / (bs * bs)); }
// the lane whose sum `lane` adds at step `step` (0 .. bsr_reduce_steps - 1), -1: none at this step
SPMV_BSR_HD constexpr int bsr_reduce_partner(int bs, int lanes, int lane, int step)
{
    const bsr_lane L = bsr_lane_map(bs, lanes, lane);
    if (!L.active) return -1;
    const int over_c = bsr_tree_steps(bs);
    int       w = step < over_c ? bs : lanes / (bs * bs), s = step < over_c ? step : step - over_c;
    const int pos = step < over_c ? L.c : L.block, unit = step < over_c ? 1 : bs * bs;
    for (; s > 0; --s) w = bsr_half(w);
    const int h = bsr_half(w);
    return w > 1 && pos + h < w ? lane + h * unit : -1;
}
}  // namespace spmv
