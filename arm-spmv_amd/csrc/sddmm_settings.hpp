// Pure host arithmetic of the sampled dense-dense product (kernels_sddmm.hip): no HIP, no state, so that tests/test_sddmm_settings.py
// can compile it with g++ (tests/sddmm_settings_check.cpp).
//
// The stored entries 0 .. nnz of a CSR pattern are cut into RUNS of kSddmmRun entries, whatever rows they belong to.  A wavefront
// takes a run, and walks it in CHUNKS of kSddmmChunk = 64 entries: lane l of the wavefront loads and stores entry chunk + l (column
// index in, value out: both coalesced).  The k products of one entry are made by a GROUP of L = sddmm_lanes(k) lanes, L the next
// power of two >= k: lane t of a group owns column t and is masked for t >= k.  Group g of the 64 / L groups of a wavefront makes the
// entries chunk + g L + i, i = 0 .. L, one after the other, so that after the butterfly sum of step i the group's lane i keeps the
// finished sum of exactly the entry it stores.  The gathers of sddmm_batch(L) steps are issued before their multiplies.
// Runs are dealt to the wavefronts of a capped grid, run w + j * (wavefronts of the grid).
#pragma once
#include <cstdint>

namespace spmv
{
constexpr int kSddmmMaxK    = 64;         // columns per call (spmv_apply_multi's limit)
constexpr int kSddmmWave    = 64;         // lanes of a wavefront
constexpr int kSddmmChunk   = 64;         // entries a wavefront loads and stores at once: one per lane
constexpr int kSddmmRun     = 512;        // entries a wavefront takes before it looks for its rows again
constexpr int kSddmmBlock   = 256;        // lanes of a workgroup
constexpr int kSddmmMaxGrid = 256 * 4;    // workgroups per launch: four per CU; more runs than that loop
constexpr int kSddmmK1Depth = 4;          // k = 1: chunks whose loads are in flight together

constexpr int sddmm_waves_per_block() { return kSddmmBlock / kSddmmWave; }
// lanes of the group that makes one entry: the next power of two >= k (1 .. 64)
constexpr int sddmm_lanes(int k)
{
    int l = 1;
    while (l < k && l < kSddmmWave) l *= 2;
    return l;
}
constexpr int sddmm_groups(int lanes) { return kSddmmWave / lanes; }
// steps of a group whose gathers are in flight before their multiplies
constexpr int sddmm_batch(int lanes) { return lanes < 8 ? lanes : lanes < 32 ? 8 : 16; }
// the lane of a wavefront: its group, and the column it owns there
constexpr int  sddmm_group_of_lane(int lane, int lanes) { return lane / lanes; }
constexpr int  sddmm_column_of_lane(int lane, int lanes) { return lane % lanes; }
constexpr bool sddmm_lane_live(int lane, int lanes, int k) { return sddmm_column_of_lane(lane, lanes) < k; }
// the entry of a chunk (0 .. 64) that group g makes at step i, and the lane of the wavefront that keeps and stores it
constexpr int sddmm_slot(int group, int step, int lanes) { return group * lanes + step; }
constexpr int sddmm_keeper(int group, int step, int lanes) { return group * lanes + step; }

constexpr int64_t sddmm_runs(int64_t nnz) { return (nnz + kSddmmRun - 1) / kSddmmRun; }
constexpr int64_t sddmm_run_begin(int64_t run) { return run * kSddmmRun; }
constexpr int64_t sddmm_run_end(int64_t run, int64_t nnz) { return (run + 1) * kSddmmRun < nnz ? (run + 1) * kSddmmRun : nnz; }
// workgroups of a launch over `runs` runs with `cap` as the limit (kSddmmMaxGrid in the engine)
constexpr int sddmm_grid(int64_t runs, int cap)
{
    const int64_t want = (runs + sddmm_waves_per_block() - 1) / sddmm_waves_per_block();
    return (int)(want < 1 ? 1 : want < cap ? want : cap);
}
// entries one trip of a full grid covers: beyond these a wavefront takes a second run
constexpr int64_t sddmm_trip_entries(int cap) { return (int64_t)cap * sddmm_waves_per_block() * kSddmmRun; }
}  // namespace spmv
