// bsr_settings_check.cpp - csrc/bsr_settings.hpp walked on the host (g++, no GPU): for every block size 2 .. 8 and every number
// of lanes per block row the header can return
//   * the lane map covers every stored value of a block row exactly once, for block rows of 0 .. 3 * slots + 1 blocks, through the
//     loop the kernel runs (start at the lane's block, step lanes / bs^2 blocks), consecutive lanes on consecutive values;
//   * a lane keeps its (r, c);
//   * the reduction's partners hold the same r, are active lanes of the same block row, and the tree leaves the sum of every
//     scalar row - each lane's accumulator counted once - in the lane with block 0, c 0;
//   * the grid covers mb block rows for mb in 0 .. 1000, no block row twice.
// Prints "<checks> checks, <n> violations".
#include <cstdio>
#include <set>
#include <vector>

#include "bsr_settings.hpp"

using namespace spmv;

static long checks = 0, violations = 0;
#define CHECK(cond, ...)               \
    do                                 \
    {                                  \
        ++checks;                      \
        if (!(cond))                   \
        {                              \
            ++violations;              \
            if (violations < 20)       \
            {                          \
                printf("VIOLATION: "); \
                printf(__VA_ARGS__);   \
                printf("\n");          \
            }                          \
        }                              \
    } while (0)

static std::vector<int> lanes_of(int bs)
{
    std::set<int> s;
    for (int tenth = 0; tenth <= 6000; ++tenth) s.insert(bsr_pick_lanes(bs, tenth / 10.0));  // every mean from 0 to 600 blocks
    s.insert(bsr_pick_lanes(bs, 1e9));
    for (int lanes = 1; lanes <= kBsrWave; ++lanes)
        if (bsr_lanes_valid(bs, lanes)) s.insert(lanes);
    return std::vector<int>(s.begin(), s.end());
}

int main()
{
    const int want_active[9] = {0, 0, 64, 63, 64, 50, 36, 49, 64};
    for (int bs : {0, 1, 9, -1}) CHECK(!bsr_bs_valid(bs) && !bsr_lanes_valid(bs, 64), "bs %d taken", bs);
    for (int bs = kBsrMinBs; bs <= kBsrMaxBs; ++bs)
    {
        const int bs2 = bs * bs;
        CHECK(bsr_active_lanes(bs) == want_active[bs], "bs %d: %d active lanes", bs, bsr_active_lanes(bs));
        CHECK(bsr_pick_lanes(bs, 0.0) == bs2 && bsr_pick_lanes(bs, 1e9) == bsr_active_lanes(bs), "bs %d: the smallest and the largest pick", bs);
        int before = 0;
        for (int tenth = 0; tenth <= 6000; ++tenth)
        {
            const int lanes = bsr_pick_lanes(bs, tenth / 10.0);
            CHECK(bsr_lanes_valid(bs, lanes) && lanes >= before, "bs %d mean %.1f: %d lanes", bs, tenth / 10.0, lanes);
            CHECK(lanes / bs2 * kBsrBlocksPerLane >= tenth / 10.0 || lanes == bsr_active_lanes(bs), "bs %d mean %.1f: %d lanes leave a lane more than %d blocks", bs, tenth / 10.0, lanes, kBsrBlocksPerLane);
            before = lanes;
        }
        for (int lanes : lanes_of(bs))
        {
            CHECK(bsr_lanes_valid(bs, lanes), "bs %d: %d lanes not valid", bs, lanes);
            const int g = lanes / bs2, rpw = bsr_rows_per_wave(bs, lanes);
            CHECK(rpw >= 1 && rpw * lanes == bsr_active_lanes(bs), "bs %d lanes %d: %d block rows per wavefront", bs, lanes, rpw);
            CHECK(bsr_rows_per_workgroup(bs, lanes) == 4 * rpw, "bs %d lanes %d: rows per workgroup", bs, lanes);
            // ---- the lane map --------------------------------------------------------------------------------------------------
            int active = 0;
            for (int lane = 0; lane < kBsrWave; ++lane)
            {
                const bsr_lane L = bsr_lane_map(bs, lanes, lane);
                if (!L.active) continue;
                ++active;
                CHECK(L.row >= 0 && L.row < rpw && L.block >= 0 && L.block < g && L.r >= 0 && L.r < bs && L.c >= 0 && L.c < bs, "bs %d lanes %d lane %d: out of range", bs,
                      lanes, lane);
                CHECK(lane == L.row * lanes + L.block * bs2 + L.r * bs + L.c, "bs %d lanes %d lane %d: not where the map says", bs, lanes, lane);
            }
            CHECK(active == bsr_active_lanes(bs), "bs %d lanes %d: %d active lanes", bs, lanes, active);
            for (int nblocks = 0; nblocks <= 3 * bsr_slots(bs) + 1; ++nblocks)
                for (int row = 0; row < rpw; ++row)
                {
                    std::vector<int> hits((size_t)nblocks * bs2, 0);
                    for (int lane = 0; lane < kBsrWave; ++lane)
                    {
                        const bsr_lane L = bsr_lane_map(bs, lanes, lane);
                        if (!L.active || L.row != row) continue;
                        int step = 0;
                        for (int b = L.block; b < nblocks; b += g, ++step)
                        {
                            const int64_t at = bsr_value_offset(b, bs, L.r, L.c);
                            CHECK(at >= 0 && at < (int64_t)hits.size(), "bs %d lanes %d lane %d: offset %lld of %zu", bs, lanes, lane, (long long)at, hits.size());
                            if (at >= 0 && at < (int64_t)hits.size()) ++hits[(size_t)at];
                            // consecutive lanes of the group read consecutive values: one contiguous run per step
                            CHECK(at == (int64_t)step * lanes + (lane - row * lanes), "bs %d lanes %d lane %d step %d: offset %lld breaks the run", bs, lanes, lane, step,
                                  (long long)at);
                        }
                    }
                    for (size_t at = 0; at < hits.size(); ++at) CHECK(hits[at] == 1, "bs %d lanes %d, %d blocks: value %zu read %d times", bs, lanes, nblocks, at, hits[at]);
                }
            CHECK(bsr_value_offset(((int64_t)1 << 31) - 65537, 8, 7, 7) == (((int64_t)1 << 31) - 65537) * 64 + 63, "64-bit value offsets");
            // ---- the reduction: accumulators as bit sets of the lanes they hold -----------------------------------------------------
            const int steps = bsr_reduce_steps(bs, lanes);
            std::vector<unsigned long long> acc(kBsrWave);
            for (int lane = 0; lane < kBsrWave; ++lane) acc[lane] = 1ull << lane;
            for (int step = 0; step < steps; ++step)
            {
                const std::vector<unsigned long long> in = acc;  // every lane reads its partner's value of before the step
                for (int lane = 0; lane < kBsrWave; ++lane)
                {
                    const int p = bsr_reduce_partner(bs, lanes, lane, step);
                    if (p < 0) continue;
                    const bsr_lane L = bsr_lane_map(bs, lanes, lane);
                    CHECK(p > lane && p < kBsrWave, "bs %d lanes %d lane %d step %d: partner %d", bs, lanes, lane, step, p);
                    if (p <= lane || p >= kBsrWave) continue;
                    const bsr_lane P = bsr_lane_map(bs, lanes, p);
                    CHECK(P.active && P.r == L.r && P.row == L.row, "bs %d lanes %d lane %d step %d: partner %d holds another row", bs, lanes, lane, step, p);
                    CHECK((in[lane] & in[p]) == 0, "bs %d lanes %d lane %d step %d: a sum counted twice", bs, lanes, lane, step);
                    acc[lane] = in[lane] | in[p];
                }
            }
            for (int lane = 0; lane < kBsrWave; ++lane)
            {
                const bsr_lane L = bsr_lane_map(bs, lanes, lane);
                if (!L.active || L.block != 0 || L.c != 0) continue;
                unsigned long long want = 0;
                for (int other = 0; other < kBsrWave; ++other)
                {
                    const bsr_lane O = bsr_lane_map(bs, lanes, other);
                    if (O.active && O.row == L.row && O.r == L.r) want |= 1ull << other;
                }
                CHECK(acc[lane] == want, "bs %d lanes %d lane %d: the tree leaves %llx, the row is %llx", bs, lanes, lane, acc[lane], want);
            }
            // ---- the grid ------------------------------------------------------------------------------------------------------------
            for (int64_t mb = 0; mb <= 1000; ++mb)
            {
                const int64_t grid = bsr_grid(mb, bs, lanes), per = bsr_rows_per_workgroup(bs, lanes);
                CHECK(grid * per >= mb && (grid == 0 || (grid - 1) * per < mb), "bs %d lanes %d: %lld workgroups for %lld block rows", bs, lanes, (long long)grid,
                      (long long)mb);
                if (mb % 97 == 0 || mb < 40)
                {
                    std::vector<int> seen((size_t)mb, 0);
                    for (int64_t w = 0; w < grid; ++w)
                        for (int wave = 0; wave < 4; ++wave)
                            for (int row = 0; row < rpw; ++row)
                            {
                                const int64_t br = bsr_first_row(w, wave, bs, lanes) + row;
                                if (br < mb) ++seen[(size_t)br];
                            }
                    for (int64_t br = 0; br < mb; ++br) CHECK(seen[(size_t)br] == 1, "bs %d lanes %d mb %lld: block row %lld taken %d times", bs, lanes, (long long)mb, (long long)br, seen[(size_t)br]);
                }
            }
        }
    }
    printf("%ld checks, %ld violations\n", checks, violations);
    return violations ? 1 : 0;
}
