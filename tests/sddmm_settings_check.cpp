// Properties of csrc/sddmm_settings.hpp, checked exhaustively on the host (tests/test_sddmm_settings.py compiles and runs this):
// for every k = 1 .. 64 and entry counts around every boundary of a run and of a grid trip, the loops of kernels_sddmm.hip - runs dealt
// to the wavefronts of the capped grid, chunks of 64, groups of L lanes, steps - give every entry to exactly one (group, step), keep it
// in exactly the lane that stores it, give every column c < k to exactly one lane of the group, and mask only lanes with c >= k.
#include <cstdio>
#include <vector>

#include "sddmm_settings.hpp"

using namespace spmv;

static long violations = 0;
#define CHECK(cond, ...)                      \
    do                                        \
    {                                         \
        if (!(cond))                          \
        {                                     \
            if (++violations <= 20)           \
            {                                 \
                std::printf("VIOLATION: ");   \
                std::printf(__VA_ARGS__);     \
                std::printf("\n");            \
            }                                 \
        }                                     \
    } while (0)

// the kernel's loops over `nnz` entries with a grid capped at `cap` workgroups
static void walk(int k, int64_t nnz, int cap)
{
    const int     L     = sddmm_lanes(k);
    const int     B     = sddmm_batch(L);
    const int64_t nruns = sddmm_runs(nnz);
    const int     grid  = sddmm_grid(nruns, cap);
    const int64_t waves = (int64_t)grid * sddmm_waves_per_block();
    std::vector<unsigned char> made((size_t)nnz, 0), stored((size_t)nnz, 0);
    CHECK(L % B == 0 && B >= 1, "k %d: batch %d does not divide %d lanes", k, B, L);
    for (int64_t w = 0; w < waves; ++w)
        for (int64_t run = w; run < nruns; run += waves)
        {
            const int64_t e0 = sddmm_run_begin(run), e1 = sddmm_run_end(run, nnz);
            CHECK(e0 < e1 && e1 <= nnz && e1 - e0 <= kSddmmRun, "run %lld of %lld entries: [%lld, %lld)", (long long)run, (long long)nnz,
                  (long long)e0, (long long)e1);
            const int64_t stride = k == 1 ? (int64_t)kSddmmK1Depth * kSddmmChunk : kSddmmChunk;
            for (int64_t c0 = e0; c0 < e1; c0 += stride)
                for (int q = 0; q < (k == 1 ? kSddmmK1Depth : 1); ++q)
                {
                    const int64_t c = c0 + (int64_t)q * kSddmmChunk;
                    for (int lane = 0; lane < kSddmmWave; ++lane)  // the loads and the store of a chunk: lane l entry c + l
                        if (c + lane < e1) ++stored[(size_t)(c + lane)];
                    for (int g = 0; g < sddmm_groups(L); ++g)
                        for (int b = 0; b < L; b += B)
                            for (int i = 0; i < B; ++i)
                            {
                                const int slot = sddmm_slot(g, b + i, L);
                                if (c + slot >= e1) continue;
                                ++made[(size_t)(c + slot)];
                                const int keeper = sddmm_keeper(g, b + i, L);
                                CHECK(keeper == slot && sddmm_group_of_lane(keeper, L) == g && sddmm_column_of_lane(keeper, L) == b + i,
                                      "k %d: entry slot %d kept by lane %d", k, slot, keeper);
                            }
                }
        }
    for (int64_t e = 0; e < nnz; ++e)
        CHECK(made[(size_t)e] == 1 && stored[(size_t)e] == 1, "k %d nnz %lld cap %d: entry %lld made %d times, stored %d times", k,
              (long long)nnz, cap, (long long)e, made[(size_t)e], stored[(size_t)e]);
}

int main()
{
    int lane_classes = 0;
    for (int k = 1; k <= kSddmmMaxK; ++k)
    {
        const int L = sddmm_lanes(k);
        CHECK(L >= k && (L & (L - 1)) == 0 && (L == 1 || L / 2 < k) && kSddmmWave % L == 0, "k %d: %d lanes", k, L);
        if (k == L) ++lane_classes;
        // columns: every c < k owned by exactly one lane of every group, every masked lane has c >= k
        for (int g = 0; g < sddmm_groups(L); ++g)
        {
            int owners[kSddmmMaxK] = {0};
            for (int lane = g * L; lane < (g + 1) * L; ++lane)
            {
                CHECK(sddmm_group_of_lane(lane, L) == g, "k %d: lane %d in group %d", k, lane, sddmm_group_of_lane(lane, L));
                const int c = sddmm_column_of_lane(lane, L);
                if (sddmm_lane_live(lane, L, k))
                {
                    CHECK(c < k, "k %d: live lane %d owns column %d", k, lane, c);
                    ++owners[c];
                }
                else
                    CHECK(c >= k, "k %d: masked lane %d owns column %d", k, lane, c);
            }
            for (int c = 0; c < k; ++c) CHECK(owners[c] == 1, "k %d group %d: column %d has %d owners", k, g, c, owners[c]);
        }
        // entries: around every boundary of a run, and around the end of a trip of a small grid (cap 2: 8 wavefronts)
        const int     cap  = 2;
        const int64_t trip = sddmm_trip_entries(cap);
        CHECK(trip == (int64_t)cap * sddmm_waves_per_block() * kSddmmRun, "trip of %lld entries", (long long)trip);
        const int64_t sizes[] = {1, 2, kSddmmChunk - 1, kSddmmChunk, kSddmmChunk + 1, kSddmmRun - 1, kSddmmRun, kSddmmRun + 1,
                                 2 * kSddmmRun + 1, trip - 1, trip, trip + 1, trip + kSddmmRun + 3, 2 * trip + 65};
        for (int64_t nnz : sizes) walk(k, nnz, cap);
        walk(k, 3 * kSddmmRun + 7, kSddmmMaxGrid);
    }
    CHECK(sddmm_grid(0, kSddmmMaxGrid) == 1 && sddmm_grid(1, kSddmmMaxGrid) == 1, "grid of an empty launch");
    CHECK(sddmm_grid(sddmm_runs(sddmm_trip_entries(kSddmmMaxGrid)), kSddmmMaxGrid) == kSddmmMaxGrid &&
              sddmm_grid(sddmm_runs(sddmm_trip_entries(kSddmmMaxGrid) + 1), kSddmmMaxGrid) == kSddmmMaxGrid,
          "the grid cap");
    CHECK(sddmm_runs(2147483647LL) * kSddmmRun >= 2147483647LL, "runs of the largest int32 pattern");
    std::printf("%d lane classes, run %d, cap %d, trip %lld, k up to %d: %ld violations\n", lane_classes, kSddmmRun, kSddmmMaxGrid,
                (long long)sddmm_trip_entries(kSddmmMaxGrid), kSddmmMaxK, violations);
    return violations ? 1 : 0;
}
