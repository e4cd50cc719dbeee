// The host arithmetic of csrc/reorder_settings.hpp held to its properties (compiled with g++ by tests/test_reorder_abi.py).
#include <cstdio>

#include "reorder_settings.hpp"

int main()
{
    using namespace spmv;
    int bad = 0, last = 0, checked = 0;
    for (double mean = 0.0; mean <= 4096.0; mean += 0.25, ++checked)
    {
        const int l = rcm_lanes(mean);
        if (l != 4 && l != 16 && l != 64) ++bad;                     // a group divides a wavefront
        if (l < last) ++bad;                                          // monotone in the mean degree
        if (l > 4 && mean <= l / 2.0) ++bad;                          // more than a neighbour for every second lane, or the smaller group
        if (l < 64 && mean > 2.0 * l) ++bad;                          // at most two neighbours a lane below the widest group
        last = l;
    }
    if (rcm_lanes(1.0) != 4 || rcm_lanes(8.0) != 4 || rcm_lanes(8.5) != 16 || rcm_lanes(32.0) != 16 || rcm_lanes(33.0) != 64) ++bad;
    if (kRcmRootRepeats != 8) ++bad;
    if (kRcmSmallLevel < 256 || kRcmSmallLevel * 12 > 64 * 1024) ++bad;  // 12 bytes of LDS a vertex, within a workgroup's 64 KiB
    std::printf("%d mean degrees, %d violations\n", checked, bad);
    return bad ? 1 : 0;
}
