// Pure host arithmetic of the reverse Cuthill-McKee ordering (reorder.hip): no HIP, no state.  tests/rcm_ref.py, the NumPy twin of
// the ordering, reads kRcmRootRepeats from this file.
#pragma once
#include <cstdint>

namespace spmv
{
// George and Liu's root rule is applied at most this many times per component
constexpr int kRcmRootRepeats = 8;
// a level of at most this many vertices is ordered by one workgroup in LDS; a larger one by two stable radix passes
constexpr int kRcmSmallLevel = 1024;

// lanes that share a frontier vertex in the breadth-first kernels: 4 up to a mean degree of 8, 16 up to 32, 64 beyond - between half
// a neighbour and two neighbours a lane at the mean degree of the vertices that have neighbours
constexpr int rcm_lanes(double mean_degree)
{
    int lanes = 4;
    while (lanes < 64 && lanes * 2 < mean_degree) lanes *= 4;
    return lanes;
}
}  // namespace spmv
