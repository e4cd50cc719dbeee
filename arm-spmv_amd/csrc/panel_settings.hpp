// Pure host arithmetic of the panel kernel's launch settings (kernels_csr_panel.hip: panel_launch; plan.hip: collect): no HIP, no
// state, so that tests/test_abi_and_host.py can compile it with g++ and walk every request (tests/panel_settings_check.cpp).
#pragma once
#include <algorithm>

namespace spmv
{
// what a panel launch runs: chunks of `unroll` x 1024 entries (2, 4, 8), the order `pipe` of a chunk's loads (0 off, 1 stream-first,
// 2 gather-first), the barrier `sync` that keeps a workgroup's wavefronts together (0 none, 1 per chunk, 3 between a chunk's loads
// and its LDS adds).  These are the instantiated combinations: panel_launch finds a kernel for every result.
struct panel_settings
{
    int unroll, pipe, sync;
};

// Precedence: the request ("panel_unroll" > 0, "panel_pipe" / "panel_sync" >= 0), else what the build-time trial found (*_tuned;
// 0 = not tried), else the defaults (8, stream-first; sync has none of its own: an untried handle runs without a barrier).
//   unroll: 16 existed through round 3 (every instance of it spilled registers to scratch and ran slower: a request for 16 runs
//     8); anything else runs the largest of 8, 4, 2 that it reaches.
//   pipe: clamped to 0 .. 2.
//   sync: the low two bits; 2 was the split barrier through an LDS counter (measured no better than 3, deleted in round 5): 2 runs 3.
inline panel_settings panel_effective(int unroll_req, int unroll_tuned, int pipe_req, int pipe_tuned, int sync_req, int sync_tuned)
{
    const int unroll = unroll_req > 0 ? unroll_req : (unroll_tuned > 0 ? unroll_tuned : 8);
    const int pipe   = pipe_req >= 0 ? pipe_req : (pipe_tuned > 0 ? pipe_tuned : 1);
    const int sync   = (sync_req >= 0 ? sync_req : sync_tuned) & 3;
    return {unroll >= 8 ? 8 : (unroll >= 4 ? 4 : 2), std::max(0, std::min(pipe, 2)), sync == 2 ? 3 : sync};
}
}  // namespace spmv
