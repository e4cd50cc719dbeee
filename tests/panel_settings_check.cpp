// Properties of arm-spmv_amd/csrc/panel_settings.hpp (the panel kernel's effective launch settings).  Compiled and run by
// tests/test_abi_and_host.py; prints one summary line.  Every combination of requests ("panel_unroll" -1 .. 32, "panel_pipe"
// -1 .. 4, "panel_sync" -1 .. 8) and build-time trial results (unroll 0 / 2 / 4 / 8, pipe 0 .. 2, sync 0 .. 3) is walked:
//   * panel_effective gives what panel_launch and the plan's collect computed, each for itself, before there was one function:
//     their expressions are restated below word for word;
//   * the result is always an instantiated combination (unroll 2 / 4 / 8, pipe 0 / 1 / 2, sync 0 / 1 / 3), so no setting can
//     reach the "is not instantiated" refusal at the end of panel_launch;
//   * on the values include/spmv_abi.h documents (unroll 0, 2, 4, 8, 16; pipe -1 .. 2; sync -1 .. 3) what spmv_mat_get_param
//     reports for the three parameters - restated too - is what runs.
#include <algorithm>
#include <cstdio>
#include "panel_settings.hpp"

int main()
{
    const int tuned_unrolls[] = {0, 2, 4, 8};
    long long walked = 0, differ = 0, outside = 0, documented = 0, report_differs = 0;
    for (int U = -1; U <= 32; ++U)
        for (int UT : tuned_unrolls)
            for (int P = -1; P <= 4; ++P)
                for (int PT = 0; PT <= 2; ++PT)
                    for (int S = -1; S <= 8; ++S)
                        for (int ST = 0; ST <= 3; ++ST)
                        {
                            ++walked;
                            const spmv::panel_settings e = spmv::panel_effective(U, UT, P, PT, S, ST);
                            // panel_launch
                            const int unroll_rq = U > 0 ? U : (UT > 0 ? UT : 8);
                            const int unroll    = unroll_rq >= 16 ? 8 : (unroll_rq >= 8 ? 8 : (unroll_rq >= 4 ? 4 : 2));
                            const int sync_rq   = (S >= 0 ? S : ST) & 3;
                            const int sync      = sync_rq == 2 ? 3 : sync_rq;
                            const int pipe_rq   = P >= 0 ? P : (PT > 0 ? PT : 1);
                            const int pipe      = std::max(0, std::min(pipe_rq, 2));
                            if (e.unroll != unroll || e.pipe != pipe || e.sync != sync) ++differ;
                            // the plan's collect
                            const int plan_unroll0 = U > 0 ? U : (UT > 0 ? UT : 8);
                            const int plan_unroll  = plan_unroll0 >= 8 ? 8 : (plan_unroll0 >= 4 ? 4 : 2);
                            const int plan_pipe    = std::max(0, std::min(P >= 0 ? P : (PT > 0 ? PT : 1), 2));
                            const int plan_sync0   = (S >= 0 ? S : ST) & 3;
                            const int plan_sync    = plan_sync0 == 2 ? 3 : plan_sync0;
                            if (e.unroll != plan_unroll || e.pipe != plan_pipe || e.sync != plan_sync) ++differ;
                            if (!(e.unroll == 2 || e.unroll == 4 || e.unroll == 8) || e.pipe < 0 || e.pipe > 2 || !(e.sync == 0 || e.sync == 1 || e.sync == 3))
                                ++outside;
                            // spmv_mat_get_param
                            if ((U == 0 || U == 2 || U == 4 || U == 8 || U == 16) && P <= 2 && S <= 3)
                            {
                                ++documented;
                                const int get_unroll = std::min(8, U > 0 ? U : (UT > 0 ? UT : 8));
                                const int get_pipe   = P >= 0 ? P : (PT > 0 ? PT : 1);
                                const int get_sync   = (S >= 0 ? S : ST) == 2 ? 3 : (S >= 0 ? S : ST);
                                if (get_unroll != e.unroll || get_pipe != e.pipe || get_sync != e.sync) ++report_differs;
                            }
                        }
    std::printf("panel_settings: %lld combinations, %lld differences, %lld not instantiated, %lld documented, %lld reported differently\n", walked,
                differ, outside, documented, report_differs);
    return differ || outside || report_differs ? 1 : 0;
}
