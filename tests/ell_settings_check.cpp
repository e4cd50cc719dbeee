// Properties of arm-spmv_amd/csrc/ell_settings.hpp (what a product of an ELL handle launches).  Compiled and run by
// tests/test_abi_and_host.py; prints one summary line.  Every combination of ell_variant 0 .. 3, lanes_per_row 0 / 1 / 2 / 4 / 8 /
// 16 / 32 / 64, SPMV_FLAG_ELL_READ_COLUMNS, the parity of nrow, the alignment of col_ind (8) / values (16) / y (16), the presence of
// slot descriptors / mask / tiled values / DIA-order copy, ell_diag_lds 0 / 1 / 5120 / 5121 and ell_pad_marked is walked:
//   * ell_effective gives what ell_own_apply decided before there was one function: its nested conditions and the three layers of
//     launch macros are restated below, branch for branch, over a stand-in for the handle;
//   * the result is always an instantiated combination: unroll 2 / 4 / 8 on the two-row paths and 8 on the one-row path, xwin and
//     tiled on the diagonal path only, none of the four on the DIA-order path.
#include <cstdio>
#include "ell_settings.hpp"

namespace
{
// the fields of the handle and of the call that the conditions read
struct handle
{
    int  ell_variant, lanes_per_row;
    bool flag_read_columns, nrow_even, b_aligned8, v_aligned16, y_aligned16;
    bool ell_diag, ell_diag_mask, ell_tval, ell_rval;
    int  ell_diag_lds;
    bool ell_pad_marked;
};

struct launched
{
    int  kernel;  // 0 dia_rows_apply + ell_rows_list_kernel, 1 ell_diag_kernel_x2, 2 ell_kernel_x2, 3 ell_kernel
    int  unroll;
    bool xwin, tiled, masked;
};

// ell_own_apply as it stood, a launch written as the record of its template arguments
launched own_apply_before(const handle& A)
{
    if (A.ell_variant == 3 && A.ell_rval && A.ell_diag && !A.flag_read_columns) return {0, 0, false, false, false};
    const bool aligned = A.nrow_even && A.b_aligned8 && A.v_aligned16 && A.y_aligned16;
    const bool x2      = aligned && !(A.lanes_per_row == 1) && A.ell_variant != 1;
    if (x2 && A.ell_diag && A.ell_diag_mask && !A.flag_read_columns && A.ell_variant != 2)
    {
        const bool xwin = A.ell_diag_lds > 0 && A.ell_diag_lds <= 5120;
        // SPMV_ELL_DIAG(U, W): by ell_pad_marked and ell_tval to SPMV_ELL_DIAG_M(U, W, T, M)
        auto diag = [&](int U, bool W) -> launched {
            if (A.ell_pad_marked)
            {
                if (A.ell_tval) return {1, U, W, true, true};
                return {1, U, W, false, true};
            }
            else if (A.ell_tval)
                return {1, U, W, true, false};
            return {1, U, W, false, false};
        };
        if (A.lanes_per_row == 4)
        {
            if (xwin) return diag(8, true); else return diag(8, false);
        }
        else if (A.lanes_per_row == 8)
        {
            if (xwin) return diag(2, true); else return diag(2, false);
        }
        else
        {
            if (xwin) return diag(4, true); else return diag(4, false);
        }
    }
    else if (x2)
    {
        // SPMV_ELL_X2(U)
        auto cols = [&](int U) -> launched {
            if (A.ell_pad_marked) return {2, U, false, false, true};
            return {2, U, false, false, false};
        };
        if (A.lanes_per_row == 4)
            return cols(8);
        else if (A.lanes_per_row == 8)
            return cols(2);
        else
            return cols(4);
    }
    else
    {
        if (A.ell_pad_marked) return {3, 8, false, false, true};
        return {3, 8, false, false, false};
    }
}

int kernel_of(spmv::ell_path p)
{
    switch (p)
    {
        case spmv::ell_path::dia_order: return 0;
        case spmv::ell_path::diag_x2: return 1;
        case spmv::ell_path::columns_x2: return 2;
        default: return 3;
    }
}
}  // namespace

int main()
{
    const int lanes[] = {0, 1, 2, 4, 8, 16, 32, 64}, lds[] = {0, 1, 5120, 5121};
    long long walked = 0, differ = 0, outside = 0, per_path[4] = {0, 0, 0, 0};
    for (int variant = 0; variant <= 3; ++variant)
        for (int L : lanes)
            for (int bits = 0; bits < (1 << 10); ++bits)  // ten yes / no facts
                for (int D : lds)
                {
                    const auto   bit = [&](int i) { return ((bits >> i) & 1) != 0; };
                    const handle A{variant, L, bit(0), bit(1), bit(2), bit(3), bit(4), bit(5), bit(6), bit(7), bit(8), D, bit(9)};
                    ++walked;
                    const spmv::ell_settings e = spmv::ell_effective(A.ell_variant, A.lanes_per_row, A.flag_read_columns, A.nrow_even, A.b_aligned8, A.v_aligned16, A.y_aligned16,
                                                                     A.ell_diag, A.ell_diag_mask, A.ell_tval, A.ell_rval, A.ell_diag_lds, A.ell_pad_marked);
                    const launched           w = own_apply_before(A);
                    const int                k = kernel_of(e.path);
                    ++per_path[k];
                    if (k != w.kernel || e.unroll != w.unroll || e.xwin != w.xwin || e.tiled != w.tiled || e.masked != w.masked) ++differ;
                    const bool two_rows = e.path == spmv::ell_path::diag_x2 || e.path == spmv::ell_path::columns_x2;
                    bool       ok       = true;
                    if (two_rows) ok = e.unroll == 2 || e.unroll == 4 || e.unroll == 8;
                    if (e.path == spmv::ell_path::one_row) ok = e.unroll == 8;
                    if (e.path == spmv::ell_path::dia_order) ok = e.unroll == 0 && !e.masked;
                    if (e.path != spmv::ell_path::diag_x2 && (e.xwin || e.tiled)) ok = false;
                    if (!ok) ++outside;
                }
    std::printf("ell_settings: %lld combinations, %lld differences, %lld not instantiated, paths %lld %lld %lld %lld\n", walked, differ, outside, per_path[0],
                per_path[1], per_path[2], per_path[3]);
    return differ || outside ? 1 : 0;
}
