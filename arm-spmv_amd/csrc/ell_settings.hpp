// Pure host arithmetic of what a product of an ELL handle launches (kernels_ell.hip: ell_own_apply): no HIP, no state, so that
// tests/test_abi_and_host.py can compile it with g++ and walk every handle state (tests/ell_settings_check.cpp).
#pragma once

namespace spmv
{
// the variants of the format's own product: spmv_mat::ell_variant, plan_node::ell_variant, "ell_variant" / "ell_copy_variant"
enum ell_variant_id : int
{
    kEllTwoRows     = 0,  // two rows per lane - over the slots' diagonals where they were found (no index stream), else reading columns
    kEllOneRow      = 1,  // one row per lane (more wavefronts: wins below ~200K rows)
    kEllReadColumns = 2,  // two rows per lane reading every column index, diagonals or not
    kEllDiaOrder    = 3,  // the DIA kernel over the DIA-order copy of the values, the non-conforming rows by a side kernel
    kEllVariants
};
// what lanes_per_row (spmv_mat_set_kernel) means on an ELL handle; every other value: two rows per lane, 4 slots in flight
constexpr int kEllLanesOneRow = 1, kEllLanesUnroll8 = 4, kEllLanesUnroll2 = 8;  // the one-row kernel; two rows per lane, 8 / 2 slots in flight
enum class ell_path
{
    dia_order,   // dia_rows_apply over the DIA-order copy, then ell_rows_list_kernel
    diag_x2,     // ell_diag_kernel_x2<unroll, xwin, tiled, masked>
    columns_x2,  // ell_kernel_x2<unroll, masked>
    one_row      // ell_kernel<8, masked>
};
// The instantiated combinations: unroll 2 / 4 / 8 on the two-row paths, 8 on the one-row path; xwin (x through LDS windows) and tiled
// (values from the tiles of 512 rows) on the diagonal path only; masked (the ELL copy of a CSR handle: padding left out of the sums)
// on the format's three kernels.  The DIA-order path takes none: unroll 0, the rest false.
struct ell_settings
{
    ell_path path;
    int      unroll;
    bool     xwin, tiled, masked;
};
constexpr int kEllMaxWindowDoubles = 5120;  // the x stretches of 512 rows fit 40 KB of LDS
// Variant 3 runs only with its copy AND the slot descriptors in memory and SPMV_FLAG_ELL_READ_COLUMNS off; anything less falls
// through as if the variant were 0.  Two rows per lane need an even nrow and col_ind / values / y aligned to 8 / 16 / 16 bytes and
// are given up for lanes_per_row 1 or variant 1; the diagonal kernel needs descriptors and mask, the flag off, a variant other than 2.
inline ell_settings ell_effective(int variant, int lanes_per_row, bool read_columns, bool nrow_even, bool col_aligned8, bool val_aligned16,
                                  bool y_aligned16, bool has_descriptors, bool has_mask, bool has_tiles, bool has_dia_copy, int diag_lds,
                                  bool pad_marked)
{
    if (variant == kEllDiaOrder && has_dia_copy && has_descriptors && !read_columns) return {ell_path::dia_order, 0, false, false, false};
    const bool x2 = nrow_even && col_aligned8 && val_aligned16 && y_aligned16 && lanes_per_row != kEllLanesOneRow && variant != kEllOneRow;
    if (!x2) return {ell_path::one_row, 8, false, false, pad_marked};
    const int unroll = lanes_per_row == kEllLanesUnroll8 ? 8 : (lanes_per_row == kEllLanesUnroll2 ? 2 : 4);
    if (has_descriptors && has_mask && !read_columns && variant != kEllReadColumns)
        return {ell_path::diag_x2, unroll, diag_lds > 0 && diag_lds <= kEllMaxWindowDoubles, has_tiles, pad_marked};
    return {ell_path::columns_x2, unroll, false, false, pad_marked};
}
}  // namespace spmv
