// Pure host arithmetic of spmv_spgemm's row classes (spgemm.hip): no HIP, no state, so that tests/test_spgemm_settings.py can
// compile it with g++ (tests/spgemm_settings_check.cpp).
//
// A row of C = A B is classed by ub, the number of its scalar products a_ip b_pj.  A class says how many lanes of a 256-lane
// workgroup own the row and how many products the row's slice of LDS holds; a product takes kSpgemmLdsBytesPerProduct bytes there
// (an 8-byte key (column << 32 | ordinal) and its 8-byte value).  Rows beyond the largest capacity go through the global sort.
#pragma once
#include <cstdint>

namespace spmv
{
enum spgemm_class : int
{
    kSpgemmNone  = 0,  // ub = 0: the row of C is empty, no lane looks at it
    kSpgemmLane16 = 1,  // 16 lanes a row, 16 rows a workgroup
    kSpgemmWave  = 2,  // a wavefront a row, 4 rows a workgroup
    kSpgemmBlock = 3,  // the workgroup a row
    kSpgemmSort  = 4,  // expand - sort - compress in global memory
    kSpgemmClasses = 5
};

constexpr int kSpgemmBlockLanes          = 256;
constexpr int kSpgemmLdsBytesPerProduct  = 16;
constexpr int kSpgemmLdsPerCu            = 160 * 1024;
// the workgroup of every LDS class allocates this much for products: 2048 of them.  With the kernel's 1 KiB of run counts beside it,
// four workgroups share a CU's 160 KiB in the filling pass - 16 wavefronts a CU, four a SIMD, to cover the barrier of every exchange
// step - and nine in the counting pass, which keeps the keys alone.
constexpr int kSpgemmLdsAllocation = 32 * 1024;

struct spgemm_class_info
{
    int lanes;     // lanes of the workgroup that own one row (0: none)
    int capacity;  // the largest ub of the class (products a row's slice holds)
};

constexpr spgemm_class_info spgemm_info(int cls)
{
    return cls == kSpgemmLane16 ? spgemm_class_info{16, 128}
         : cls == kSpgemmWave   ? spgemm_class_info{64, 512}
         : cls == kSpgemmBlock  ? spgemm_class_info{256, 2048}
                                : spgemm_class_info{0, 0};
}
constexpr int spgemm_rows_per_block(int cls) { return spgemm_info(cls).lanes ? kSpgemmBlockLanes / spgemm_info(cls).lanes : 0; }
constexpr int spgemm_lds_bytes(int cls) { return spgemm_rows_per_block(cls) * spgemm_info(cls).capacity * kSpgemmLdsBytesPerProduct; }
constexpr int64_t kSpgemmLdsProducts = spgemm_info(kSpgemmBlock).capacity;  // "spgemm_lds_products"

// the class of a row with ub scalar products; total, and monotone in ub
constexpr int spgemm_class_of(int64_t ub)
{
    return ub <= 0                                     ? kSpgemmNone
         : ub <= spgemm_info(kSpgemmLane16).capacity ? kSpgemmLane16
         : ub <= spgemm_info(kSpgemmWave).capacity   ? kSpgemmWave
         : ub <= spgemm_info(kSpgemmBlock).capacity  ? kSpgemmBlock
                                                       : kSpgemmSort;
}

// the size of the sorting network a row of ub products needs: the next power of two, at least 2
constexpr int spgemm_network(int64_t ub)
{
    int p = 2;
    while (p < ub) p <<= 1;
    return p;
}
}  // namespace spmv
