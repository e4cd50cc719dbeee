// Properties of arm-spmv_amd/csrc/spgemm_settings.hpp (spmv_spgemm: the class of a row of C by its number of scalar products).
// Compiled and run by tests/test_spgemm_settings.py; prints one summary line.
//   * the class function is total (one of the five classes for every ub, negative and huge ones included) and monotone in ub;
//   * ub = 0 gets no work (no lanes, no LDS); every other class below SORT has lanes that divide the workgroup;
//   * a class's LDS bytes (rows a workgroup x capacity x bytes a product) fit the declared allocation and the CU's 160 KiB;
//   * the values on both sides of every class edge land where the header says; capacities are powers of two (the network's size)
//     and the network of every ub of a class fits the class's capacity;
//   * the largest capacity is "spgemm_lds_products" and is at least 2048.
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include "spgemm_settings.hpp"

int main()
{
    using namespace spmv;
    long long bad = 0, checked = 0;
    int       prev = kSpgemmNone;
    for (int64_t ub = -3; ub <= 3 * kSpgemmLdsProducts; ++ub)
    {
        const int c = spgemm_class_of(ub);
        ++checked;
        if (c < kSpgemmNone || c >= kSpgemmClasses || c < prev) ++bad;
        if ((c == kSpgemmNone) != (ub <= 0)) ++bad;
        if (c != kSpgemmNone && c != kSpgemmSort && (ub > spgemm_info(c).capacity || spgemm_network(ub) > spgemm_info(c).capacity)) ++bad;
        if (spgemm_network(ub) < 2 || spgemm_network(ub) < ub || (ub > 2 && spgemm_network(ub) >= 2 * ub)) ++bad;
        prev = c;
    }
    for (int64_t ub : {(int64_t)1 << 31, (int64_t)1 << 40, INT64_MAX})
        if (spgemm_class_of(ub) != kSpgemmSort) ++bad;
    if (spgemm_class_of(INT64_MIN) != kSpgemmNone) ++bad;
    // the edges, by the header's own capacities
    int edges = 0;
    for (int c = kSpgemmLane16; c <= kSpgemmBlock; ++c)
    {
        const spgemm_class_info info = spgemm_info(c);
        const int64_t           cap  = info.capacity;
        ++edges;
        if (spgemm_class_of(cap) != c || spgemm_class_of(cap + 1) != c + 1 || spgemm_class_of(cap - 1) != c) ++bad;
        if (info.lanes <= 0 || kSpgemmBlockLanes % info.lanes || (cap & (cap - 1))) ++bad;
        if (spgemm_lds_bytes(c) > kSpgemmLdsAllocation || spgemm_lds_bytes(c) > kSpgemmLdsPerCu) ++bad;
        if (spgemm_lds_bytes(c) != spgemm_rows_per_block(c) * info.capacity * kSpgemmLdsBytesPerProduct) ++bad;
        if (c > kSpgemmLane16 && (info.capacity <= spgemm_info(c - 1).capacity || info.lanes <= spgemm_info(c - 1).lanes)) ++bad;
    }
    if (spgemm_class_of(1) != kSpgemmLane16 || spgemm_class_of(0) != kSpgemmNone) ++bad;
    if (spgemm_info(kSpgemmNone).lanes || spgemm_lds_bytes(kSpgemmNone) || spgemm_info(kSpgemmSort).lanes || spgemm_lds_bytes(kSpgemmSort)) ++bad;
    if (kSpgemmLdsProducts != spgemm_info(kSpgemmBlock).capacity || kSpgemmLdsProducts < 2048) ++bad;
    if (kSpgemmLdsAllocation > kSpgemmLdsPerCu) ++bad;
    std::printf("spgemm_settings: %lld values of ub, %d class edges, capacity %lld, %lld violations\n", checked, edges, (long long)kSpgemmLdsProducts, bad);
    return bad ? 1 : 0;
}
