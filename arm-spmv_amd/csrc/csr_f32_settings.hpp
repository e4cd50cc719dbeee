// csr_f32_settings.hpp - the arithmetic of CSR with single-precision value storage (SPMV_FMT_CSR_F32; kernels_csr_f32.hip,
// convert_f32.hip) as plain functions that a host compiler takes too: the packed entry word, what rounding one double to float
// does to it, which lane counts a row may get and the size of the grid.  tests/csr_f32_settings_check.cpp walks every one of
// them with g++.
//
// An entry is ONE 8-byte word: the column in the low 32 bits, the IEEE bits of the float value in the high 32.  A negative
// value sets bit 63 of the word, so the word is unsigned everywhere and the column is taken from its low half alone: nothing
// is shifted down through a signed type.
//
// The product follows the row-parallel CSR kernel: LPR = 2^k lanes per row, kCsrF32Workgroup / LPR rows per workgroup, lane l of a
// row's group on entries l, l + LPR, ..., kCsrF32InFlight entries in flight per lane before the first fma.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SPMV_F32_HD __host__ __device__
#else
#define SPMV_F32_HD
#endif

namespace spmv
{
constexpr int kCsrF32Workgroup = 256;  // four wavefronts
constexpr int kCsrF32MaxLanes  = 64;   // a row's lanes stay inside one wavefront
constexpr int kCsrF32InFlight  = 4;    // entries a lane has in flight before its first fma

// ---- the entry word --------------------------------------------------------------------------------------------------------------
SPMV_F32_HD inline uint32_t f32_bits(float v) { return __builtin_bit_cast(uint32_t, v); }
SPMV_F32_HD inline float    f32_from_bits(uint32_t b) { return __builtin_bit_cast(float, b); }
SPMV_F32_HD inline uint64_t f32_pack_bits(int32_t col, uint32_t value_bits) { return (uint64_t)(uint32_t)col | ((uint64_t)value_bits << 32); }
SPMV_F32_HD inline uint64_t f32_pack(int32_t col, float v) { return f32_pack_bits(col, f32_bits(v)); }
SPMV_F32_HD inline int32_t  f32_entry_col(uint64_t word) { return (int32_t)(uint32_t)(word & 0xFFFFFFFFull); }
SPMV_F32_HD inline uint32_t f32_entry_bits(uint64_t word) { return (uint32_t)(word >> 32); }
SPMV_F32_HD inline float    f32_entry_value(uint64_t word) { return f32_from_bits(f32_entry_bits(word)); }

// ---- one double under rounding to float (nearest, ties to even) --------------------------------------------------------------------
// exact:     float(v) == v, and v is 0 or a normal float;
// inexact:   float(v) != v, the result a normal float: counted as changed, and its relative change takes part in the maximum;
// underflow: v != 0 and float(v) is zero or subnormal (whether the bits changed or not: f32_changed says); no part in the maximum;
// overflow:  v is not finite, or float(v) is +-inf: the conversion is refused.
enum f32_class : int
{
    kF32Exact     = 0,
    kF32Inexact   = 1,
    kF32Underflow = 2,
    kF32Overflow  = 3
};
constexpr double kF32Max = 0x1.fffffep+127;  // FLT_MAX
constexpr double kF32Min = 0x1p-126;         // FLT_MIN, the smallest normal float
// the first double that rounds to +inf: FLT_MAX + half an ulp (the tie goes to the even neighbour, which is 2^128)
constexpr double kF32FirstInf = 0x1.ffffffp+127;

SPMV_F32_HD inline f32_class f32_classify(double v, float* rounded)
{
    const double a = v < 0 ? -v : v;
    if (!(a < kF32FirstInf))  // (NaN compares false: refused as well; the value is never converted)
    {
        *rounded = 0.0f;
        return kF32Overflow;
    }
    const float  f  = (float)v;
    const double fa = f < 0 ? -(double)f : (double)f;
    *rounded        = f;
    if (a != 0.0 && fa < kF32Min) return kF32Underflow;
    return (double)f == v ? kF32Exact : kF32Inexact;
}
SPMV_F32_HD inline bool f32_changed(double v, float rounded) { return !((double)rounded == v); }
// |float(v) - v| / |v| of a value classified inexact (the subtraction is exact: both are multiples of v's last place)
SPMV_F32_HD inline double f32_rel_change(double v, float rounded)
{
    const double d = (double)rounded - v;
    return (d < 0 ? -d : d) / (v < 0 ? -v : v);
}

// ---- lanes and grid --------------------------------------------------------------------------------------------------------------
SPMV_F32_HD constexpr bool csr_f32_lanes_valid(int lanes) { return lanes >= 1 && lanes <= kCsrF32MaxLanes && (lanes & (lanes - 1)) == 0; }
SPMV_F32_HD constexpr int  csr_f32_rows_per_workgroup(int lanes) { return kCsrF32Workgroup / lanes; }
// workgroups of a product over nrow rows (0: nothing to launch)
SPMV_F32_HD constexpr int64_t csr_f32_grid(int64_t nrow, int lanes)
{
    return (nrow + csr_f32_rows_per_workgroup(lanes) - 1) / csr_f32_rows_per_workgroup(lanes);
}
// a launch holds fewer than 2^32 work-items: the most lanes <= `lanes` under which nrow rows still fit (as the CSR kernel's launch)
SPMV_F32_HD constexpr int csr_f32_lanes_that_fit(int64_t nrow, int lanes)
{
    while (lanes > 1 && nrow * lanes >= ((int64_t)1 << 32) - kCsrF32Workgroup) lanes >>= 1;
    return lanes;
}
}  // namespace spmv
