// csr_f32_settings_check.cpp - csrc/csr_f32_settings.hpp walked on the host (tests/test_csr_f32_settings.py builds it with
// g++ -Wall -Werror): the entry word for every sign and the edge columns and bit patterns, the classification of a double at the
// boundaries of the float range and at the ties, the lane counts and the grid.  Prints "<checks> checks, <n> violations".
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "csr_f32_settings.hpp"

using namespace spmv;

static long checks = 0, violations = 0;
#define CHECK(cond)                                                        \
    do                                                                     \
    {                                                                      \
        ++checks;                                                          \
        if (!(cond))                                                       \
        {                                                                  \
            if (++violations <= 20) printf("line %d: %s\n", __LINE__, #cond); \
        }                                                                  \
    } while (0)

static uint32_t bits_of(float f)
{
    uint32_t b;
    memcpy(&b, &f, sizeof(b));
    return b;
}

static f32_class cls(double v)
{
    float f;
    return f32_classify(v, &f);
}
static float rounded(double v)
{
    float f;
    (void)f32_classify(v, &f);
    return f;
}

int main()
{
    // ---- the entry word ----
    const int32_t  cols[]     = {0, 1, INT32_MAX, 2, 65536, INT32_MAX - 1};
    const uint32_t patterns[] = {0x00000000u, 0x80000000u /* -0.0 */, 0x00000001u /* the smallest subnormal */, 0x807FFFFFu /* -(the largest subnormal) */,
                                 0x00800000u /* FLT_MIN */, 0x7F7FFFFFu /* FLT_MAX */, 0xFF7FFFFFu /* -FLT_MAX */, 0x3F800000u, 0xBF800000u, 0xFFFFFFFFu, 0x7FFFFFFFu};
    for (int32_t c : cols)
        for (uint32_t p : patterns)
        {
            const uint64_t w = f32_pack_bits(c, p);
            CHECK(f32_entry_col(w) == c);
            CHECK(f32_entry_bits(w) == p);
            CHECK((w >> 63) == (p >> 31));  // a negative value sets bit 63
            CHECK((uint32_t)(w & 0xFFFFFFFFull) == (uint32_t)c);
            if ((p & 0x7F800000u) != 0x7F800000u)  // (a float, not a NaN pattern: through the float itself as well)
            {
                const float f = f32_from_bits(p);
                CHECK(bits_of(f) == p);
                CHECK(f32_pack(c, f) == w);
                CHECK(bits_of(f32_entry_value(w)) == p);
            }
        }
    CHECK(f32_pack(1, -1.5f) == ((0xBFC00000ull << 32) | 1ull));
    CHECK(std::signbit(f32_entry_value(f32_pack(INT32_MAX, -0.0f))) && f32_entry_col(f32_pack(INT32_MAX, -0.0f)) == INT32_MAX);
    CHECK(f32_entry_value(f32_pack(7, -FLT_MAX)) == -FLT_MAX && f32_entry_col(f32_pack(7, -FLT_MAX)) == 7);

    // ---- the classification ----
    CHECK(kF32Max == (double)FLT_MAX && kF32Min == (double)FLT_MIN);
    CHECK(kF32FirstInf == (double)FLT_MAX + std::ldexp(1.0, 103));  // FLT_MAX + half an ulp
    for (double s : {1.0, -1.0})
    {
        CHECK(cls(s * 0.0) == kF32Exact && cls(s * 1.5) == kF32Exact);
        CHECK(cls(s * (double)FLT_MAX) == kF32Exact && rounded(s * (double)FLT_MAX) == (float)s * FLT_MAX);
        CHECK(cls(s * kF32FirstInf) == kF32Overflow);                            // the first double that rounds to inf
        CHECK(cls(s * std::nextafter(kF32FirstInf, 0.0)) == kF32Inexact);        // the last one that rounds to FLT_MAX
        CHECK(rounded(s * std::nextafter(kF32FirstInf, 0.0)) == (float)s * FLT_MAX);
        CHECK(cls(s * 1e39) == kF32Overflow && cls(s * std::numeric_limits<double>::infinity()) == kF32Overflow);
        CHECK(cls(s * std::numeric_limits<double>::max()) == kF32Overflow);
        CHECK(cls(s * (double)FLT_MIN) == kF32Exact);
        CHECK(cls(s * std::nextafter((double)FLT_MIN, 0.0)) == kF32Inexact && rounded(s * std::nextafter((double)FLT_MIN, 0.0)) == (float)s * FLT_MIN);
        CHECK(cls(s * std::ldexp(1.0, -127)) == kF32Underflow && !f32_changed(s * std::ldexp(1.0, -127), rounded(s * std::ldexp(1.0, -127))));
        CHECK(cls(s * std::ldexp(1.0, -149)) == kF32Underflow && bits_of(rounded(std::ldexp(1.0, -149))) == 1u);
        CHECK(cls(s * 1e-40) == kF32Underflow && f32_changed(s * 1e-40, rounded(s * 1e-40)) && rounded(s * 1e-40) != 0.0f);
        CHECK(cls(s * 1e-46) == kF32Underflow && rounded(s * 1e-46) == 0.0f && f32_changed(s * 1e-46, rounded(s * 1e-46)));
        CHECK(std::signbit(rounded(s * 1e-46)) == (s < 0));
        CHECK(cls(s * std::ldexp(1.0, -150)) == kF32Underflow && rounded(s * std::ldexp(1.0, -150)) == 0.0f);  // the tie below the smallest subnormal: to even, 0
        CHECK(bits_of(rounded(std::ldexp(3.0, -150))) == 2u);                                                   // 1.5 of it: the tie goes to the even 2
        // ties at half an ulp of 1.0 (ulp 2^-23): to the even neighbour
        CHECK(rounded(s * (1.0 + std::ldexp(1.0, -24))) == (float)s * 1.0f);
        CHECK(rounded(s * (1.0 + std::ldexp(3.0, -24))) == (float)s * (1.0f + std::ldexp(1.0f, -22)));
        CHECK(rounded(s * (1.0 + std::ldexp(1.0, -24) + std::ldexp(1.0, -52))) == (float)s * (1.0f + std::ldexp(1.0f, -23)));  // just above the tie: up
        CHECK(cls(s * (1.0 + std::ldexp(1.0, -24))) == kF32Inexact);
        CHECK(f32_rel_change(s * (1.0 + std::ldexp(1.0, -24)), (float)s * 1.0f) == std::ldexp(1.0, -24) / (1.0 + std::ldexp(1.0, -24)));
    }
    CHECK(cls(std::numeric_limits<double>::quiet_NaN()) == kF32Overflow);
    CHECK(!f32_changed(0.0, 0.0f) && !f32_changed(-0.0, -0.0f) && f32_changed(0.1, 0.1f) && !f32_changed(0.5, 0.5f));

    // ---- lanes and grid ----
    int valid = 0;
    for (int lanes = -2; lanes <= 130; ++lanes)
    {
        const bool pow2 = lanes == 1 || lanes == 2 || lanes == 4 || lanes == 8 || lanes == 16 || lanes == 32 || lanes == 64;
        CHECK(csr_f32_lanes_valid(lanes) == pow2);
        valid += csr_f32_lanes_valid(lanes) ? 1 : 0;
    }
    CHECK(valid == 7);
    for (int lanes = 1; lanes <= kCsrF32MaxLanes; lanes *= 2)
    {
        const int rows = csr_f32_rows_per_workgroup(lanes);
        CHECK(rows * lanes == kCsrF32Workgroup);
        for (int64_t nrow = 0; nrow <= 300; ++nrow)
        {
            const int64_t g = csr_f32_grid(nrow, lanes);
            CHECK(g * rows >= nrow);                    // every row has a lane group
            CHECK(nrow == 0 ? g == 0 : (g - 1) * rows < nrow);  // and the last workgroup holds at least one
            CHECK(csr_f32_lanes_that_fit(nrow, lanes) == lanes);
        }
        // the largest handle: fewer lanes until a launch holds fewer than 2^32 work-items
        const int fit = csr_f32_lanes_that_fit(INT32_MAX, lanes);
        CHECK(csr_f32_lanes_valid(fit) && fit <= lanes && (int64_t)INT32_MAX * fit < ((int64_t)1 << 32) && (fit == lanes || fit == 1));
        CHECK(csr_f32_grid(INT32_MAX, fit) * rows >= 0 && csr_f32_grid(INT32_MAX, fit) < ((int64_t)1 << 31));
    }
    CHECK(kCsrF32InFlight == 4);
    printf("%ld checks, %ld violations\n", checks, violations);
    return violations ? 1 : 0;
}
