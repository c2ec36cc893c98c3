// Division of a tile index by a run-time divisor without a division in the kernel: the launcher turns the divisor into a
// (multiplier, shift) pair, the kernel takes the high word of one 32 x 32-bit product and shifts it (fprop_dma.hip:
// set_fetch_tile -- tile index -> (image, tile row, tile column)).  Plain C++ with no HIP in it: the host test of the pair
// (tests/test_tile_div_cpu.py) compiles this file with the host compiler alone.
//
//   n / d = (2 n + 1) / (2 d)  in integers, so with D = 2 d >= 2, s = ceil(log2 D) - 1 (2^s < D <= 2^(s+1)) and
//   m = ceil(2^(32+s) / D) -- which lies in [2^31, 2^32) --   n / d = (((2 n + 1) * m) >> 32) >> s.
//
// Why it is exact: m = (2^(32+s) + e) / D with 0 <= e < D, so N m / 2^(32+s) = N / D + N e / (D 2^(32+s)); the floor is that
// of N / D as long as N e < 2^(32+s), and e < D <= 2^(s+1) makes N < 2^31 sufficient.  With N = 2 n + 1: every n < 2^30 and
// every d in [1, 2^30).  The odd numerator is what lets d = 1 through (its own multiplier would be 2^32).
// The launchers hold the tile indices below TILE_DIV_MAX, the bound up to which the test compares every quotient and
// remainder with / and %, and decline a launch beyond it.
#pragma once
#include <stdint.h>

struct TileDiv {
    uint32_t mul, shift;
};

constexpr uint32_t TILE_DIV_MAX = 1u << 21;      // tile indices the kernels may pass (the look-ahead beyond IT included)

constexpr TileDiv tile_div_make(uint32_t d) {      // 1 <= d < 2^30
    const uint32_t D = 2u * d;
    uint32_t s = 0;
    while ((2ull << s) < D) ++s;
    return TileDiv{(uint32_t)(((1ull << (32 + s)) + D - 1) / D), s};
}

constexpr uint32_t tile_div(uint32_t n, TileDiv m) {      // n / d for n < 2^30
    return (uint32_t)(((uint64_t)(2u * n + 1u) * m.mul) >> 32) >> m.shift;
}
