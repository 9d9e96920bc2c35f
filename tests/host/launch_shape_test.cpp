// Host test of ginkgo_amd/csrc/launch_shape.hpp: the grid of a grid-stride kernel and the lanes-per-row choice.
// Built and run by tests/test_launch_shape_cpu.py:
//   g++ -std=c++17 -I ginkgo_amd/csrc tests/host/launch_shape_test.cpp
// capped_grid is compared with the formulas the launchers spelled out before they shared it, at every
// (items per workgroup, cap) pair some launcher of ginkgo_amd/csrc uses.
#include "launch_shape.hpp"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

namespace {

constexpr int max_stream_blocks = 2048;      // common.hpp

int64_t ceildiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// split_grid, sor_grid, symb_grid, cv_grid, flat_grid and (with blocks = ceildiv(items, per_block) at the call)
// the capped_grid of isai.hip and pgm.hip
unsigned old_floor_last(int64_t items, int per_block, int64_t cap)
{
    int64_t b = ceildiv(items, per_block);
    if (b > cap) b = cap;
    return unsigned(b < 1 ? 1 : b);
}
// grid_of, grid_for, blocks_for of complex_formats.hip, stream_blocks of gmres.hip
unsigned old_floor_first(int64_t items, int per_block, int64_t cap)
{
    int64_t b = ceildiv(items > 0 ? items : 1, per_block);
    if (b > cap) b = cap;
    return unsigned(b);
}
// fb_grid
unsigned old_fb(int64_t items, int per_block, int64_t cap)
{
    const int64_t g = ceildiv(items, per_block);
    return unsigned(g < cap ? (g > 0 ? g : 1) : cap);
}
// idr_blocks
unsigned old_idr(int64_t items, int per_block, int64_t cap)
{
    int64_t nb = ceildiv(items, per_block);
    return unsigned(nb > cap ? cap : (nb < 1 ? 1 : nb));
}
// the open-coded form and stream_blocks of par_ilut.hip: no floor, their callers have items >= 1
unsigned old_open(int64_t items, int per_block, int64_t cap)
{
    int64_t blocks = ceildiv(items, per_block);
    if (blocks > cap) blocks = cap;
    return unsigned(blocks);
}
// blocks_for of formats.hip: no cap
unsigned old_uncapped(int64_t items, int per_block) { return unsigned(ceildiv(items > 0 ? items : 1, per_block)); }

void check_pair(int per_block, int64_t cap)
{
    const int64_t full = cap * per_block;
    const int64_t items[] = {0, 1, per_block - 1, per_block, per_block + 1, full - 1, full, full + 1,
                             int64_t(1) << 40};
    for (const int64_t n : items) {
        const unsigned g = gkoc::capped_grid(n, per_block, cap);
        CHECK(g == old_floor_last(n, per_block, cap));
        CHECK(g == old_floor_first(n, per_block, cap));
        CHECK(g == old_fb(n, per_block, cap));
        CHECK(g == old_idr(n, per_block, cap));
        if (n >= 1) CHECK(g == old_open(n, per_block, cap));
        // what the formula is for: between 1 and cap workgroups, and enough of them below the cap
        CHECK(g >= 1 && int64_t(g) <= cap);
        CHECK(int64_t(g) == cap || int64_t(g) * per_block >= n);
        CHECK(g == 1 || (int64_t(g) - 1) * per_block < n);
    }
}

int picked(int longest, const int (&limits)[3])
{
    return gkoc::with_lanes(longest, limits, [](auto w) { return int(decltype(w)::value); });
}

}  // namespace

int main()
{
    // every (items per workgroup, cap) pair of the launchers: 256 threads take 256 items or 256 / W rows with
    // W = 16, 32, 64 lanes per row, isai.hip's workgroup kernel takes one row; caps of 1, 4 and 8 times
    // max_stream_blocks
    const int64_t m = max_stream_blocks;
    for (const int per_block : {256, 16, 8, 4, 1}) check_pair(per_block, 4 * m);
    for (const int per_block : {256, 16, 8, 4}) check_pair(per_block, m);
    check_pair(256, 8 * m);
    // without a cap (formats.hip), the conversion to unsigned included
    for (const int64_t n : {int64_t(0), int64_t(1), int64_t(255), int64_t(256), int64_t(257), int64_t(1) << 40}) {
        CHECK(gkoc::capped_grid(n, 256, gkoc::no_grid_cap) == old_uncapped(n, 256));
    }
    // pgm.hip multiplies by 4 after capping
    CHECK(gkoc::capped_grid(int64_t(1) << 40, 4, m) * 4 == 4 * 2048u);

    // 16 lanes up to limits[0], 32 up to limits[1], else 64 - also where a table goes on after its second entry
    const int tables[][3] = {{16, 32, 64}, {5, 9, 100}};
    for (const auto& limits : tables) {
        CHECK(picked(0, limits) == 16);
        CHECK(picked(limits[0], limits) == 16);
        CHECK(picked(limits[0] + 1, limits) == 32);
        CHECK(picked(limits[1], limits) == 32);
        CHECK(picked(limits[1] + 1, limits) == 64);
        CHECK(picked(INT_MAX, limits) == 64);
    }
    const int general[] = {16, 32, 64, 128};      // isai.hip's general_row_limits
    const auto width = [](auto w) { return int(decltype(w)::value); };
    CHECK(gkoc::with_lanes(0, general, width) == 16);
    CHECK(gkoc::with_lanes(16, general, width) == 16);
    CHECK(gkoc::with_lanes(17, general, width) == 32);
    CHECK(gkoc::with_lanes(32, general, width) == 32);
    CHECK(gkoc::with_lanes(33, general, width) == 64);
    CHECK(gkoc::with_lanes(65, general, width) == 64);
    CHECK(gkoc::with_lanes(INT_MAX, general, width) == 64);
    // the result of f is handed through
    CHECK(gkoc::with_lanes(1, general, [](auto) { return -7; }) == -7);
    std::printf("launch_shape_test OK\n");
    return 0;
}
