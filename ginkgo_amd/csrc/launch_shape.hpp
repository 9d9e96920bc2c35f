// The two host-side choices every launcher of the library makes: how many workgroups a grid-stride kernel gets,
// and how many lanes (16, 32 or 64) take one row of a sparse matrix.  Host only, no ROCm include: it compiles
// with a plain C++17 compiler (tests/host/launch_shape_test.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace gkoc {

// ceil(items / per_block) workgroups, at most `cap`, at least 1
inline unsigned capped_grid(int64_t items, int per_block, int64_t cap)
{
    int64_t blocks = (items + per_block - 1) / per_block;
    if (blocks > cap) blocks = cap;
    return unsigned(blocks < 1 ? 1 : blocks);
}
// for the few grids that have no cap
constexpr int64_t no_grid_cap = INT64_MAX;

// f(std::integral_constant<int, W>{}) with W = 16 for a longest row of at most limits[0] entries, 32 up to
// limits[1], else 64 (a group of 64 lanes streams a longer row); the table may go on (isai.hip's does)
template <size_t N, typename F>
int with_lanes(int longest, const int (&limits)[N], F&& f)
{
    static_assert(N >= 2, "the limits of 16 and of 32 lanes");
    if (longest <= limits[0]) return f(std::integral_constant<int, 16>{});
    if (longest <= limits[1]) return f(std::integral_constant<int, 32>{});
    return f(std::integral_constant<int, 64>{});
}

}  // namespace gkoc
