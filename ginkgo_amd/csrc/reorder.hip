// Nested dissection: the graph kernels of reorder::NestedDissection (include/gko_cdna4.h, "Nested dissection").
//   reorder_components   min-label propagation inside every region           one launch per sweep
//   reorder_levels       breadth-first levels of every region from its root  one launch per step
//   reorder_far_roots    the smallest vertex of the last level, per region
//   reorder_split        |R|, h, m* per region, then the class (A, B, S, undivided) of every vertex
//   reorder_regroup      order[] stably sorted by (segment, key, vertex); the runs are the new segments
//
// All regions of one recursion depth are worked on at once.  State: order[] (every region one contiguous ascending
// segment) and region[v] (the position where v's segment starts, -1: v is final).  Arrays "per region" are indexed
// by the segment's start, so they need no more than n words and no numbering of the regions.
//
// Kernels that read rows: one group of W = 16 / 32 / 64 lanes per row (W from the longest row of the call, limits
// in reorder_row_limits), lane = stored entry, rows spread over the grid; a row with more entries than W (W is 64
// then) is streamed in rounds of W entries.  The searches (levels, the separator test of split) leave the rounds
// at the first hit.  Pull style: a vertex looks at its neighbours and writes its own word.
//
// Invariants:
//   1. every output word is written by exactly one lane.  The histogram and the far roots use integer atomics on
//      scratch words (add, max, min: order-independent); "something changed" is a plain store of 1;
//   2. a components sweep reads one label buffer and writes the other.  A level step works in place: it tests
//      level[u] == t while other groups store t + 1 into words that held -1, and neither value equals t;
//   3. the loops the host drives (sweeps, steps) end after at most n iterations, with an error if the last one
//      still changed something; no kernel waits for another workgroup;
//   4. a slot s + level, a run index and a position are compared with the array's size before they index;
//   5. no entry writes an index array of a matrix: everything written is state of the reordering
//      (gkoc_reorder_i32 / _i64 in the header), like the aggregation state of pgm.hip.
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <climits>
#include <type_traits>

#include "common.hpp"
#include "scan.hpp"
#include "sparse_rows.hpp"

namespace gkoc {
namespace {

constexpr int reorder_row_limits[] = {16, 32, 64};
constexpr int reo_block = 256;

// the unsigned twin of an index type: what the integer atomics work on (every value they see is >= 0)
template <typename I>
using atomic_word = std::conditional_t<sizeof(I) == 4, unsigned int, unsigned long long>;

template <typename I>
__device__ __forceinline__ atomic_word<I>* as_atomic(I* p)
{
    return reinterpret_cast<atomic_word<I>*>(p);
}

template <int W>
__device__ __forceinline__ long long group_min(long long v)
{
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) {
        const long long o = __shfl_xor(v, off, W);
        v = o < v ? o : v;
    }
    return v;
}

// status words of the checks
enum : int { st_pattern = 0, st_region, st_root, st_longest, st_level, st_order, st_key, st_changed, st_words };

// ------------------------------------------------------------------ checks (one thread per vertex)
// Every array may be null: its check is skipped.  level: inside [-1, n); with need_level a live vertex has one and
// its slot (segment start + level) lies inside the array.  filled: order scattered into a -1-filled array by
// scatter_positions - every word written means order is a permutation.  key: of a live vertex, in [0, key_end).
template <typename I>
__global__ __launch_bounds__(reo_block) void reorder_check_kernel(
    int64_t n, int64_t nnz, const I* __restrict__ rp, const I* __restrict__ ci, const I* __restrict__ region,
    const I* __restrict__ root, const I* __restrict__ level, int need_level, const I* __restrict__ order,
    const I* __restrict__ filled, const I* __restrict__ key, int64_t key_end, int* __restrict__ status)
{
    const int64_t stride = int64_t(gridDim.x) * reo_block;
    int longest = 0;
    for (int64_t v = int64_t(blockIdx.x) * reo_block + threadIdx.x; v < n; v += stride) {
        int64_t s = -1;
        if (region) {
            s = region[v];
            if (s < -1 || s >= n) {
                status[st_region] = 1;
                s = -1;
            }
        }
        if (root && s >= 0) {
            const int64_t r = root[s];
            if (r < 0 || r >= n) status[st_root] = 1;
        }
        if (level) {
            const int64_t l = level[v];
            if (l < -1 || l >= n || (need_level && s >= 0 && (l < 0 || s + l >= n))) status[st_level] = 1;
        }
        if (order) {
            const int64_t o = order[v];
            if (o < 0 || o >= n || int64_t(filled[v]) < 0) status[st_order] = 1;
        }
        if (key && s >= 0) {
            const int64_t k = key[v];
            if (k < 0 || k >= key_end) status[st_key] = 1;
        }
        if (rp) {
            const int64_t begin = rp[v], end = rp[v + 1];
            if (begin < 0 || end < begin || end > nnz || (v == 0 && begin != 0) || (v == n - 1 && end != nnz)) {
                status[st_pattern] = 1;
            } else {
                for (int64_t k = begin; k < end; ++k) {
                    const int64_t col = ci[k];
                    if (col < 0 || col >= n) status[st_pattern] = 1;
                }
                const int64_t len = end - begin;
                longest = len > longest ? int(len > INT_MAX ? INT_MAX : len) : longest;
            }
        }
    }
    note_longest(longest, &status[st_longest]);
}

// pos[order[p]] = p wherever order[p] is inside [0, n) (the check kernel reports the others)
template <typename I>
__global__ __launch_bounds__(reo_block) void scatter_positions_kernel(int64_t n, const I* __restrict__ order,
                                                                      I* __restrict__ pos)
{
    const int64_t stride = int64_t(gridDim.x) * reo_block;
    for (int64_t p = int64_t(blockIdx.x) * reo_block + threadIdx.x; p < n; p += stride) {
        const int64_t v = order[p];
        if (v >= 0 && v < n) pos[v] = I(p);
    }
}

inline int require_checked(const int (&host)[st_words])
{
    GKOC_REQUIRE(host[st_pattern] == 0, GKOC_E_INVALID,
                 "row pointers do not ascend from 0 to nnz, or a column outside [0, n)");
    GKOC_REQUIRE(host[st_region] == 0, GKOC_E_INVALID, "region[v] outside [-1, n)");
    GKOC_REQUIRE(host[st_root] == 0, GKOC_E_INVALID, "the root of a region outside [0, n)");
    GKOC_REQUIRE(host[st_level] == 0, GKOC_E_INVALID,
                 "level[v] outside [-1, n), a live vertex without a level, or a level that leaves its segment");
    GKOC_REQUIRE(host[st_order] == 0, GKOC_E_INVALID, "order is no permutation of [0, n)");
    GKOC_REQUIRE(host[st_key] == 0, GKOC_E_INVALID, "the key of a live vertex outside [0, max(n, 4))");
    return GKOC_OK;
}

// the checks of an entry, one launch and one copy; *longest = the longest row (0 without a pattern)
template <typename I>
int reorder_checked(status_words<st_words>& status, int64_t n, int64_t nnz, const I* rp, const I* ci,
                    const I* region, const I* root, const I* level, int need_level, const I* order,
                    const I* filled, const I* key, int64_t key_end, int* longest)
{
    reorder_check_kernel<I><<<dim3(stream_grid(n, reo_block)), dim3(reo_block), 0, status.st>>>(
        n, nnz, rp, ci, region, root, level, need_level, order, filled, key, key_end, status.dev);
    GKOC_LAUNCH_OK();
    GKOC_TRY(status.read());
    GKOC_TRY(require_checked(status.host));
    *longest = status[st_longest];
    return GKOC_OK;
}

// one sweep or step after the other until one changes nothing; at most n of them.  step(t) launches number t.
template <typename Step>
int bounded_loop(status_words<st_words>& status, int64_t n, long long* done_host, Step&& step)
{
    int* changed_dev = status.dev + st_changed;
    for (int64_t t = 0; t < n; ++t) {
        GKOC_HIP(hipMemsetAsync(changed_dev, 0, sizeof(int), status.st));
        GKOC_TRY(step(t, changed_dev));
        int changed = 0;
        GKOC_HIP(hipMemcpyAsync(&changed, changed_dev, sizeof(int), hipMemcpyDeviceToHost, status.st));
        GKOC_HIP(hipStreamSynchronize(status.st));
        if (!changed) {
            *done_host = t + 1;
            return GKOC_OK;
        }
    }
    set_last_error("%s:%d: %s", __FILE__, __LINE__, "still changing after n iterations: the state is inconsistent");
    return GKOC_E_INVALID;
}

// ------------------------------------------------------------------ components
template <typename I>
__global__ __launch_bounds__(reo_block) void components_init_kernel(int64_t n, const I* __restrict__ region,
                                                                    I* __restrict__ label)
{
    const int64_t stride = int64_t(gridDim.x) * reo_block;
    for (int64_t v = int64_t(blockIdx.x) * reo_block + threadIdx.x; v < n; v += stride) {
        label[v] = int64_t(region[v]) >= 0 ? I(v) : I(-1);
    }
}

template <int W, typename I>
__global__ __launch_bounds__(reo_block) void components_sweep_kernel(
    int64_t n, const I* __restrict__ rp, const I* __restrict__ ci, const I* __restrict__ region,
    const I* __restrict__ before, I* __restrict__ now, int* __restrict__ changed)
{
    constexpr int groups = reo_block / W;
    const int lane = threadIdx.x % W;
    const int64_t stride = int64_t(gridDim.x) * groups;
    for (int64_t row = int64_t(blockIdx.x) * groups + threadIdx.x / W; row < n; row += stride) {
        const int64_t s = region[row];
        const long long mine = before[row];
        long long best = mine;
        if (s >= 0) {
            const int64_t begin = rp[row], end = rp[row + 1];
            for (int64_t k = begin + lane; k < end; k += W) {
                const int64_t u = ci[k];
                if (u != row && int64_t(region[u]) == s) {
                    const long long l = before[u];
                    best = l < best ? l : best;
                }
            }
            best = group_min<W>(best);
        }
        if (lane == 0) {
            now[row] = I(best);
            if (best != mine) *changed = 1;
        }
    }
}

template <typename I>
int reorder_components(gkoc_stream_t s, int64_t n, int64_t nnz, const I* rp, const I* ci, const I* region,
                       I* label, long long* sweeps_host)
{
    GKOC_REQUIRE(n >= 0 && nnz >= 0, GKOC_E_INVALID, "negative size");
    GKOC_REQUIRE(sweeps_host, GKOC_E_INVALID, "null pointer for the result");
    *sweeps_host = 0;
    if (n == 0) return GKOC_OK;
    GKOC_REQUIRE(rp && region && label && (nnz == 0 || ci), GKOC_E_INVALID, "null pointer");
    hipStream_t st = as_stream(s);
    status_words<st_words> status(st);
    GKOC_TRY(status.init(sizeof(I) * size_t(n)));
    int longest = 0;
    const I* none = nullptr;
    GKOC_TRY(reorder_checked<I>(status, n, nnz, rp, ci, region, none, none, 0, none, none, none, 0, &longest));
    I* other = status.template behind<I>();
    components_init_kernel<I><<<dim3(stream_grid(n, reo_block)), dim3(reo_block), 0, st>>>(n, region, label);
    GKOC_LAUNCH_OK();
    // the sweep that changes nothing leaves the same labels in both buffers: the caller's holds the result
    return with_lanes(longest, reorder_row_limits, [&](auto w) {
        constexpr int W = decltype(w)::value;
        return bounded_loop(status, n, sweeps_host, [&](int64_t t, int* changed) {
            const I* from = t % 2 == 0 ? label : other;
            I* to = t % 2 == 0 ? other : label;
            components_sweep_kernel<W, I><<<dim3(stream_grid(n, reo_block / W)), dim3(reo_block), 0, st>>>(
                n, rp, ci, region, from, to, changed);
            GKOC_LAUNCH_OK();
            return GKOC_OK;
        });
    });
}

// ------------------------------------------------------------------ levels
template <typename I>
__global__ __launch_bounds__(reo_block) void levels_init_kernel(int64_t n, const I* __restrict__ region,
                                                                const I* __restrict__ root, I* __restrict__ level)
{
    const int64_t stride = int64_t(gridDim.x) * reo_block;
    for (int64_t v = int64_t(blockIdx.x) * reo_block + threadIdx.x; v < n; v += stride) {
        const int64_t s = region[v];
        level[v] = s >= 0 && int64_t(root[s]) == v ? I(0) : I(-1);
    }
}

// does row `row` store a neighbour of region s whose level is `wanted`?  The same answer in every lane of the group.
template <int W, typename I>
__device__ __forceinline__ int has_neighbour_at(int64_t row, int lane, int64_t s, int64_t wanted,
                                                const I* __restrict__ rp, const I* __restrict__ ci,
                                                const I* __restrict__ region, const I* level)
{
    const int64_t begin = rp[row], end = rp[row + 1];
    // rounds of W entries; the trip count and the exit are uniform in the group
    for (int64_t round = begin; round < end; round += W) {
        const int64_t k = round + lane;
        int hit = 0;
        if (k < end) {
            const int64_t u = ci[k];
            hit = u != row && int64_t(region[u]) == s && int64_t(level[u]) == wanted;
        }
        if (group_any<W>(hit)) return 1;
    }
    return 0;
}

template <int W, typename I>
__global__ __launch_bounds__(reo_block) void level_step_kernel(int64_t n, const I* __restrict__ rp,
                                                               const I* __restrict__ ci,
                                                               const I* __restrict__ region, I* level,
                                                               int64_t current, int* __restrict__ changed)
{
    constexpr int groups = reo_block / W;
    const int lane = threadIdx.x % W;
    const int64_t stride = int64_t(gridDim.x) * groups;
    for (int64_t row = int64_t(blockIdx.x) * groups + threadIdx.x / W; row < n; row += stride) {
        const int64_t s = region[row];
        if (s < 0 || int64_t(level[row]) >= 0) continue;
        if (has_neighbour_at<W, I>(row, lane, s, current, rp, ci, region, level) && lane == 0) {
            level[row] = I(current + 1);
            *changed = 1;
        }
    }
}

template <typename I>
int reorder_levels(gkoc_stream_t s, int64_t n, int64_t nnz, const I* rp, const I* ci, const I* region,
                   const I* root, I* level, long long* steps_host)
{
    GKOC_REQUIRE(n >= 0 && nnz >= 0, GKOC_E_INVALID, "negative size");
    GKOC_REQUIRE(steps_host, GKOC_E_INVALID, "null pointer for the result");
    *steps_host = 0;
    if (n == 0) return GKOC_OK;
    GKOC_REQUIRE(rp && region && root && level && (nnz == 0 || ci), GKOC_E_INVALID, "null pointer");
    hipStream_t st = as_stream(s);
    status_words<st_words> status(st);
    GKOC_TRY(status.init());
    int longest = 0;
    const I* none = nullptr;
    GKOC_TRY(reorder_checked<I>(status, n, nnz, rp, ci, region, root, none, 0, none, none, none, 0, &longest));
    levels_init_kernel<I><<<dim3(stream_grid(n, reo_block)), dim3(reo_block), 0, st>>>(n, region, root, level);
    GKOC_LAUNCH_OK();
    return with_lanes(longest, reorder_row_limits, [&](auto w) {
        constexpr int W = decltype(w)::value;
        return bounded_loop(status, n, steps_host, [&](int64_t t, int* changed) {
            level_step_kernel<W, I><<<dim3(stream_grid(n, reo_block / W)), dim3(reo_block), 0, st>>>(
                n, rp, ci, region, level, t, changed);
            GKOC_LAUNCH_OK();
            return GKOC_OK;
        });
    });
}

// ------------------------------------------------------------------ far roots
// deepest[s] = 1 + the largest level of the region that starts at s (0: no region starts there)
template <typename I>
__global__ __launch_bounds__(reo_block) void deepest_level_kernel(int64_t n, const I* __restrict__ region,
                                                                  const I* __restrict__ level, I* deepest)
{
    const int64_t stride = int64_t(gridDim.x) * reo_block;
    for (int64_t v = int64_t(blockIdx.x) * reo_block + threadIdx.x; v < n; v += stride) {
        const int64_t s = region[v];
        if (s >= 0) atomicMax(as_atomic(deepest + s), atomic_word<I>(int64_t(level[v]) + 1));
    }
}

// smallest[s] (all ones before) = the smallest vertex of that level
template <typename I>
__global__ __launch_bounds__(reo_block) void smallest_deepest_kernel(int64_t n, const I* __restrict__ region,
                                                                     const I* __restrict__ level,
                                                                     const I* __restrict__ deepest, I* smallest)
{
    const int64_t stride = int64_t(gridDim.x) * reo_block;
    for (int64_t v = int64_t(blockIdx.x) * reo_block + threadIdx.x; v < n; v += stride) {
        const int64_t s = region[v];
        if (s >= 0 && int64_t(level[v]) + 1 == int64_t(deepest[s])) {
            atomicMin(as_atomic(smallest + s), atomic_word<I>(v));
        }
    }
}

template <typename I>
__global__ __launch_bounds__(reo_block) void far_roots_kernel(int64_t n, const I* __restrict__ deepest,
                                                              const I* __restrict__ smallest, I* __restrict__ far)
{
    const int64_t stride = int64_t(gridDim.x) * reo_block;
    for (int64_t s = int64_t(blockIdx.x) * reo_block + threadIdx.x; s < n; s += stride) {
        far[s] = int64_t(deepest[s]) > 0 ? smallest[s] : I(-1);
    }
}

template <typename I>
int reorder_far_roots(gkoc_stream_t s, int64_t n, const I* region, const I* level, I* far)
{
    GKOC_REQUIRE(n >= 0, GKOC_E_INVALID, "negative size");
    if (n == 0) return GKOC_OK;
    GKOC_REQUIRE(region && level && far, GKOC_E_INVALID, "null pointer");
    hipStream_t st = as_stream(s);
    const size_t words = sizeof(I) * size_t(n);
    status_words<st_words> status(st);
    GKOC_TRY(status.init(2 * words));
    int longest = 0;
    const I* none = nullptr;
    GKOC_TRY(reorder_checked<I>(status, n, 0, none, none, region, none, level, 1, none, none, none, 0, &longest));
    I* deepest = status.template behind<I>();
    I* smallest = deepest + n;
    GKOC_HIP(hipMemsetAsync(deepest, 0, words, st));
    GKOC_HIP(hipMemsetAsync(smallest, 0xff, words, st));
    const dim3 grid(stream_grid(n, reo_block)), block(reo_block);
    deepest_level_kernel<I><<<grid, block, 0, st>>>(n, region, level, deepest);
    GKOC_LAUNCH_OK();
    smallest_deepest_kernel<I><<<grid, block, 0, st>>>(n, region, level, deepest, smallest);
    GKOC_LAUNCH_OK();
    far_roots_kernel<I><<<grid, block, 0, st>>>(n, deepest, smallest, far);
    GKOC_LAUNCH_OK();
    GKOC_HIP(hipStreamSynchronize(st));     // the scratch ends here
    return GKOC_OK;
}

// ------------------------------------------------------------------ split
// hist[s + level] = the vertices of that level in the region that starts at s (the slot is inside: checked)
template <typename I>
__global__ __launch_bounds__(reo_block) void level_histogram_kernel(int64_t n, const I* __restrict__ region,
                                                                    const I* __restrict__ level, I* hist)
{
    const int64_t stride = int64_t(gridDim.x) * reo_block;
    for (int64_t v = int64_t(blockIdx.x) * reo_block + threadIdx.x; v < n; v += stride) {
        const int64_t s = region[v];
        if (s >= 0) atomicAdd(as_atomic(hist + s + int64_t(level[v])), atomic_word<I>(1));
    }
}

// size[s] = |R| from the last position of the segment that starts at s
template <typename I>
__global__ __launch_bounds__(reo_block) void segment_sizes_kernel(int64_t n, const I* __restrict__ order,
                                                                  const I* __restrict__ region,
                                                                  I* __restrict__ size)
{
    const int64_t stride = int64_t(gridDim.x) * reo_block;
    for (int64_t p = int64_t(blockIdx.x) * reo_block + threadIdx.x; p < n; p += stride) {
        const int64_t s = region[order[p]];
        if (s < 0 || s > p) continue;
        if (p == n - 1 || int64_t(region[order[p + 1]]) != s) size[s] = I(p + 1 - s);
    }
}

// position p = s + L is the slot of level L: hmax[s] = the last level that has vertices, mstar[s] = the level at
// which the running count reaches ceil(|R| / 2).  before[] is the exclusive scan of hist[].
template <typename I>
__global__ __launch_bounds__(reo_block) void median_level_kernel(
    int64_t n, const I* __restrict__ order, const I* __restrict__ region, const I* __restrict__ hist,
    const I* __restrict__ before, const I* __restrict__ size, I* __restrict__ mstar, I* __restrict__ hmax)
{
    const int64_t stride = int64_t(gridDim.x) * reo_block;
    for (int64_t p = int64_t(blockIdx.x) * reo_block + threadIdx.x; p < n; p += stride) {
        const int64_t s = region[order[p]];
        if (s < 0 || s > p) continue;
        const int64_t count = hist[p];
        if (count <= 0) continue;
        const int64_t below = int64_t(before[p]) - int64_t(before[s]);
        const int64_t half = (int64_t(size[s]) + 1) / 2;
        if (below < half && half <= below + count) mstar[s] = I(p - s);
        if (p + 1 >= s + int64_t(size[s]) || p + 1 >= n || int64_t(hist[p + 1]) == 0) hmax[s] = I(p - s);
    }
}

template <int W, typename I>
__global__ __launch_bounds__(reo_block) void split_class_kernel(
    int64_t n, const I* __restrict__ rp, const I* __restrict__ ci, const I* __restrict__ region,
    const I* __restrict__ level, const I* __restrict__ mstar, const I* __restrict__ hmax, I* __restrict__ cls)
{
    constexpr int groups = reo_block / W;
    const int lane = threadIdx.x % W;
    const int64_t stride = int64_t(gridDim.x) * groups;
    for (int64_t row = int64_t(blockIdx.x) * groups + threadIdx.x / W; row < n; row += stride) {
        const int64_t s = region[row];
        int c = -1;
        if (s >= 0) {
            const int64_t h = hmax[s];
            if (h < 2) {
                c = 3;
            } else {
                const int64_t ms = mstar[s];
                const int64_t m = ms < 1 ? 1 : (ms > h - 1 ? h - 1 : ms);
                const int64_t l = level[row];
                if (l != m) {
                    c = l < m ? 0 : 1;
                } else {
                    c = has_neighbour_at<W, I>(row, lane, s, m + 1, rp, ci, region, level) ? 2 : 0;
                }
            }
        }
        if (lane == 0) cls[row] = I(c);
    }
}

template <typename I>
int reorder_split(gkoc_stream_t s, int64_t n, int64_t nnz, const I* rp, const I* ci, const I* order,
                  const I* region, const I* level, I* cls)
{
    GKOC_REQUIRE(n >= 0 && nnz >= 0, GKOC_E_INVALID, "negative size");
    if (n == 0) return GKOC_OK;
    GKOC_REQUIRE(rp && order && region && level && cls && (nnz == 0 || ci), GKOC_E_INVALID, "null pointer");
    hipStream_t st = as_stream(s);
    const size_t words = sizeof(I) * size_t(n);
    status_words<st_words> status(st);
    GKOC_TRY(status.init(6 * words));
    I* pos = status.template behind<I>();
    I *hist = pos + n, *before = hist + n, *size = before + n, *mstar = size + n, *hmax = mstar + n;
    const dim3 grid(stream_grid(n, reo_block)), block(reo_block);
    GKOC_HIP(hipMemsetAsync(pos, 0xff, words, st));
    scatter_positions_kernel<I><<<grid, block, 0, st>>>(n, order, pos);
    GKOC_LAUNCH_OK();
    int longest = 0;
    const I* none = nullptr;
    GKOC_TRY(reorder_checked<I>(status, n, nnz, rp, ci, region, none, level, 1, order, pos, none, 0, &longest));
    GKOC_HIP(hipMemsetAsync(hist, 0, 5 * words, st));
    level_histogram_kernel<I><<<grid, block, 0, st>>>(n, region, level, hist);
    GKOC_LAUNCH_OK();
    GKOC_HIP(hipMemcpyAsync(before, hist, words, hipMemcpyDeviceToDevice, st));
    GKOC_TRY(device_exclusive_scan<I>(st, before, n));
    segment_sizes_kernel<I><<<grid, block, 0, st>>>(n, order, region, size);
    GKOC_LAUNCH_OK();
    median_level_kernel<I><<<grid, block, 0, st>>>(n, order, region, hist, before, size, mstar, hmax);
    GKOC_LAUNCH_OK();
    GKOC_TRY(with_lanes(longest, reorder_row_limits, [&](auto w) {
        constexpr int W = decltype(w)::value;
        split_class_kernel<W, I><<<dim3(stream_grid(n, reo_block / W)), block, 0, st>>>(n, rp, ci, region, level,
                                                                                       mstar, hmax, cls);
        GKOC_LAUNCH_OK();
        return GKOC_OK;
    }));
    GKOC_HIP(hipStreamSynchronize(st));     // the scratch ends here
    return GKOC_OK;
}

// ------------------------------------------------------------------ regroup
// per vertex: the two sort keys and the identity the first sort starts from.  A final vertex keeps its place:
// its segment key is its own position, which lies in no live segment.
template <typename I>
__global__ __launch_bounds__(reo_block) void regroup_keys_kernel(int64_t n, const I* __restrict__ region,
                                                                 const I* __restrict__ pos,
                                                                 const I* __restrict__ key,
                                                                 I* __restrict__ segment_key,
                                                                 I* __restrict__ inner_key, I* __restrict__ iota)
{
    const int64_t stride = int64_t(gridDim.x) * reo_block;
    for (int64_t v = int64_t(blockIdx.x) * reo_block + threadIdx.x; v < n; v += stride) {
        const bool live = int64_t(region[v]) >= 0;
        segment_key[v] = live ? region[v] : pos[v];
        inner_key[v] = live ? key[v] : I(0);
        iota[v] = I(v);
    }
}

template <typename I>
__global__ __launch_bounds__(reo_block) void gather_kernel(int64_t n, const I* __restrict__ from,
                                                           const I* __restrict__ index, I* __restrict__ out)
{
    const int64_t stride = int64_t(gridDim.x) * reo_block;
    for (int64_t i = int64_t(blockIdx.x) * reo_block + threadIdx.x; i < n; i += stride) out[i] = from[index[i]];
}

// head[p] = 1 where a run of equal (segment key, inner key) starts; count[p] the same, to be scanned
template <typename I>
__global__ __launch_bounds__(reo_block) void run_heads_kernel(int64_t n, const I* __restrict__ sorted_segment,
                                                              const I* __restrict__ sorted,
                                                              const I* __restrict__ inner_key,
                                                              I* __restrict__ head, I* __restrict__ count)
{
    const int64_t stride = int64_t(gridDim.x) * reo_block;
    for (int64_t p = int64_t(blockIdx.x) * reo_block + threadIdx.x; p < n; p += stride) {
        const bool first = p == 0 || sorted_segment[p] != sorted_segment[p - 1] ||
                           inner_key[sorted[p]] != inner_key[sorted[p - 1]];
        head[p] = I(first);
        count[p] = I(first);
    }
}

// starts[r] = the position where run r begins, starts[number of runs] = n
template <typename I>
__global__ __launch_bounds__(reo_block) void run_starts_kernel(int64_t n, const I* __restrict__ head,
                                                               const I* __restrict__ runs_before,
                                                               I* __restrict__ starts)
{
    const int64_t stride = int64_t(gridDim.x) * reo_block;
    for (int64_t p = int64_t(blockIdx.x) * reo_block + threadIdx.x; p < n; p += stride) {
        const int64_t r = runs_before[p];
        if (r < 0 || r >= n) continue;
        if (int64_t(head[p])) starts[r] = I(p);
        if (p == n - 1) starts[r + int64_t(head[p])] = I(n);
    }
}

template <typename I>
__global__ __launch_bounds__(reo_block) void regroup_assign_kernel(
    int64_t n, int64_t leaf_size, int64_t final_from, const I* __restrict__ sorted, const I* __restrict__ head,
    const I* __restrict__ runs_before, const I* __restrict__ starts, const I* __restrict__ key,
    I* __restrict__ order, I* region, unsigned long long* __restrict__ live)
{
    const int64_t stride = int64_t(gridDim.x) * reo_block;
    unsigned long long mine = 0;
    for (int64_t p = int64_t(blockIdx.x) * reo_block + threadIdx.x; p < n; p += stride) {
        const int64_t v = sorted[p];
        const int64_t r = int64_t(runs_before[p]) + int64_t(head[p]) - 1;
        bool final = true;
        int64_t start = -1;
        if (r >= 0 && r < n && int64_t(region[v]) >= 0 && int64_t(key[v]) < final_from) {
            start = starts[r];
            final = int64_t(starts[r + 1]) - start <= leaf_size;
        }
        region[v] = final ? I(-1) : I(start);
        order[p] = I(v);
        mine += final ? 0 : 1;
    }
#pragma unroll
    for (int off = wave_size / 2; off > 0; off >>= 1) mine += __shfl_xor(mine, off, wave_size);
    if ((threadIdx.x & (wave_size - 1)) == 0 && mine) atomicAdd(live, mine);
}

inline int key_bits(int64_t n)
{
    int bits = 3;       // keys below max(n, 4)
    while (bits < 63 && (int64_t(1) << bits) < n) ++bits;
    return bits;
}

inline size_t aligned(size_t bytes) { return (bytes + 255) / 256 * 256; }

template <typename I>
int reorder_regroup(gkoc_stream_t s, int64_t n, int64_t leaf_size, int64_t final_from, const I* key, I* order,
                    I* region, long long* live_host)
{
    GKOC_REQUIRE(n >= 0, GKOC_E_INVALID, "negative size");
    GKOC_REQUIRE(leaf_size >= 1, GKOC_E_INVALID, "leaf_size < 1");
    GKOC_REQUIRE(live_host, GKOC_E_INVALID, "null pointer for the result");
    *live_host = 0;
    if (n == 0) return GKOC_OK;
    GKOC_REQUIRE(key && order && region, GKOC_E_INVALID, "null pointer");
    hipStream_t st = as_stream(s);
    const int bits = key_bits(n);
    size_t sort_bytes = 0;
    {
        I* p = nullptr;
        GKOC_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, p, p, p, p, size_t(n), 0, bits, st));
    }
    // scratch: eleven arrays of n (+ 1) words, the live counter, the sort's own
    const size_t words = aligned(sizeof(I) * size_t(n + 1));
    status_words<st_words> status(st);
    GKOC_TRY(status.init(256 + 11 * words + 256 + aligned(sort_bytes)));
    char* base = status.template behind<char>();
    base += (256 - reinterpret_cast<uintptr_t>(base) % 256) % 256;      // the sort's scratch on a 256-byte boundary
    auto array = [&](int k) { return reinterpret_cast<I*>(base + size_t(k) * words); };
    I *pos = array(0), *segment_key = array(1), *inner_key = array(2), *iota = array(3), *inner_sorted = array(4),
      *by_inner = array(5), *segment_gathered = array(6), *segment_sorted = array(7), *sorted = array(8),
      *head = array(9), *runs_before = array(10);
    I* starts = pos;        // pos is read for the last time before the sorts
    auto* live = reinterpret_cast<unsigned long long*>(base + 11 * words);
    void* sort_scratch = base + 11 * words + 256;
    const dim3 grid(stream_grid(n, reo_block)), block(reo_block);
    GKOC_HIP(hipMemsetAsync(pos, 0xff, sizeof(I) * size_t(n), st));
    scatter_positions_kernel<I><<<grid, block, 0, st>>>(n, order, pos);
    GKOC_LAUNCH_OK();
    int longest = 0;
    const I* none = nullptr;
    GKOC_TRY(reorder_checked<I>(status, n, 0, none, none, region, none, none, 0, order, pos, key, n > 4 ? n : 4,
                                &longest));
    regroup_keys_kernel<I><<<grid, block, 0, st>>>(n, region, pos, key, segment_key, inner_key, iota);
    GKOC_LAUNCH_OK();
    // LSD: the vertices are ascending to begin with, then stably by the inner key, then stably by the segment
    GKOC_HIP(rocprim::radix_sort_pairs(sort_scratch, sort_bytes, inner_key, inner_sorted, iota, by_inner, size_t(n),
                                       0, bits, st));
    gather_kernel<I><<<grid, block, 0, st>>>(n, segment_key, by_inner, segment_gathered);
    GKOC_LAUNCH_OK();
    GKOC_HIP(rocprim::radix_sort_pairs(sort_scratch, sort_bytes, segment_gathered, segment_sorted, by_inner, sorted,
                                       size_t(n), 0, bits, st));
    run_heads_kernel<I><<<grid, block, 0, st>>>(n, segment_sorted, sorted, inner_key, head, runs_before);
    GKOC_LAUNCH_OK();
    GKOC_TRY(device_exclusive_scan<I>(st, runs_before, n));
    run_starts_kernel<I><<<grid, block, 0, st>>>(n, head, runs_before, starts);
    GKOC_LAUNCH_OK();
    GKOC_HIP(hipMemsetAsync(live, 0, sizeof(unsigned long long), st));
    regroup_assign_kernel<I><<<grid, block, 0, st>>>(n, leaf_size, final_from, sorted, head, runs_before, starts,
                                                    key, order, region, live);
    GKOC_LAUNCH_OK();
    unsigned long long count = 0;
    GKOC_HIP(hipMemcpyAsync(&count, live, sizeof(count), hipMemcpyDeviceToHost, st));
    GKOC_HIP(hipStreamSynchronize(st));     // the scratch ends here
    *live_host = (long long)(count);
    return GKOC_OK;
}

}  // namespace
}  // namespace gkoc

using namespace gkoc;

extern "C" int gkoc_reorder_row_limits(int* limits_host, int* count_host)
{
    return export_row_limits(reorder_row_limits, limits_host, count_host);
}

#define GKOC_DEF_REORDER(I, A, IN)                                                                               \
    extern "C" int gkoc_reorder_components_##IN(gkoc_stream_t s, int64_t n, int64_t nnz, const I* row_ptrs,      \
                                                const I* col_idxs, const I* region, A* label,                    \
                                                long long* sweeps_host)                                          \
    {                                                                                                            \
        return reorder_components<I>(s, n, nnz, row_ptrs, col_idxs, region, label, sweeps_host);                 \
    }                                                                                                            \
    extern "C" int gkoc_reorder_levels_##IN(gkoc_stream_t s, int64_t n, int64_t nnz, const I* row_ptrs,          \
                                            const I* col_idxs, const I* region, const I* root, A* level,         \
                                            long long* steps_host)                                               \
    {                                                                                                            \
        return reorder_levels<I>(s, n, nnz, row_ptrs, col_idxs, region, root, level, steps_host);                \
    }                                                                                                            \
    extern "C" int gkoc_reorder_far_roots_##IN(gkoc_stream_t s, int64_t n, const I* region, const I* level,      \
                                               A* far)                                                           \
    {                                                                                                            \
        return reorder_far_roots<I>(s, n, region, level, far);                                                   \
    }                                                                                                            \
    extern "C" int gkoc_reorder_split_##IN(gkoc_stream_t s, int64_t n, int64_t nnz, const I* row_ptrs,           \
                                           const I* col_idxs, const I* order, const I* region, const I* level,   \
                                           A* cls)                                                               \
    {                                                                                                            \
        return reorder_split<I>(s, n, nnz, row_ptrs, col_idxs, order, region, level, cls);                       \
    }                                                                                                            \
    extern "C" int gkoc_reorder_regroup_##IN(gkoc_stream_t s, int64_t n, int64_t leaf_size, int64_t final_from,  \
                                             const I* key, A* order, A* region, long long* live_host)            \
    {                                                                                                            \
        return reorder_regroup<I>(s, n, leaf_size, final_from, key, order, region, live_host);                   \
    }
GKOC_DEF_REORDER(int32_t, gkoc_reorder_i32, i32)
GKOC_DEF_REORDER(int64_t, gkoc_reorder_i64, i64)
