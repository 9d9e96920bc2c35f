// Symbolic Cholesky: the fill pattern of L for a symmetric pattern S (factorization::Cholesky / Lu).
//   symbolic_forest            elimination forest, postorder and first descendants (host, like trs_generate)
//   symbolic_post_keys         S's lower triangle with post[col] in place of col, and post^-1
//   symbolic_cholesky_count    triplets per row of L -> int64 offsets and their total
//   symbolic_cholesky_expand   the entries (row, col, 1) of L as matrix_data entries, unordered inside a row
//
// Contract (integer-exact, include/gko_cdna4.h "Symbolic Cholesky / sparse direct"): row i of L holds i and every
// j < i that S's fill path reaches, which is the row subtree of i in the elimination forest: the union of the
// paths p, parent[p], ... from every strictly-lower neighbour p of i up to (not including) i.
//
// Skeleton rule: with the neighbours ordered by post rank, p_1 < ... < p_k, the path from p_t is cut where it
// meets the path from p_{t+1} (from i for t = k), that is at the first node that is an ancestor of p_{t+1}:
// a is an ancestor of q  <=>  first[a] <= post[q] <= post[a].  The pieces are disjoint and their union is the
// row subtree, so the walks of one row need no marks, and every node of L costs one parent look-up.
//
// Kernels: one group of W = 16 / 32 / 64 lanes per row (W from the longest row of the call, limits in
// symbolic_row_limits), lane = stored strictly-lower entry, rows spread over the grid.  A row with more lower
// entries than W (W is 64 then) is streamed in rounds of W entries.  count folds the lanes' path lengths by
// group shuffles; expand counts again, gives every lane its place by a group scan and walks a second time.
//
// Invariants:
//   1. every output word is written by exactly one lane; no atomics, no marks, no shared scratch;
//   2. a walk stops at the latest at row i and follows parent[v] > v only (checked before), so it ends;
//   3. expand writes an entry only at a position inside [0, total);
//   4. no entry writes an index array of a matrix, like the aggregation state of pgm.hip: the forest arrays, the
//      keys, post^-1 and the offsets are state of the symbolic factorization (gkoc_symbolic_i32 / _i64 in the
//      header), and the pattern leaves as matrix_data entries, which become index arrays only through
//      gkoc_aos_to_soa and gkoc_sort_row_major.
#include <hip/hip_runtime.h>

#include <climits>
#include <vector>

#include "common.hpp"
#include "scan.hpp"
#include "sparse_rows.hpp"

namespace gkoc {
namespace {

constexpr int symb_row_limits[] = {16, 32, 64};
constexpr int symb_block = 256;

// ------------------------------------------------------------------ checks (one thread per row / vertex)
// status[0]: row pointers or columns (keys) out of range, [1]: parent, [2]: post / inv_post, [3]: the longest row,
// [4]: a row that is empty or (with_last) does not end with post[row].  Every array may be null: its check is
// skipped.  inv is checked against post (post[inv[r]] == r for every r makes both permutations); without inv
// the caller has scattered post into a -1-filled `filled` and every word of it must have been written.
template <typename I>
__global__ __launch_bounds__(symb_block) void symbolic_check_kernel(
    int64_t n, int64_t nnz, const I* __restrict__ rp, const I* __restrict__ ci, const I* __restrict__ parent,
    const I* __restrict__ post, const I* __restrict__ inv, const I* __restrict__ filled, int with_last,
    int* __restrict__ status)
{
    const int64_t stride = int64_t(gridDim.x) * symb_block;
    int longest = 0;
    for (int64_t row = int64_t(blockIdx.x) * symb_block + threadIdx.x; row < n; row += stride) {
        bool post_ok = true;
        if (post) {
            const int64_t p = post[row];
            post_ok = p >= 0 && p < n;
            if (!post_ok) status[2] = 1;
        }
        if (inv) {
            const int64_t v = inv[row];
            if (v < 0 || v >= n || int64_t(post[v]) != row) status[2] = 1;
        }
        if (filled && int64_t(filled[row]) < 0) status[2] = 1;
        if (parent) {
            const int64_t p = parent[row];
            if (p != -1 && (p <= row || p >= n)) status[1] = 1;
        }
        if (rp) {
            const int64_t begin = rp[row], end = rp[row + 1];
            if (begin < 0 || end < begin || end > nnz || (row == 0 && begin != 0) || (row == n - 1 && end != nnz)) {
                status[0] = 1;
            } else {
                for (int64_t k = begin; k < end; ++k) {
                    const int64_t col = ci[k];
                    if (col < 0 || col >= n) status[0] = 1;
                }
                if (with_last && (end == begin || !post_ok || int64_t(ci[end - 1]) != int64_t(post[row]))) {
                    status[4] = 1;
                }
                const int64_t len = end - begin;
                longest = len > longest ? int(len > INT_MAX ? INT_MAX : len) : longest;
            }
        }
    }
    note_longest(longest, &status[3]);
}

// filled[post[v]] = v wherever post[v] is inside [0, n) (the check kernel reports the others)
template <typename I>
__global__ __launch_bounds__(symb_block) void symbolic_scatter_kernel(int64_t n, const I* __restrict__ post,
                                                                      I* __restrict__ filled)
{
    const int64_t stride = int64_t(gridDim.x) * symb_block;
    for (int64_t v = int64_t(blockIdx.x) * symb_block + threadIdx.x; v < n; v += stride) {
        const int64_t p = post[v];
        if (p >= 0 && p < n) filled[p] = I(v);
    }
}

template <typename I>
__global__ __launch_bounds__(symb_block) void symbolic_keys_kernel(int64_t nnz, const I* __restrict__ ci,
                                                                   const I* __restrict__ post, I* __restrict__ keys)
{
    const int64_t stride = int64_t(gridDim.x) * symb_block;
    for (int64_t k = int64_t(blockIdx.x) * symb_block + threadIdx.x; k < nnz; k += stride) keys[k] = post[ci[k]];
}

// ------------------------------------------------------------------ the walks
// gko::matrix_data_entry<T, I> with natural alignment, the layout of gkoc_soa_to_aos / gkoc_aos_to_soa
template <typename T, typename I>
struct pattern_entry {
    I row;
    I column;
    T value;
};

// the nodes of the path from `a` that are below `row` and no ancestor of the node of post rank `bound`
template <bool WRITE, typename T, typename I>
__device__ __forceinline__ int64_t walk(int64_t a, int64_t bound, int64_t row, const I* __restrict__ parent,
                                        const I* __restrict__ post, const I* __restrict__ first, int64_t pos,
                                        int64_t total, pattern_entry<T, I>* __restrict__ entries)
{
    int64_t count = 0;
    while (a >= 0 && a < row && !(int64_t(first[a]) <= bound && bound <= int64_t(post[a]))) {
        if (WRITE) {
            const int64_t p = pos + count;
            if (p >= 0 && p < total) entries[p] = pattern_entry<T, I>{I(row), I(a), T(1)};
        }
        ++count;
        a = parent[a];
    }
    return count;
}

// one row by one group of W lanes; `lane` in [0, W).  (rp, keys): the post ranks of the row's strictly-lower
// neighbours ascending, then post[row] - the bound of the last lane.
template <bool EXPAND, int W, typename T, typename I>
__device__ __forceinline__ void symbolic_row(int64_t row, int lane, const I* __restrict__ rp,
                                             const I* __restrict__ keys, const I* __restrict__ parent,
                                             const I* __restrict__ post, const I* __restrict__ first,
                                             const I* __restrict__ inv_post, int64_t* __restrict__ counts,
                                             const int64_t* __restrict__ offsets, int64_t total,
                                             pattern_entry<T, I>* __restrict__ entries)
{
    const int64_t begin = rp[row];
    const int64_t n_lower = int64_t(rp[row + 1]) - begin - 1;
    int64_t base = EXPAND ? offsets[row] : 0;
    int64_t mine = 0;
    // rounds of W entries: one for a row within the limit, the group's trip count is uniform
    for (int64_t round = 0; round < n_lower; round += W) {
        const int64_t t = round + lane;
        const bool active = t < n_lower;
        const int64_t start = active ? int64_t(inv_post[keys[begin + t]]) : -1;
        const int64_t bound = active ? int64_t(keys[begin + t + 1]) : 0;
        const int64_t len = walk<false, T, I>(start, bound, row, parent, post, first, 0, 0, nullptr);
        if (!EXPAND) {
            mine += len;
        } else {
            long long incl = len;
#pragma unroll
            for (int off = 1; off < W; off <<= 1) {
                const long long o = __shfl_up(incl, off, W);
                if (lane >= off) incl += o;
            }
            walk<true, T, I>(start, bound, row, parent, post, first, base + incl - len, total, entries);
            base += __shfl(incl, W - 1, W);
        }
    }
    if (EXPAND) {
        if (lane == 0 && base >= 0 && base < total) entries[base] = pattern_entry<T, I>{I(row), I(row), T(1)};
    } else {
        const long long sum = group_sum<W>((long long)(mine));
        if (lane == 0) counts[row] = sum + 1;
    }
}

template <bool EXPAND, int W, typename T, typename I>
__global__ __launch_bounds__(symb_block) void symbolic_rows_kernel(
    int64_t n, const I* __restrict__ rp, const I* __restrict__ keys, const I* __restrict__ parent,
    const I* __restrict__ post, const I* __restrict__ first, const I* __restrict__ inv_post,
    int64_t* __restrict__ counts, const int64_t* __restrict__ offsets, int64_t total,
    pattern_entry<T, I>* __restrict__ entries)
{
    constexpr int groups = symb_block / W;
    const int lane = threadIdx.x % W;
    const int64_t stride = int64_t(gridDim.x) * groups;
    for (int64_t row = int64_t(blockIdx.x) * groups + threadIdx.x / W; row < n; row += stride) {
        symbolic_row<EXPAND, W, T, I>(row, lane, rp, keys, parent, post, first, inv_post, counts, offsets, total,
                                      entries);
    }
    if (!EXPAND && blockIdx.x == 0 && threadIdx.x == 0) counts[n] = 0;
}

template <bool EXPAND, int W, typename T, typename I>
int symbolic_rows_launch(hipStream_t st, int64_t n, const I* rp, const I* keys, const I* parent, const I* post,
                         const I* first, const I* inv_post, int64_t* counts, const int64_t* offsets, int64_t total,
                         pattern_entry<T, I>* entries)
{
    symbolic_rows_kernel<EXPAND, W, T, I><<<dim3(stream_grid(n, symb_block / W)), dim3(symb_block), 0, st>>>(
        n, rp, keys, parent, post, first, inv_post, counts, offsets, total, entries);
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

// the checks of count and expand: everything the walks index with.  *longest_lower = the most strictly-lower
// entries of a row.  Synchronises the stream.
template <typename I>
int symbolic_checked(hipStream_t st, int64_t n, int64_t nnz, const I* rp, const I* keys, const I* parent,
                     const I* post, const I* inv_post, int* longest_lower)
{
    status_words<5> status(st);
    GKOC_TRY(status.init());
    symbolic_check_kernel<I><<<dim3(stream_grid(n, symb_block)), dim3(symb_block), 0, st>>>(
        n, nnz, rp, keys, parent, post, inv_post, static_cast<const I*>(nullptr), 1, status.dev);
    GKOC_LAUNCH_OK();
    GKOC_TRY(status.read());
    GKOC_REQUIRE(status[0] == 0, GKOC_E_INVALID, "row pointers do not ascend from 0 to nnz, or a key outside [0, n)");
    GKOC_REQUIRE(status[1] == 0, GKOC_E_INVALID, "parent[v] is neither -1 nor inside (v, n)");
    GKOC_REQUIRE(status[2] == 0, GKOC_E_INVALID, "post is no permutation with the inverse inv_post");
    GKOC_REQUIRE(status[4] == 0, GKOC_E_INVALID, "a row that does not end with the post rank of its diagonal");
    *longest_lower = status[3] - 1;
    return GKOC_OK;
}

template <bool EXPAND, typename T, typename I>
int symbolic_rows(gkoc_stream_t s, int64_t n, int64_t nnz, const I* rp, const I* keys, const I* parent,
                  const I* post, const I* first, const I* inv_post, int64_t* counts, const int64_t* offsets,
                  int64_t total, pattern_entry<T, I>* entries)
{
    hipStream_t st = as_stream(s);
    int longest = 0;
    GKOC_TRY(symbolic_checked<I>(st, n, nnz, rp, keys, parent, post, inv_post, &longest));
    return with_lanes(longest, symb_row_limits, [&](auto w) {
        return symbolic_rows_launch<EXPAND, decltype(w)::value, T, I>(st, n, rp, keys, parent, post, first, inv_post,
                                                                      counts, offsets, total, entries);
    });
}

template <typename I>
int symbolic_count(gkoc_stream_t s, int64_t n, int64_t nnz, const I* rp, const I* keys, const I* parent,
                   const I* post, const I* first, const I* inv_post, int64_t* offsets, long long* total_host)
{
    GKOC_REQUIRE(n >= 0 && nnz >= 0, GKOC_E_INVALID, "negative size");
    GKOC_REQUIRE(total_host, GKOC_E_INVALID, "null pointer for the result");
    if (n == 0) {
        *total_host = 0;
        if (offsets) GKOC_HIP(hipMemsetAsync(offsets, 0, 8, as_stream(s)));
        return GKOC_OK;
    }
    GKOC_REQUIRE(rp && keys && parent && post && first && inv_post && offsets, GKOC_E_INVALID, "null pointer");
    // (the value type only shapes expand's entries; count writes none)
    GKOC_TRY((symbolic_rows<false, float, I>(s, n, nnz, rp, keys, parent, post, first, inv_post, offsets, nullptr, 0,
                                             nullptr)));
    GKOC_TRY(device_exclusive_scan<int64_t>(as_stream(s), offsets, n + 1));
    int64_t total = 0;
    GKOC_HIP(hipMemcpyAsync(&total, offsets + n, 8, hipMemcpyDeviceToHost, as_stream(s)));
    GKOC_HIP(hipStreamSynchronize(as_stream(s)));
    *total_host = total;
    return GKOC_OK;
}

template <typename T, typename I>
int symbolic_expand(gkoc_stream_t s, int64_t n, int64_t nnz, const I* rp, const I* keys, const I* parent,
                    const I* post, const I* first, const I* inv_post, const int64_t* offsets, int64_t total,
                    void* entries)
{
    GKOC_REQUIRE(n >= 0 && nnz >= 0 && total >= 0, GKOC_E_INVALID, "negative size");
    if (n == 0) return GKOC_OK;
    GKOC_REQUIRE(rp && keys && parent && post && first && inv_post && offsets && entries, GKOC_E_INVALID,
                 "null pointer");
    return symbolic_rows<true, T, I>(s, n, nnz, rp, keys, parent, post, first, inv_post, nullptr, offsets, total,
                                     static_cast<pattern_entry<T, I>*>(entries));
}

template <typename I>
int symbolic_post_keys(gkoc_stream_t s, int64_t n, int64_t nnz, const I* rp, const I* ci, const I* post, I* keys,
                       I* inv_post)
{
    GKOC_REQUIRE(n >= 0 && nnz >= 0, GKOC_E_INVALID, "negative size");
    if (n == 0) return GKOC_OK;
    GKOC_REQUIRE(rp && post && inv_post && (nnz == 0 || (ci && keys)), GKOC_E_INVALID, "null pointer");
    hipStream_t st = as_stream(s);
    // scratch: the status words, then post^-1 - the caller's inv_post is written only after the checks
    status_words<5> status(st);
    GKOC_TRY(status.init(sizeof(I) * size_t(n)));
    I* filled = status.template behind<I>();
    GKOC_HIP(hipMemsetAsync(filled, 0xff, sizeof(I) * size_t(n), st));
    symbolic_scatter_kernel<I><<<dim3(stream_grid(n, symb_block)), dim3(symb_block), 0, st>>>(n, post, filled);
    GKOC_LAUNCH_OK();
    symbolic_check_kernel<I><<<dim3(stream_grid(n, symb_block)), dim3(symb_block), 0, st>>>(
        n, nnz, rp, ci, static_cast<const I*>(nullptr), post, static_cast<const I*>(nullptr), filled, 0, status.dev);
    GKOC_LAUNCH_OK();
    GKOC_TRY(status.read());
    GKOC_REQUIRE(status[0] == 0, GKOC_E_INVALID, "row pointers do not ascend from 0 to nnz, or a column outside the matrix");
    GKOC_REQUIRE(status[2] == 0, GKOC_E_INVALID, "post is no permutation of [0, n)");
    GKOC_HIP(hipMemcpyAsync(inv_post, filled, sizeof(I) * size_t(n), hipMemcpyDeviceToDevice, st));
    if (nnz > 0) {
        symbolic_keys_kernel<I><<<dim3(stream_grid(nnz, symb_block)), dim3(symb_block), 0, st>>>(nnz, ci, post, keys);
        GKOC_LAUNCH_OK();
    }
    return GKOC_OK;
}

// ------------------------------------------------------------------ the forest (host, O(nnz alpha))
// Liu's algorithm with path compression over the entries left of the diagonal; children in ascending index,
// so the postorder is fixed; first[v] = post[v] - (size of v's subtree) + 1.
template <typename I>
int symbolic_forest(gkoc_stream_t s, int64_t n, int64_t nnz, const I* row_ptrs, const I* col_idxs, I* parent_dev,
                    I* post_dev, I* first_dev)
{
    GKOC_REQUIRE(n >= 0 && nnz >= 0, GKOC_E_INVALID, "negative size");
    if (n == 0) return GKOC_OK;
    GKOC_REQUIRE(row_ptrs && parent_dev && post_dev && first_dev && (nnz == 0 || col_idxs), GKOC_E_INVALID,
                 "null pointer");
    hipStream_t st = as_stream(s);
    std::vector<I> rp(size_t(n) + 1, I(0)), ci;
    GKOC_HIP(hipMemcpyAsync(rp.data(), row_ptrs, sizeof(I) * size_t(n + 1), hipMemcpyDeviceToHost, st));
    GKOC_HIP(hipStreamSynchronize(st));
    GKOC_REQUIRE(rp[0] == 0 && int64_t(rp[n]) == nnz, GKOC_E_INVALID, "row pointers do not run from 0 to nnz");
    for (int64_t r = 0; r < n; ++r) {
        GKOC_REQUIRE(rp[r] <= rp[r + 1], GKOC_E_INVALID, "row pointers do not ascend");
    }
    if (nnz > 0) {
        ci.resize(size_t(nnz));
        GKOC_HIP(hipMemcpyAsync(ci.data(), col_idxs, sizeof(I) * size_t(nnz), hipMemcpyDeviceToHost, st));
        GKOC_HIP(hipStreamSynchronize(st));
    }
    for (int64_t k = 0; k < nnz; ++k) {
        GKOC_REQUIRE(ci[k] >= 0 && int64_t(ci[k]) < n, GKOC_E_INVALID, "column index outside the matrix");
    }
    std::vector<I> parent(size_t(n), I(-1)), post(size_t(n), I(0)), first(size_t(n), I(0));
    std::vector<int64_t> ancestor(size_t(n), -1);
    for (int64_t i = 0; i < n; ++i) {
        for (int64_t k = rp[i]; k < rp[i + 1]; ++k) {
            for (int64_t r = ci[k]; r != -1 && r < i;) {
                const int64_t next = ancestor[r];
                ancestor[r] = i;
                if (next == -1) parent[r] = I(i);
                r = next;
            }
        }
    }
    // child lists, ascending: filled from the last vertex down
    std::vector<int64_t> head(size_t(n), -1), next(size_t(n), -1), stack, size(size_t(n), 1);
    for (int64_t v = n - 1; v >= 0; --v) {
        const int64_t p = parent[v];
        if (p >= 0) {
            next[v] = head[p];
            head[p] = v;
        }
    }
    int64_t rank = 0;
    for (int64_t root = 0; root < n; ++root) {
        if (parent[root] != -1) continue;
        stack.push_back(root);
        while (!stack.empty()) {
            const int64_t v = stack.back();
            const int64_t child = head[v];
            if (child == -1) {
                post[v] = I(rank++);
                stack.pop_back();
            } else {
                head[v] = next[child];
                stack.push_back(child);
            }
        }
    }
    for (int64_t v = 0; v < n; ++v) {
        if (parent[v] >= 0) size[parent[v]] += size[v];
        first[v] = I(int64_t(post[v]) - size[v] + 1);
    }
    GKOC_HIP(hipMemcpyAsync(parent_dev, parent.data(), sizeof(I) * size_t(n), hipMemcpyHostToDevice, st));
    GKOC_HIP(hipMemcpyAsync(post_dev, post.data(), sizeof(I) * size_t(n), hipMemcpyHostToDevice, st));
    GKOC_HIP(hipMemcpyAsync(first_dev, first.data(), sizeof(I) * size_t(n), hipMemcpyHostToDevice, st));
    GKOC_HIP(hipStreamSynchronize(st));      // the host vectors end here
    return GKOC_OK;
}

}  // namespace
}  // namespace gkoc

using namespace gkoc;

extern "C" int gkoc_symbolic_row_limits(int* limits_host, int* count_host)
{
    return export_row_limits(symb_row_limits, limits_host, count_host);
}

#define GKOC_DEF_SYMBOLIC(I, A, IN)                                                                            \
    extern "C" int gkoc_symbolic_forest_##IN(gkoc_stream_t s, int64_t n, int64_t nnz, const I* row_ptrs,       \
                                             const I* col_idxs, A* parent, A* post, A* first)                  \
    {                                                                                                          \
        return symbolic_forest<I>(s, n, nnz, row_ptrs, col_idxs, parent, post, first);                         \
    }                                                                                                          \
    extern "C" int gkoc_symbolic_post_keys_##IN(gkoc_stream_t s, int64_t n, int64_t nnz, const I* row_ptrs,    \
                                                const I* col_idxs, const I* post, A* keys, A* inv_post)        \
    {                                                                                                          \
        return symbolic_post_keys<I>(s, n, nnz, row_ptrs, col_idxs, post, keys, inv_post);                     \
    }                                                                                                          \
    extern "C" int gkoc_symbolic_cholesky_count_##IN(gkoc_stream_t s, int64_t n, int64_t nnz,                  \
                                                     const I* row_ptrs, const I* keys, const I* parent,        \
                                                     const I* post, const I* first, const I* inv_post,         \
                                                     gkoc_symbolic_i64* offsets, long long* total_host)        \
    {                                                                                                          \
        return symbolic_count<I>(s, n, nnz, row_ptrs, keys, parent, post, first, inv_post, offsets,            \
                                 total_host);                                                                  \
    }
GKOC_DEF_SYMBOLIC(int32_t, gkoc_symbolic_i32, i32)
GKOC_DEF_SYMBOLIC(int64_t, gkoc_symbolic_i64, i64)

#define GKOC_DEF_SYMBOLIC_EXPAND(T, TN, I, IN)                                                                 \
    extern "C" int gkoc_symbolic_cholesky_expand_##TN##_##IN(                                                  \
        gkoc_stream_t s, int64_t n, int64_t nnz, const I* row_ptrs, const I* keys, const I* parent,            \
        const I* post, const I* first, const I* inv_post, const int64_t* offsets, int64_t total,               \
        void* entries)                                                                                         \
    {                                                                                                          \
        return symbolic_expand<T, I>(s, n, nnz, row_ptrs, keys, parent, post, first, inv_post, offsets, total, \
                                     entries);                                                                 \
    }
GKOC_DEF_SYMBOLIC_EXPAND(double, f64, int32_t, i32)
GKOC_DEF_SYMBOLIC_EXPAND(double, f64, int64_t, i64)
GKOC_DEF_SYMBOLIC_EXPAND(float, f32, int32_t, i32)
GKOC_DEF_SYMBOLIC_EXPAND(float, f32, int64_t, i64)
