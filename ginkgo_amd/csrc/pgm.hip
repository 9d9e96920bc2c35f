// Parallel graph match aggregation (multigrid::Pgm) and its grid transfers:
//   pgm_select / pgm_match / pgm_leftover / pgm_renumber   the aggregation rounds (integers only)
//   pgm_map_entries                                        the triplets of P^T A P from those of A
//   pgm_check_transfers / pgm_restrict / pgm_prolong_add   b_c = P^T r and x += P e from agg and the member lists
//
// Contract: include/gko_cdna4.h, "Pgm aggregation".  W = 0.5 |A| + 0.5 |A^T| (rows sorted, no duplicates) and
// d = diag(W) are the caller's.  A candidate j != i of row i has the key (s_ij, h_ij, j), s_ij = w_ij /
// max(d_i, d_j) (one division in T, skipped unless s >= 0), h_ij a symmetric 32-bit hash of the pair; keys are
// compared lexicographically and the largest wins.
//
// select is the kernel with a shape: a group of W lanes (16, 32 or 64, from the longest row of W of the call)
// takes a row, lane = stored entry, a row longer than W is streamed (lane l reads the entries l, l + W, ...);
// every lane keeps its best unaggregated and its best aggregated candidate, the group reduces both by a
// butterfly of shuffles.  No length cap, no serial path.  leftover is the same kernel without the unaggregated
// candidates.
//
// Invariants:
//   1. no atomics: every output element has exactly one writer (row i's entry by lane 0 of its group; status
//      flags are plain stores of 1; counts and maxima leave the device as one partial per block);
//   2. a round never reads what it writes: select reads agg and writes the proposals, match reads the proposals
//      and writes agg[i] only, leftover reads a snapshot and writes another array;
//   3. nothing is indexed by a value that was not checked: select / leftover index with columns of W (checked
//      by the entry), match with proposals (checked), renumber and map_entries with agg (checked); restrict and
//      prolong_add check nothing on the device - gkoc_pgm_check_transfers does, once, at generate;
//   4. no entry writes an index array of a matrix: agg and the proposals are state of the aggregation
//      (gkoc_pgm_i32 / _i64 in the header) and the coarse triplets leave as matrix_data entries, which
//      gkoc_aos_to_soa and gkoc_sort_row_major - both known to csr::spmv's column-offset plan - turn into arrays.
#include <hip/hip_runtime.h>

#include <climits>

#include "common.hpp"
#include "scan.hpp"
#include "sparse_rows.hpp"

namespace gkoc {
namespace {

constexpr int pgm_block = 256;
constexpr int pgm_row_limits[] = {16, 32, 64};

// this file's grids: at most max_stream_blocks workgroups (the partials per block that match and check_csr
// read back have that many places)
inline unsigned pgm_grid(int64_t items, int per_block = pgm_block)
{
    return capped_grid(items, per_block, max_stream_blocks);
}

// ------------------------------------------------------------------ the key
template <typename T>
struct candidate {
    T s;
    uint32_t h;
    long long j;    // < 0: none
};

__device__ __forceinline__ uint32_t pair_hash(int64_t i, int64_t j)
{
    const uint32_t lo = uint32_t(i < j ? i : j), hi = uint32_t(i < j ? j : i);
    uint32_t h = (lo * 0x9E3779B1u) ^ (hi * 0x85EBCA77u);
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 12;
    return h;
}

// a beats b
template <typename T>
__device__ __forceinline__ bool better(const candidate<T>& a, const candidate<T>& b)
{
    if (a.j < 0) return false;
    if (b.j < 0) return true;
    if (a.s != b.s) return a.s > b.s;
    if (a.h != b.h) return a.h > b.h;
    return a.j > b.j;
}

// the best candidate of the group of W lanes this lane belongs to, in every lane of the group
template <int W, typename T>
__device__ __forceinline__ candidate<T> group_best(candidate<T> c)
{
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) {
        candidate<T> o;
        o.s = __shfl_xor(c.s, off, W);
        o.h = uint32_t(__shfl_xor(int(c.h), off, W));
        o.j = __shfl_xor(c.j, off, W);
        if (better(o, c)) c = o;
    }
    return c;
}

// One row by one group of W lanes.  LEFTOVER == false: out[row] = -1 (row is aggregated), k >= 0 (it proposes
// to k; k == row: to itself), -2 - a (it joins the aggregate a of its best aggregated neighbour).
// LEFTOVER == true: out[row] = the aggregate of the row after the leftover step.
template <bool LEFTOVER, int W, typename T, typename I>
__device__ __forceinline__ void select_row(int64_t row, int lane, const I* __restrict__ rp,
                                           const I* __restrict__ ci, const T* __restrict__ wv,
                                           const T* __restrict__ d, const I* __restrict__ agg,
                                           I* __restrict__ out)
{
    const I own = agg[row];
    if (own != I(-1)) {
        if (lane == 0) out[row] = LEFTOVER ? own : I(-1);
        return;
    }
    const int64_t begin = rp[row], end = rp[row + 1];
    const T di = d[row];
    candidate<T> u{T(0), 0u, -1LL}, g{T(0), 0u, -1LL};
    for (int64_t e = begin + lane; e < end; e += W) {
        const int64_t j = ci[e];
        if (j == row) continue;
        const T dj = d[j];
        const T s = wv[e] / (di > dj ? di : dj);
        if (!(s >= T(0))) continue;
        const candidate<T> c{s, pair_hash(row, j), (long long)(j)};
        if (agg[j] == I(-1)) {
            if (!LEFTOVER && better(c, u)) u = c;
        } else if (better(c, g)) {
            g = c;
        }
    }
    if (!LEFTOVER) u = group_best<W, T>(u);
    g = group_best<W, T>(g);
    if (lane != 0) return;
    if (LEFTOVER) {
        out[row] = g.j >= 0 ? agg[g.j] : I(row);
    } else if (u.j >= 0) {
        out[row] = I(u.j);
    } else if (g.j >= 0) {
        out[row] = I(-2) - agg[g.j];
    } else {
        out[row] = I(row);
    }
}

template <bool LEFTOVER, int W, typename T, typename I>
__global__ __launch_bounds__(pgm_block) void select_kernel(int64_t n, const I* __restrict__ rp,
                                                           const I* __restrict__ ci, const T* __restrict__ wv,
                                                           const T* __restrict__ d, const I* __restrict__ agg,
                                                           I* __restrict__ out)
{
    constexpr int groups = pgm_block / W;
    const int lane = threadIdx.x % W;
    const int64_t stride = int64_t(gridDim.x) * groups;
    for (int64_t row = int64_t(blockIdx.x) * groups + threadIdx.x / W; row < n; row += stride) {
        select_row<LEFTOVER, W, T, I>(row, lane, rp, ci, wv, d, agg, out);
    }
}

// ------------------------------------------------------------------ checks (one thread per element)
// status[0]: row pointers that do not ascend from 0, status[1]: a column outside the matrix;
// longest[block]: the longest row the block saw.  A row is read only if its pointers are sound.
template <typename I>
__global__ __launch_bounds__(pgm_block) void check_csr_kernel(int64_t n, const I* __restrict__ rp,
                                                              const I* __restrict__ ci, int* __restrict__ status,
                                                              int* __restrict__ longest_of_block)
{
    __shared__ int lds[pgm_block / wave_size];
    const int64_t stride = int64_t(gridDim.x) * pgm_block;
    const int64_t nnz = rp[n];
    int longest = 0;
    for (int64_t row = int64_t(blockIdx.x) * pgm_block + threadIdx.x; row < n; row += stride) {
        const int64_t begin = rp[row], end = rp[row + 1];
        if (begin < 0 || end < begin || end > nnz || (row == 0 && begin != 0)) {
            status[0] = 1;
            continue;
        }
        for (int64_t k = begin; k < end; ++k) {
            const int64_t col = ci[k];
            if (col < 0 || col >= n) status[1] = 1;
        }
        const int64_t len = end - begin;
        longest = len > longest ? int(len > INT_MAX ? INT_MAX : len) : longest;
    }
    longest = wave_max(longest);
    if ((threadIdx.x & (wave_size - 1)) == 0) lds[threadIdx.x / wave_size] = longest;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < pgm_block / wave_size; ++w) longest = lds[w] > longest ? lds[w] : longest;
        longest_of_block[blockIdx.x] = longest;
    }
}

// *flag = 1 if a value lies outside [lo, hi)
template <typename I>
__global__ __launch_bounds__(pgm_block) void check_range_kernel(int64_t n, const I* __restrict__ v, int64_t lo,
                                                                int64_t hi, int* __restrict__ flag)
{
    const int64_t stride = int64_t(gridDim.x) * pgm_block;
    for (int64_t i = int64_t(blockIdx.x) * pgm_block + threadIdx.x; i < n; i += stride) {
        const int64_t x = v[i];
        if (x < lo || x >= hi) *flag = 1;
    }
}

// proposals: -1, k in [0, n), or -2 - a with a in [0, n)
template <typename I>
__global__ __launch_bounds__(pgm_block) void check_proposals_kernel(int64_t n, const I* __restrict__ prop,
                                                                    int* __restrict__ flag)
{
    const int64_t stride = int64_t(gridDim.x) * pgm_block;
    for (int64_t i = int64_t(blockIdx.x) * pgm_block + threadIdx.x; i < n; i += stride) {
        const int64_t p = prop[i];
        if (p >= n || p < -1 - n) *flag = 1;
    }
}

// agg holds roots: agg[i] in [0, n) and agg[agg[i]] == agg[i]
template <typename I>
__global__ __launch_bounds__(pgm_block) void check_roots_kernel(int64_t n, const I* __restrict__ agg,
                                                                int* __restrict__ flag)
{
    const int64_t stride = int64_t(gridDim.x) * pgm_block;
    for (int64_t i = int64_t(blockIdx.x) * pgm_block + threadIdx.x; i < n; i += stride) {
        const int64_t a = agg[i];
        if (a < 0 || a >= n || int64_t(agg[a]) != a) *flag = 1;
    }
}

// ptrs[0] == 0, ptrs ascending, ptrs[n] == total
template <typename I>
__global__ __launch_bounds__(pgm_block) void check_ptrs_kernel(int64_t n, const I* __restrict__ ptrs,
                                                               int64_t total, int* __restrict__ flag)
{
    const int64_t stride = int64_t(gridDim.x) * pgm_block;
    for (int64_t i = int64_t(blockIdx.x) * pgm_block + threadIdx.x; i <= n; i += stride) {
        const int64_t p = ptrs[i];
        if ((i == 0 && p != 0) || (i == n && p != total) || (i < n && int64_t(ptrs[i + 1]) < p) || p < 0 ||
            p > total) {
            *flag = 1;
        }
    }
}

// ------------------------------------------------------------------ match, count, renumber, map
template <typename I>
__global__ __launch_bounds__(pgm_block) void match_kernel(int64_t n, const I* __restrict__ prop, I* agg)
{
    const int64_t stride = int64_t(gridDim.x) * pgm_block;
    for (int64_t i = int64_t(blockIdx.x) * pgm_block + threadIdx.x; i < n; i += stride) {
        const int64_t p = prop[i];
        if (p <= -2) {
            agg[i] = I(-2 - p);
        } else if (p == i) {
            agg[i] = I(i);
        } else if (p >= 0 && int64_t(prop[p]) == i) {
            agg[i] = I(i < p ? i : p);
        }
    }
}

template <typename I>
__global__ __launch_bounds__(pgm_block) void count_unassigned_kernel(int64_t n, const I* __restrict__ agg,
                                                                     long long* __restrict__ count_of_block)
{
    __shared__ long long lds[pgm_block / wave_size];
    const int64_t stride = int64_t(gridDim.x) * pgm_block;
    long long count = 0;
    for (int64_t i = int64_t(blockIdx.x) * pgm_block + threadIdx.x; i < n; i += stride) {
        count += agg[i] == I(-1) ? 1 : 0;
    }
    count = block_sum<pgm_block>(count, lds);
    if (threadIdx.x == 0) count_of_block[blockIdx.x] = count;
}

// rank[i] = 1 if i is a root, rank[n] = 0
template <typename I>
__global__ __launch_bounds__(pgm_block) void mark_roots_kernel(int64_t n, const I* __restrict__ agg,
                                                               I* __restrict__ rank)
{
    const int64_t stride = int64_t(gridDim.x) * pgm_block;
    for (int64_t i = int64_t(blockIdx.x) * pgm_block + threadIdx.x; i <= n; i += stride) {
        rank[i] = i < n && int64_t(agg[i]) == i ? I(1) : I(0);
    }
}

// out[i] = map[in[i]]; in == out is allowed (one reader and one writer per element)
template <typename I>
__global__ __launch_bounds__(pgm_block) void gather_kernel(int64_t n, const I* __restrict__ map, const I* in,
                                                           I* out)
{
    const int64_t stride = int64_t(gridDim.x) * pgm_block;
    for (int64_t i = int64_t(blockIdx.x) * pgm_block + threadIdx.x; i < n; i += stride) out[i] = map[in[i]];
}

// gko::matrix_data_entry<T, I> with natural alignment, the layout of gkoc_soa_to_aos / gkoc_aos_to_soa
template <typename T, typename I>
struct coarse_entry {
    I row;
    I column;
    T value;
};

// entries[k] = (agg[row of k], agg[column of k], value of k), in storage order
template <typename T, typename I>
__global__ __launch_bounds__(pgm_block) void map_entries_kernel(int64_t nnz, const I* __restrict__ agg,
                                                                const I* __restrict__ rows,
                                                                const I* __restrict__ cols,
                                                                const T* __restrict__ vals,
                                                                coarse_entry<T, I>* __restrict__ entries)
{
    const int64_t stride = int64_t(gridDim.x) * pgm_block;
    for (int64_t k = int64_t(blockIdx.x) * pgm_block + threadIdx.x; k < nnz; k += stride) {
        coarse_entry<T, I> e;
        e.row = agg[rows[k]];
        e.column = agg[cols[k]];
        e.value = vals[k];
        entries[k] = e;
    }
}

// ------------------------------------------------------------------ transfers
// bc[J, c] = sum over the members i of J, ascending, of r[i, c]: sequential in T, one thread per (J, c)
template <typename T, typename I>
__global__ __launch_bounds__(pgm_block) void restrict_kernel(int64_t n_c, int64_t cols,
                                                             const I* __restrict__ member_ptrs,
                                                             const I* __restrict__ members,
                                                             const T* __restrict__ r, int64_t ldr,
                                                             T* __restrict__ bc, int64_t ldbc)
{
    const int64_t total = n_c * cols;
    const int64_t stride = int64_t(gridDim.x) * pgm_block;
    for (int64_t idx = int64_t(blockIdx.x) * pgm_block + threadIdx.x; idx < total; idx += stride) {
        const int64_t row = cols == 1 ? idx : idx / cols;
        const int64_t col = cols == 1 ? 0 : idx - row * cols;
        const int64_t begin = member_ptrs[row], end = member_ptrs[row + 1];
        T sum = T(0);
        for (int64_t k = begin; k < end; ++k) sum += r[int64_t(members[k]) * ldr + col];
        bc[row * ldbc + col] = sum;
    }
}

// x[i, c] = x[i, c] + e[agg[i], c]
template <typename T, typename I>
__global__ __launch_bounds__(pgm_block) void prolong_add_kernel(int64_t n, int64_t cols,
                                                                const I* __restrict__ agg,
                                                                const T* __restrict__ e, int64_t lde, T* x,
                                                                int64_t ldx)
{
    const int64_t total = n * cols;
    const int64_t stride = int64_t(gridDim.x) * pgm_block;
    for (int64_t idx = int64_t(blockIdx.x) * pgm_block + threadIdx.x; idx < total; idx += stride) {
        const int64_t row = cols == 1 ? idx : idx / cols;
        const int64_t col = cols == 1 ? 0 : idx - row * cols;
        x[row * ldx + col] = x[row * ldx + col] + e[int64_t(agg[row]) * lde + col];
    }
}

// ------------------------------------------------------------------ host side
// checks W's index arrays; *longest = its longest row
template <typename I>
int check_csr(hipStream_t st, int64_t n, const I* rp, const I* ci, int* longest)
{
    const unsigned grid = pgm_grid(n);
    void* raw = nullptr;
    GKOC_TRY(scratch_malloc(st, &raw, sizeof(int) * (2 + size_t(grid))));
    scratch_guard guard{st, raw};
    int* status = static_cast<int*>(raw);
    GKOC_HIP(hipMemsetAsync(status, 0, sizeof(int) * (2 + size_t(grid)), st));
    check_csr_kernel<I><<<dim3(grid), dim3(pgm_block), 0, st>>>(n, rp, ci, status, status + 2);
    GKOC_LAUNCH_OK();
    static thread_local int host[2 + max_stream_blocks];
    GKOC_HIP(hipMemcpyAsync(host, status, sizeof(int) * (2 + size_t(grid)), hipMemcpyDeviceToHost, st));
    GKOC_HIP(hipStreamSynchronize(st));
    GKOC_REQUIRE(host[0] == 0, GKOC_E_INVALID, "row pointers do not ascend from 0");
    GKOC_REQUIRE(host[1] == 0, GKOC_E_INVALID, "a column outside the matrix");
    *longest = 0;
    for (unsigned b = 0; b < grid; ++b) *longest = host[2 + b] > *longest ? host[2 + b] : *longest;
    return GKOC_OK;
}

template <bool LEFTOVER, int W, typename T, typename I>
int select_launch(hipStream_t st, int64_t n, const I* rp, const I* ci, const T* wv, const T* d, const I* agg,
                  I* out)
{
    select_kernel<LEFTOVER, W, T, I>
        <<<dim3(pgm_grid(n, pgm_block / W) * 4), dim3(pgm_block), 0, st>>>(n, rp, ci, wv, d, agg, out);
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

template <bool LEFTOVER, typename T, typename I>
int select(gkoc_stream_t s, int64_t n, const I* rp, const I* ci, const T* wv, const T* d, const I* agg, I* out)
{
    GKOC_REQUIRE(n >= 0, GKOC_E_INVALID, "negative number of rows");
    if (n == 0) return GKOC_OK;
    GKOC_REQUIRE(rp && ci && wv && d && agg && out, GKOC_E_INVALID, "null pointer");
    GKOC_REQUIRE(agg != out, GKOC_E_INVALID, "the aggregation that is read and the array that is written are one");
    hipStream_t st = as_stream(s);
    int longest = 0;
    GKOC_TRY(check_csr<I>(st, n, rp, ci, &longest));
    return with_lanes(longest, pgm_row_limits, [&](auto w) {
        return select_launch<LEFTOVER, decltype(w)::value, T, I>(st, n, rp, ci, wv, d, agg, out);
    });
}

template <typename I>
int match(gkoc_stream_t s, int64_t n, const I* prop, I* agg, long long* unassigned_host)
{
    GKOC_REQUIRE(n >= 0, GKOC_E_INVALID, "negative number of rows");
    GKOC_REQUIRE(unassigned_host, GKOC_E_INVALID, "null pointer");
    *unassigned_host = 0;
    if (n == 0) return GKOC_OK;
    GKOC_REQUIRE(prop && agg, GKOC_E_INVALID, "null pointer");
    GKOC_REQUIRE(prop != agg, GKOC_E_INVALID, "the proposals and the aggregation are one array");
    hipStream_t st = as_stream(s);
    const unsigned grid = pgm_grid(n);
    // scratch: the flag, then one count per block
    status_words<1> bad(st);
    GKOC_TRY(bad.init(sizeof(long long) * size_t(grid)));
    long long* counts = bad.template behind<long long>();
    check_proposals_kernel<I><<<dim3(grid), dim3(pgm_block), 0, st>>>(n, prop, bad.dev);
    GKOC_LAUNCH_OK();
    GKOC_TRY(bad.read());
    GKOC_REQUIRE(bad[0] == 0, GKOC_E_INVALID, "a proposal outside the matrix");
    match_kernel<I><<<dim3(grid), dim3(pgm_block), 0, st>>>(n, prop, agg);
    GKOC_LAUNCH_OK();
    count_unassigned_kernel<I><<<dim3(grid), dim3(pgm_block), 0, st>>>(n, agg, counts);
    GKOC_LAUNCH_OK();
    static thread_local long long host[max_stream_blocks];
    GKOC_HIP(hipMemcpyAsync(host, counts, sizeof(long long) * grid, hipMemcpyDeviceToHost, st));
    GKOC_HIP(hipStreamSynchronize(st));
    for (unsigned b = 0; b < grid; ++b) *unassigned_host += host[b];
    return GKOC_OK;
}

template <typename I>
int renumber(gkoc_stream_t s, int64_t n, I* agg, long long* num_aggregates_host)
{
    GKOC_REQUIRE(n >= 0, GKOC_E_INVALID, "negative number of rows");
    GKOC_REQUIRE(num_aggregates_host, GKOC_E_INVALID, "null pointer");
    *num_aggregates_host = 0;
    if (n == 0) return GKOC_OK;
    GKOC_REQUIRE(agg, GKOC_E_INVALID, "null pointer");
    hipStream_t st = as_stream(s);
    const unsigned grid = pgm_grid(n + 1);
    // scratch: the flag, then the ranks (n + 1 entries)
    status_words<1> bad(st);
    GKOC_TRY(bad.init(sizeof(I) * size_t(n + 1)));
    I* rank = bad.template behind<I>();
    check_roots_kernel<I><<<dim3(grid), dim3(pgm_block), 0, st>>>(n, agg, bad.dev);
    GKOC_LAUNCH_OK();
    GKOC_TRY(bad.read());
    GKOC_REQUIRE(bad[0] == 0, GKOC_E_INVALID, "an entry of agg is not the root of an aggregate");
    mark_roots_kernel<I><<<dim3(grid), dim3(pgm_block), 0, st>>>(n, agg, rank);
    GKOC_LAUNCH_OK();
    GKOC_TRY(device_exclusive_scan<I>(st, rank, n + 1));
    gather_kernel<I><<<dim3(grid), dim3(pgm_block), 0, st>>>(n, rank, agg, agg);
    GKOC_LAUNCH_OK();
    I total = 0;
    GKOC_HIP(hipMemcpyAsync(&total, rank + n, sizeof(I), hipMemcpyDeviceToHost, st));
    GKOC_HIP(hipStreamSynchronize(st));
    *num_aggregates_host = (long long)(total);
    return GKOC_OK;
}

template <typename T, typename I>
int map_entries(gkoc_stream_t s, int64_t nnz, int64_t n, int64_t n_c, const I* agg, const I* rows_in,
                const I* cols_in, const T* vals, void* entries)
{
    GKOC_REQUIRE(nnz >= 0 && n >= 0 && n_c >= 0 && n_c <= n, GKOC_E_INVALID, "bad sizes");
    if (nnz == 0) return GKOC_OK;
    GKOC_REQUIRE(agg && rows_in && cols_in && vals && entries, GKOC_E_INVALID, "null pointer");
    hipStream_t st = as_stream(s);
    const unsigned grid = pgm_grid(nnz), grid_n = pgm_grid(n);
    status_words<2> bad(st);
    GKOC_TRY(bad.init());
    check_range_kernel<I><<<dim3(grid_n), dim3(pgm_block), 0, st>>>(n, agg, 0, n_c, bad.dev);
    GKOC_LAUNCH_OK();
    check_range_kernel<I><<<dim3(grid), dim3(pgm_block), 0, st>>>(nnz, rows_in, 0, n, bad.dev + 1);
    GKOC_LAUNCH_OK();
    check_range_kernel<I><<<dim3(grid), dim3(pgm_block), 0, st>>>(nnz, cols_in, 0, n, bad.dev + 1);
    GKOC_LAUNCH_OK();
    GKOC_TRY(bad.read());
    GKOC_REQUIRE(bad[0] == 0, GKOC_E_INVALID, "an entry of agg outside [0, n_coarse)");
    GKOC_REQUIRE(bad[1] == 0, GKOC_E_INVALID, "a row or column index outside the matrix");
    map_entries_kernel<T, I><<<dim3(grid), dim3(pgm_block), 0, st>>>(nnz, agg, rows_in, cols_in, vals,
                                                                      static_cast<coarse_entry<T, I>*>(entries));
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

template <typename I>
int check_transfers(gkoc_stream_t s, int64_t n, int64_t n_c, const I* agg, const I* member_ptrs,
                    const I* members)
{
    GKOC_REQUIRE(n >= 0 && n_c >= 0 && n_c <= n, GKOC_E_INVALID, "bad sizes");
    if (n == 0) return GKOC_OK;
    GKOC_REQUIRE(agg && member_ptrs && members, GKOC_E_INVALID, "null pointer");
    hipStream_t st = as_stream(s);
    const unsigned grid = pgm_grid(n + 1);
    status_words<3> bad(st);
    GKOC_TRY(bad.init());
    check_range_kernel<I><<<dim3(grid), dim3(pgm_block), 0, st>>>(n, agg, 0, n_c, bad.dev);
    GKOC_LAUNCH_OK();
    check_ptrs_kernel<I><<<dim3(grid), dim3(pgm_block), 0, st>>>(n_c, member_ptrs, n, bad.dev + 1);
    GKOC_LAUNCH_OK();
    check_range_kernel<I><<<dim3(grid), dim3(pgm_block), 0, st>>>(n, members, 0, n, bad.dev + 2);
    GKOC_LAUNCH_OK();
    GKOC_TRY(bad.read());
    GKOC_REQUIRE(bad[0] == 0, GKOC_E_INVALID, "an entry of agg outside [0, n_coarse)");
    GKOC_REQUIRE(bad[1] == 0, GKOC_E_INVALID, "the member pointers do not ascend from 0 to the number of rows");
    GKOC_REQUIRE(bad[2] == 0, GKOC_E_INVALID, "a member outside the matrix");
    return GKOC_OK;
}

template <typename T, typename I>
int restrict_apply(gkoc_stream_t s, int64_t n_c, int64_t cols, const I* member_ptrs, const I* members,
                   const T* r, int64_t ldr, T* bc, int64_t ldbc)
{
    GKOC_REQUIRE(n_c >= 0 && cols >= 0, GKOC_E_INVALID, "negative size");
    if (n_c == 0 || cols == 0) return GKOC_OK;
    GKOC_REQUIRE(member_ptrs && members && r && bc, GKOC_E_INVALID, "null pointer");
    GKOC_REQUIRE(ldr >= cols && ldbc >= cols, GKOC_E_INVALID, "a stride smaller than the number of columns");
    restrict_kernel<T, I><<<dim3(pgm_grid(n_c * cols) * 4), dim3(pgm_block), 0,
                            as_stream(s)>>>(n_c, cols, member_ptrs, members, r, ldr, bc, ldbc);
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

template <typename T, typename I>
int prolong_add(gkoc_stream_t s, int64_t n, int64_t cols, const I* agg, const T* e, int64_t lde, T* x,
                int64_t ldx)
{
    GKOC_REQUIRE(n >= 0 && cols >= 0, GKOC_E_INVALID, "negative size");
    if (n == 0 || cols == 0) return GKOC_OK;
    GKOC_REQUIRE(agg && e && x, GKOC_E_INVALID, "null pointer");
    GKOC_REQUIRE(lde >= cols && ldx >= cols, GKOC_E_INVALID, "a stride smaller than the number of columns");
    prolong_add_kernel<T, I><<<dim3(pgm_grid(n * cols) * 4), dim3(pgm_block), 0,
                               as_stream(s)>>>(n, cols, agg, e, lde, x, ldx);
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

}  // namespace
}  // namespace gkoc

using namespace gkoc;

extern "C" int gkoc_pgm_row_limits(int* limits_host, int* count_host)
{
    return export_row_limits(pgm_row_limits, limits_host, count_host);
}

// A: the header's gkoc_pgm_i32 / gkoc_pgm_i64 (an aggregation array; the same type as I)
#define GKOC_DEF_PGM_IDX(I, A, IN)                                                                             \
    extern "C" int gkoc_pgm_match_##IN(gkoc_stream_t s, int64_t n_rows, const I* proposals, A* agg,            \
                                       long long* unassigned_host)                                             \
    {                                                                                                          \
        return match<I>(s, n_rows, proposals, agg, unassigned_host);                                           \
    }                                                                                                          \
    extern "C" int gkoc_pgm_renumber_##IN(gkoc_stream_t s, int64_t n_rows, A* agg,                             \
                                          long long* num_aggregates_host)                                      \
    {                                                                                                          \
        return renumber<I>(s, n_rows, agg, num_aggregates_host);                                               \
    }                                                                                                          \
    extern "C" int gkoc_pgm_check_transfers_##IN(gkoc_stream_t s, int64_t n_rows, int64_t n_coarse,            \
                                                 const I* agg, const I* member_ptrs, const I* members)         \
    {                                                                                                          \
        return check_transfers<I>(s, n_rows, n_coarse, agg, member_ptrs, members);                             \
    }
GKOC_DEF_PGM_IDX(int32_t, gkoc_pgm_i32, i32)
GKOC_DEF_PGM_IDX(int64_t, gkoc_pgm_i64, i64)

#define GKOC_DEF_PGM(T, TN, I, A, IN)                                                                          \
    extern "C" int gkoc_pgm_select_##TN##_##IN(gkoc_stream_t s, int64_t n_rows, const I* w_rp, const I* w_ci,  \
                                               const T* w_v, const T* d, const I* agg, A* proposals)           \
    {                                                                                                          \
        return select<false, T, I>(s, n_rows, w_rp, w_ci, w_v, d, agg, proposals);                             \
    }                                                                                                          \
    extern "C" int gkoc_pgm_leftover_##TN##_##IN(gkoc_stream_t s, int64_t n_rows, const I* w_rp,               \
                                                 const I* w_ci, const T* w_v, const T* d,                      \
                                                 const I* agg_before, A* agg)                                  \
    {                                                                                                          \
        return select<true, T, I>(s, n_rows, w_rp, w_ci, w_v, d, agg_before, agg);                             \
    }                                                                                                          \
    extern "C" int gkoc_pgm_map_entries_##TN##_##IN(gkoc_stream_t s, int64_t nnz, int64_t n_rows,              \
                                                    int64_t n_coarse, const I* agg, const I* row_idxs,         \
                                                    const I* col_idxs, const T* vals, void* entries)           \
    {                                                                                                          \
        return map_entries<T, I>(s, nnz, n_rows, n_coarse, agg, row_idxs, col_idxs, vals, entries);            \
    }                                                                                                          \
    extern "C" int gkoc_pgm_restrict_##TN##_##IN(gkoc_stream_t s, int64_t n_coarse, int64_t cols,              \
                                                 const I* member_ptrs, const I* members, const T* r,           \
                                                 int64_t ldr, T* b_coarse, int64_t ldb)                        \
    {                                                                                                          \
        return restrict_apply<T, I>(s, n_coarse, cols, member_ptrs, members, r, ldr, b_coarse, ldb);           \
    }                                                                                                          \
    extern "C" int gkoc_pgm_prolong_add_##TN##_##IN(gkoc_stream_t s, int64_t n_rows, int64_t cols,             \
                                                    const I* agg, const T* e, int64_t lde, T* x, int64_t ldx)  \
    {                                                                                                          \
        return prolong_add<T, I>(s, n_rows, cols, agg, e, lde, x, ldx);                                        \
    }
GKOC_DEF_PGM(double, f64, int32_t, gkoc_pgm_i32, i32)
GKOC_DEF_PGM(double, f64, int64_t, gkoc_pgm_i64, i64)
GKOC_DEF_PGM(float, f32, int32_t, gkoc_pgm_i32, i32)
GKOC_DEF_PGM(float, f32, int64_t, gkoc_pgm_i64, i64)
