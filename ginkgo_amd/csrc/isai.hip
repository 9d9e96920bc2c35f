// Incomplete sparse approximate inverse of a triangular matrix (preconditioner::LowerIsai / UpperIsai):
//   isai_generate_tri_inverse      the VALUES of W on a given pattern, (W A)(i, S_i) = e_i(S_i) for every row i
//                                  (reference/preconditioner/isai_kernels.cpp: generate_tri_inverse)
//
// Contract (it fixes the rounding; -ffp-contract=off keeps multiply and subtract apart).  A is triangular on
// the stated side, rows sorted, the diagonal LAST in every row (lower) or FIRST (upper).  Row i of the pattern,
// S_i, is sorted, lies on the same side and contains i.
//   lower: c_0 < ... < c_{m-1} = i the columns of S_i.  For t = m-1 down to 0: s = (c_t == i) ? 1 : 0; for
//          u = m-1 down to t+1, whenever (c_u, c_t) is stored in A: s = s - w[c_u] * a[c_u, c_t];
//          w[c_t] = s / a[c_t, c_t].
//   upper: the mirror image - c_0 = i < ... < c_{m-1}, t ascending, u ascending from 0 to t-1.
//   If any w of a row is not finite, the row becomes all zeros with 1 on the diagonal (Ginkgo's rule).
// This is the row's small triangular system (A(S_i, S_i))^T w = e_i solved by substitution, column-oriented:
// the finished w[c_u] is subtracted from every entry still open, in the order u is finished.
//
// One launch for all rows: no row depends on another.  A group of W lanes (16, 32 or 64, from the longest
// pattern row of the call) takes a row, lane = stored entry of S_i, the value in a register.  In step u the
// lane that owns c_u finishes its value with the division and the group gets it by a shuffle; every lane
// still open looks its own column up in row c_u of A by a binary search and subtracts.  A pattern row longer
// than 64 entries (W is 64 then) is streamed: lane l owns the entries l, l + 64, ... and keeps them in w_v,
// the finished value still travels by shuffle.  There is no length cap and no serial path.
//
// Invariants:
//   1. every entry of w_v is written by exactly one lane (entry e of a row by lane e % W), no atomics on values;
//   2. an entry's updates happen in the order of the contract (u runs the same way in every lane);
//   3. no kernel writes an index array: every index pointer of the entry is const, so the column-offset plan of
//      csr::spmv has nothing to be told (the pattern of W is made by entries that exist already);
//   4. A is read-only (const __restrict__); w_v is read and written by the streamed path, so it is ONE plain
//      pointer there, neither const nor __restrict__.
#include <hip/hip_runtime.h>

#include <climits>

#include "common.hpp"

namespace gkoc {
namespace {

constexpr int isai_block = 256;
constexpr int isai_row_limits[] = {16, 32, 64};

// position of column c in ci[lo, hi) (ascending), -1 if it is not stored
template <typename I>
__device__ __forceinline__ int64_t find_column(const I* __restrict__ ci, int64_t lo, int64_t hi, int64_t c)
{
    const int64_t end = hi;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (int64_t(ci[mid]) < c) {
            lo = mid + 1;
        } else {
            hi = mid;
        }
    }
    return lo < end && int64_t(ci[lo]) == c ? lo : int64_t(-1);
}

__device__ __forceinline__ bool is_finite(double v) { return ::isfinite(v); }
__device__ __forceinline__ bool is_finite(float v) { return ::isfinite(v); }

// `flag` of any lane of the group of W lanes this lane belongs to
template <int W>
__device__ __forceinline__ int group_any(int flag)
{
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) {
        flag |= __shfl_xor(flag, off, W);
    }
    return flag;
}

// The off-diagonal part of row k of A and the position of its diagonal.
template <bool LOWER, typename I>
__device__ __forceinline__ void row_of_a(int64_t k, const I* __restrict__ a_rp, int64_t& lo, int64_t& hi,
                                         int64_t& diag)
{
    const int64_t begin = a_rp[k], end = a_rp[k + 1];
    diag = LOWER ? end - 1 : begin;
    lo = LOWER ? begin : begin + 1;
    hi = LOWER ? end - 1 : end;
}

// v - w_u * a[k, col] if (k, col) is stored in the off-diagonal part [lo, hi) of row k of A, else v
template <typename T, typename I>
__device__ __forceinline__ T updated(T v, T w_u, int64_t col, int64_t lo, int64_t hi, const I* __restrict__ a_ci,
                                     const T* __restrict__ a_v)
{
    const int64_t pos = find_column(a_ci, lo, hi, col);
    return pos >= 0 ? v - w_u * a_v[pos] : v;
}

// one row of W by one group of W lanes; `lane` in [0, W)
template <bool LOWER, int W, typename T, typename I>
__device__ __forceinline__ void inverse_row(int64_t row, int lane, const I* __restrict__ a_rp,
                                            const I* __restrict__ a_ci, const T* __restrict__ a_v,
                                            const I* __restrict__ w_rp, const I* __restrict__ w_ci, T* w_v)
{
    const int64_t begin = w_rp[row];
    const int len = int(int64_t(w_rp[row + 1]) - begin);
    const int diag_entry = LOWER ? len - 1 : 0;
    if (len <= W) {
        const bool valid = lane < len;
        const long long col = valid ? (long long)(w_ci[begin + lane]) : -1LL;
        T v = lane == diag_entry ? T(1) : T(0);
        for (int step = 0; step < len; ++step) {
            const int u = LOWER ? len - 1 - step : step;
            const int64_t k = __shfl(col, u, W);
            int64_t lo, hi, diag;
            row_of_a<LOWER, I>(k, a_rp, lo, hi, diag);
            if (lane == u) v = v / a_v[diag];
            const T w_u = __shfl(v, u, W);
            if (valid && (LOWER ? lane < u : lane > u)) v = updated<T, I>(v, w_u, col, lo, hi, a_ci, a_v);
        }
        if (group_any<W>(valid && !is_finite(v))) v = lane == diag_entry ? T(1) : T(0);
        if (valid) w_v[begin + lane] = v;
    } else if (W == wave_size) {
        // streamed: lane l owns the entries l, l + W, ... and keeps them in memory
        for (int e = lane; e < len; e += W) w_v[begin + e] = e == diag_entry ? T(1) : T(0);
        for (int step = 0; step < len; ++step) {
            const int u = LOWER ? len - 1 - step : step;
            const int64_t k = w_ci[begin + u];
            int64_t lo, hi, diag;
            row_of_a<LOWER, I>(k, a_rp, lo, hi, diag);
            const int owner = u & (W - 1);
            T v = T(0);
            if (lane == owner) {
                v = w_v[begin + u] / a_v[diag];
                w_v[begin + u] = v;
            }
            const T w_u = __shfl(v, owner, W);
            // the entries still open: e < u (lower), e > u (upper)
            const int first = LOWER ? lane : u + 1 + ((lane - (u + 1)) & (W - 1));
            const int last = LOWER ? u : len;
            for (int e = first; e < last; e += W) {
                w_v[begin + e] = updated<T, I>(w_v[begin + e], w_u, int64_t(w_ci[begin + e]), lo, hi, a_ci, a_v);
            }
        }
        int bad = 0;
        for (int e = lane; e < len; e += W) bad |= !is_finite(w_v[begin + e]);
        if (group_any<W>(bad)) {
            for (int e = lane; e < len; e += W) w_v[begin + e] = e == diag_entry ? T(1) : T(0);
        }
    }
}

template <bool LOWER, int W, typename T, typename I>
__global__ __launch_bounds__(isai_block) void tri_inverse_kernel(int64_t n, const I* __restrict__ a_rp,
                                                                 const I* __restrict__ a_ci,
                                                                 const T* __restrict__ a_v,
                                                                 const I* __restrict__ w_rp,
                                                                 const I* __restrict__ w_ci, T* w_v)
{
    constexpr int groups = isai_block / W;
    const int lane = threadIdx.x % W;
    const int64_t stride = int64_t(gridDim.x) * groups;
    for (int64_t row = int64_t(blockIdx.x) * groups + threadIdx.x / W; row < n; row += stride) {
        inverse_row<LOWER, W, T, I>(row, lane, a_rp, a_ci, a_v, w_rp, w_ci, w_v);
    }
}

// One thread per row of one index structure (A or the pattern).  status[0]: row pointers that do not ascend
// from 0, [1]: a column outside the matrix, [2]: an entry on the wrong side, [3]: a row whose last (lower) /
// first (upper) entry is not its diagonal, [4]: the longest row.  A row is read only if its pointers are sound.
template <typename I>
__global__ __launch_bounds__(256) void check_triangle_kernel(int64_t n, int is_lower, const I* __restrict__ rp,
                                                             const I* __restrict__ ci, int* __restrict__ status)
{
    const int64_t stride = int64_t(gridDim.x) * 256;
    const int64_t nnz = rp[n];
    int longest = 0;
    for (int64_t row = int64_t(blockIdx.x) * 256 + threadIdx.x; row < n; row += stride) {
        const int64_t begin = rp[row], end = rp[row + 1];
        if (begin < 0 || end < begin || end > nnz || (row == 0 && begin != 0)) {
            status[0] = 1;
            continue;
        }
        bool sound = true;
        for (int64_t k = begin; k < end; ++k) {
            const int64_t col = ci[k];
            if (col < 0 || col >= n) {
                status[1] = 1;
                sound = false;
            } else if (is_lower ? col > row : col < row) {
                status[2] = 1;
                sound = false;
            }
        }
        if (end == begin || (sound && int64_t(ci[is_lower ? end - 1 : begin]) != row)) status[3] = 1;
        const int64_t len = end - begin;
        longest = len > longest ? int(len > INT_MAX ? INT_MAX : len) : longest;
    }
    longest = wave_max(longest);
    if ((threadIdx.x & (wave_size - 1)) == 0 && longest > 0) atomicMax(&status[4], longest);
}

struct scratch_guard {
    hipStream_t st;
    void* ptr;
    ~scratch_guard()
    {
        if (ptr) (void)scratch_free(st, ptr);
    }
};

inline unsigned capped_grid(int64_t blocks)
{
    if (blocks > 4 * max_stream_blocks) blocks = 4 * max_stream_blocks;
    return unsigned(blocks < 1 ? 1 : blocks);
}

template <bool LOWER, int W, typename T, typename I>
int tri_inverse_launch(hipStream_t st, int64_t n, const I* a_rp, const I* a_ci, const T* a_v, const I* w_rp,
                       const I* w_ci, T* w_v)
{
    tri_inverse_kernel<LOWER, W, T, I><<<dim3(capped_grid(ceildiv(n, isai_block / W))), dim3(isai_block), 0, st>>>(
        n, a_rp, a_ci, a_v, w_rp, w_ci, w_v);
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

template <bool LOWER, typename T, typename I>
int tri_inverse_width(hipStream_t st, int longest, int64_t n, const I* a_rp, const I* a_ci, const T* a_v,
                      const I* w_rp, const I* w_ci, T* w_v)
{
    if (longest <= isai_row_limits[0]) return tri_inverse_launch<LOWER, 16, T, I>(st, n, a_rp, a_ci, a_v, w_rp, w_ci, w_v);
    if (longest <= isai_row_limits[1]) return tri_inverse_launch<LOWER, 32, T, I>(st, n, a_rp, a_ci, a_v, w_rp, w_ci, w_v);
    return tri_inverse_launch<LOWER, 64, T, I>(st, n, a_rp, a_ci, a_v, w_rp, w_ci, w_v);
}

template <typename T, typename I>
int generate_tri_inverse(gkoc_stream_t s, int64_t n, int is_lower, const I* a_rp, const I* a_ci, const T* a_v,
                         const I* w_rp, const I* w_ci, T* w_v)
{
    GKOC_REQUIRE(n >= 0, GKOC_E_INVALID, "negative number of rows");
    if (n == 0) return GKOC_OK;
    GKOC_REQUIRE(a_rp && a_ci && a_v && w_rp && w_ci && w_v, GKOC_E_INVALID, "null pointer");
    hipStream_t st = as_stream(s);
    // scratch: 5 status words for A, 5 for the pattern
    constexpr int words = 5;
    void* raw = nullptr;
    GKOC_TRY(scratch_malloc(st, &raw, 2 * words * sizeof(int)));
    scratch_guard guard{st, raw};
    int* status = static_cast<int*>(raw);
    GKOC_HIP(hipMemsetAsync(status, 0, 2 * words * sizeof(int), st));
    const unsigned grid = capped_grid(ceildiv(n, 256));
    check_triangle_kernel<I><<<dim3(grid), dim3(256), 0, st>>>(n, is_lower, a_rp, a_ci, status);
    GKOC_LAUNCH_OK();
    if (w_rp != a_rp || w_ci != a_ci) {
        check_triangle_kernel<I><<<dim3(grid), dim3(256), 0, st>>>(n, is_lower, w_rp, w_ci, status + words);
        GKOC_LAUNCH_OK();
    }
    int host[2 * words] = {};
    GKOC_HIP(hipMemcpyAsync(host, status, sizeof(host), hipMemcpyDeviceToHost, st));
    GKOC_HIP(hipStreamSynchronize(st));
    if (w_rp == a_rp && w_ci == a_ci) host[words + 4] = host[4];
    for (int m = 0; m < 2; ++m) {
        const int* h = host + m * words;
        GKOC_REQUIRE(h[0] == 0, GKOC_E_INVALID,
                     m ? "the pattern's row pointers do not ascend from 0" : "A's row pointers do not ascend from 0");
        GKOC_REQUIRE(h[1] == 0, GKOC_E_INVALID,
                     m ? "the pattern has a column outside the matrix" : "A has a column outside the matrix");
        GKOC_REQUIRE(h[2] == 0, GKOC_E_INVALID,
                     m ? "the pattern has an entry on the wrong side of the diagonal"
                       : "A has an entry on the wrong side of the diagonal");
        GKOC_REQUIRE(h[3] == 0, GKOC_E_INVALID,
                     m ? "a pattern row whose last (lower) / first (upper) entry is not its diagonal"
                       : "a row of A whose last (lower) / first (upper) entry is not its diagonal");
    }
    const int longest = host[words + 4];
    if (is_lower) return tri_inverse_width<true, T, I>(st, longest, n, a_rp, a_ci, a_v, w_rp, w_ci, w_v);
    return tri_inverse_width<false, T, I>(st, longest, n, a_rp, a_ci, a_v, w_rp, w_ci, w_v);
}

}  // namespace
}  // namespace gkoc

using namespace gkoc;

extern "C" int gkoc_isai_row_limits(int* limits_host, int* count_host)
{
    GKOC_REQUIRE(limits_host && count_host, GKOC_E_INVALID, "null pointer");
    constexpr int count = int(sizeof(isai_row_limits) / sizeof(isai_row_limits[0]));
    for (int p = 0; p < count; ++p) limits_host[p] = isai_row_limits[p];
    *count_host = count;
    return GKOC_OK;
}

#define GKOC_DEF_ISAI(T, TN, I, IN)                                                                            \
    extern "C" int gkoc_isai_generate_tri_inverse_##TN##_##IN(gkoc_stream_t s, int64_t n_rows, int is_lower,   \
                                                              const I* a_rp, const I* a_ci, const T* a_v,      \
                                                              const I* w_rp, const I* w_ci, T* w_v)            \
    {                                                                                                          \
        return generate_tri_inverse<T, I>(s, n_rows, is_lower, a_rp, a_ci, a_v, w_rp, w_ci, w_v);              \
    }
GKOC_DEF_ISAI(double, f64, int32_t, i32)
GKOC_DEF_ISAI(double, f64, int64_t, i64)
GKOC_DEF_ISAI(float, f32, int32_t, i32)
GKOC_DEF_ISAI(float, f32, int64_t, i64)
