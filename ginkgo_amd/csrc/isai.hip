// Incomplete sparse approximate inverses (preconditioner::LowerIsai / UpperIsai / GeneralIsai / SpdIsai):
//   isai_generate_tri_inverse      the VALUES of W on a given pattern, (W A)(i, S_i) = e_i(S_i) for every row i,
//                                  A triangular (reference/preconditioner/isai_kernels.cpp: generate_tri_inverse)
//   isai_generate_general_inverse  the same for any square A, and its scaled lower triangular form for an spd A
//                                  (generate_general_inverse; second half of this file)
//
// ---- the triangular entry ----
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
#include "sparse_rows.hpp"

namespace gkoc {
namespace {

constexpr int isai_block = 256;
constexpr int isai_row_limits[] = {16, 32, 64};

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
    note_longest(longest, &status[4]);
}

template <bool LOWER, int W, typename T, typename I>
int tri_inverse_launch(hipStream_t st, int64_t n, const I* a_rp, const I* a_ci, const T* a_v, const I* w_rp,
                       const I* w_ci, T* w_v)
{
    tri_inverse_kernel<LOWER, W, T, I><<<dim3(stream_grid(n, isai_block / W)), dim3(isai_block), 0, st>>>(
        n, a_rp, a_ci, a_v, w_rp, w_ci, w_v);
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

template <bool LOWER, typename T, typename I>
int tri_inverse_width(hipStream_t st, int longest, int64_t n, const I* a_rp, const I* a_ci, const T* a_v,
                      const I* w_rp, const I* w_ci, T* w_v)
{
    return with_lanes(longest, isai_row_limits, [&](auto w) {
        return tri_inverse_launch<LOWER, decltype(w)::value, T, I>(st, n, a_rp, a_ci, a_v, w_rp, w_ci, w_v);
    });
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
    status_words<2 * words> status(st);
    GKOC_TRY(status.init());
    const unsigned grid = stream_grid(n);
    check_triangle_kernel<I><<<dim3(grid), dim3(256), 0, st>>>(n, is_lower, a_rp, a_ci, status.dev);
    GKOC_LAUNCH_OK();
    if (w_rp != a_rp || w_ci != a_ci) {
        check_triangle_kernel<I><<<dim3(grid), dim3(256), 0, st>>>(n, is_lower, w_rp, w_ci, status.dev + words);
        GKOC_LAUNCH_OK();
    }
    GKOC_TRY(status.read());
    int* host = status.host;
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

// ---------------------------------------------------------------------------------------------------------
// General and spd ISAI (preconditioner::GeneralIsai / SpdIsai): isai_generate_general_inverse, the VALUES of W
// with (W A)(i, S_i) = e_i(S_i) for a square A that need not be triangular
// (reference/preconditioner/isai_kernels.cpp: generate_general_inverse).
//
// Contract (the arithmetic is stated in include/gko_cdna4.h and restated in numpy by
// tests/isai_general_refs.py).  Row i of the pattern has the columns c_0 < ... < c_{m-1}, i among them at
// position p (spd: every column <= i, so p = m-1).  The dense system is M[j][k] = a[c_k, c_j] (0 where A stores
// nothing) with the right-hand side e_p; it is solved by Gauss-Jordan with implicit partial pivoting: for
// col = 0 .. m-1 the pivot q is the row not yet used with the largest |M[r][col]| (a NaN counts as the largest,
// a tie goes to the smallest r), and every OTHER row r, used or not, takes f = M[r][col] / M[q][col],
// M[r][k] = M[r][k] - f * M[q][k] for k > col and rhs[r] = rhs[r] - f * rhs[q].  Then
// w[c_col] = rhs[q(col)] / M[q(col)][col]; spd: every w is divided by d = sqrt(w[c_{m-1}]); a row with a
// non-finite w becomes zeros with 1 at p.
//
// Thread = row r of M, M in LDS with the leading dimension W + 1 (cap + 1): a thread walks its own row
// (stride ld, an odd number of elements, so the rows start on different banks) and reads the pivot row as a
// broadcast.  An element
// M[r][k] is only ever written by the thread(s) of row r, in the order of col, so the layout does not touch
// the rounding.
//   rows of at most 64 entries: a group of W = 16, 32 or 64 lanes (from the longest pattern row of the call,
//     64 if it is longer) per row, isai_block / W rows per workgroup; the argmax and rhs[q] travel by shuffle,
//     the lanes of a group only ever meet inside their own wave (wave_lds_sync);
//   longer rows, up to general_cap = 128: one workgroup of 256 threads per row, TWO threads per row of M (the
//     halves t < 128 and t >= 128 take the even and the odd k of the update), argmax across the two waves of the
//     first half and rhs through LDS, __syncthreads between the columns.
// A call with rows on both sides of 64 launches both kernels, each skipping the other's rows.
// Invariants 1, 3 and 4 of the triangular kernel hold: one writer per entry of w_v, no atomics, every index
// pointer const.  LDS: 4 groups * 64 * 65 * 8 B = 133120 B (f64, W = 64) and 134424 B (f64, workgroup path:
// 128 * 129 + 2 * 128 values and the two pivot candidates) are the largest, both below the 160 KiB of a CU.
constexpr int general_row_limits[] = {16, 32, 64, 128};
constexpr int general_wave_cap = 64;
constexpr int general_cap = 128;
constexpr int general_block = 2 * general_cap;

// what the pivot search compares: |v|, a NaN as the largest
__device__ __forceinline__ double pivot_key(double v) { return v != v ? HUGE_VAL : __builtin_fabs(v); }
__device__ __forceinline__ float pivot_key(float v) { return v != v ? HUGE_VALF : __builtin_fabsf(v); }

// a[c_k, c_j], 0 if it is not stored
template <typename T, typename I>
__device__ __forceinline__ T entry_of_a(int64_t c_k, int64_t c_j, const I* __restrict__ a_rp,
                                        const I* __restrict__ a_ci, const T* __restrict__ a_v)
{
    const int64_t pos = find_column(a_ci, int64_t(a_rp[c_k]), int64_t(a_rp[c_k + 1]), c_j);
    return pos >= 0 ? a_v[pos] : T(0);
}

// the larger key, on a tie the smaller index
template <typename T>
__device__ __forceinline__ void better_pivot(T& key, int& q, T other_key, int other_q)
{
    if (other_key > key || (other_key == key && other_q < q)) {
        key = other_key;
        q = other_q;
    }
}

// the best (key, q) of the group of W lanes, in every lane
template <int W, typename T>
__device__ __forceinline__ void group_pivot(T& key, int& q)
{
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) {
        const T other_key = __shfl_xor(key, off, W);
        const int other_q = __shfl_xor(q, off, W);
        better_pivot(key, q, other_key, other_q);
    }
}

template <int W, typename T, typename I>
__global__ __launch_bounds__(isai_block) void general_inverse_wave_kernel(
    int64_t n, int spd, const I* __restrict__ a_rp, const I* __restrict__ a_ci, const T* __restrict__ a_v,
    const I* __restrict__ w_rp, const I* __restrict__ w_ci, T* __restrict__ w_v)
{
    constexpr int groups = isai_block / W, ld = W + 1;
    __shared__ T lds[groups * W * ld];
    const int lane = threadIdx.x % W;
    T* const m = lds + (threadIdx.x / W) * (W * ld);
    T* const mine = m + lane * ld;
    const int64_t stride = int64_t(gridDim.x) * groups;
    for (int64_t row = int64_t(blockIdx.x) * groups + threadIdx.x / W; row < n; row += stride) {
        const int64_t begin = w_rp[row];
        const int len = int(int64_t(w_rp[row + 1]) - begin);
        if (len > W) continue;          // the workgroup kernel's row
        const bool valid = lane < len;
        const long long col_mine = valid ? (long long)(w_ci[begin + lane]) : -1LL;
        const int p = group_max<W>(col_mine == row ? lane : -1);
        for (int k = 0; k < len; ++k) {
            const int64_t c_k = __shfl(col_mine, k, W);
            if (valid) mine[k] = entry_of_a<T, I>(c_k, col_mine, a_rp, a_ci, a_v);
        }
        T rhs = lane == p ? T(1) : T(0);
        int pivot_col = -1;             // the column this lane's row was the pivot of
        wave_lds_sync();
        for (int col = 0; col < len; ++col) {
            const T v = valid ? mine[col] : T(0);
            T key = valid && pivot_col < 0 ? pivot_key(v) : T(-1);
            int q = lane;
            group_pivot<W, T>(key, q);
            const T f = v / m[q * ld + col];
            const T rhs_q = __shfl(rhs, q, W);
            if (lane == q) {
                pivot_col = col;
            } else if (valid) {
                for (int k = col + 1; k < len; ++k) mine[k] = mine[k] - f * m[q * ld + k];
                rhs = rhs - f * rhs_q;
            }
            wave_lds_sync();
        }
        T w = valid ? rhs / mine[pivot_col] : T(0);
        if (spd) {
            const int last = group_max<W>(pivot_col == len - 1 ? lane : -1);
            w = w / root_of(__shfl(w, last, W));
        }
        if (group_any<W>(valid && !is_finite(w))) w = pivot_col == p ? T(1) : T(0);
        if (valid) w_v[begin + pivot_col] = w;
    }
}

template <typename T, typename I>
__global__ __launch_bounds__(general_block) void general_inverse_block_kernel(
    int64_t n, int spd, const I* __restrict__ a_rp, const I* __restrict__ a_ci, const T* __restrict__ a_v,
    const I* __restrict__ w_rp, const I* __restrict__ w_ci, T* __restrict__ w_v)
{
    constexpr int ld = general_cap + 1;
    __shared__ T m[general_cap * ld];
    __shared__ T rhs[general_cap];
    __shared__ T sol[general_cap];
    __shared__ T wave_key[2];
    __shared__ int wave_q[2];
    const int r = threadIdx.x % general_cap, half = threadIdx.x / general_cap;     // half is wave-uniform
    T* const mine = m + r * ld;
    for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
        const int64_t begin = w_rp[row];
        const int len = int(int64_t(w_rp[row + 1]) - begin);
        if (len <= general_wave_cap || len > general_cap) continue;    // the same for the whole workgroup
        const bool valid = r < len;
        const int64_t col_mine = valid ? int64_t(w_ci[begin + r]) : int64_t(-1);
        if (valid) {
            for (int k = half; k < len; k += 2) {
                mine[k] = entry_of_a<T, I>(int64_t(w_ci[begin + k]), col_mine, a_rp, a_ci, a_v);
            }
            if (half == 0) rhs[r] = col_mine == row ? T(1) : T(0);
        }
        int pivot_col = -1;
        __syncthreads();
        for (int col = 0; col < len; ++col) {
            const T v = valid ? mine[col] : T(0);
            if (half == 0) {
                T key = valid && pivot_col < 0 ? pivot_key(v) : T(-1);
                int q = r;
                group_pivot<wave_size, T>(key, q);
                if (r % wave_size == 0) {
                    wave_key[r / wave_size] = key;
                    wave_q[r / wave_size] = q;
                }
            }
            __syncthreads();
            // the first wave holds the smaller indices, so it keeps a tie
            const int q = wave_key[1] > wave_key[0] ? wave_q[1] : wave_q[0];
            const T f = v / m[q * ld + col];
            const T rhs_q = rhs[q];
            if (r == q) {
                pivot_col = col;
            } else if (valid) {
                for (int k = col + 1 + half; k < len; k += 2) mine[k] = mine[k] - f * m[q * ld + k];
                if (half == 0) rhs[r] = rhs[r] - f * rhs_q;
            }
            __syncthreads();
        }
        if (half == 0 && valid) sol[pivot_col] = rhs[r] / mine[pivot_col];
        __syncthreads();
        // from here thread t < len of the first half owns the entry t of the row
        T w = valid ? sol[r] : T(0);
        if (spd) w = w / root_of(sol[len - 1]);
        if (__syncthreads_or(valid && !is_finite(w))) w = col_mine == row ? T(1) : T(0);
        if (half == 0 && valid) w_v[begin + r] = w;
    }
}

// One thread per row of one index structure (A or the pattern).  status[0]: row pointers that do not ascend
// from 0, [1]: a column outside the matrix, [2]: a row that is not strictly ascending, [3]: a row without its
// diagonal, [4]: an entry right of the diagonal, [5]: the longest row.  A row is read only if its pointers are
// sound.
constexpr int general_status_words = 6;
template <typename I>
__global__ __launch_bounds__(256) void check_general_kernel(int64_t n, const I* __restrict__ rp,
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
        bool diagonal = false;
        int64_t before = -1;
        for (int64_t k = begin; k < end; ++k) {
            const int64_t col = ci[k];
            if (col < 0 || col >= n) status[1] = 1;
            if (k > begin && col <= before) status[2] = 1;
            if (col > row) status[4] = 1;
            diagonal = diagonal || col == row;
            before = col;
        }
        if (!diagonal) status[3] = 1;
        const int64_t len = end - begin;
        longest = len > longest ? int(len > INT_MAX ? INT_MAX : len) : longest;
    }
    note_longest(longest, &status[5]);
}

template <int W, typename T, typename I>
int general_inverse_wave_launch(hipStream_t st, int64_t n, int spd, const I* a_rp, const I* a_ci, const T* a_v,
                                const I* w_rp, const I* w_ci, T* w_v)
{
    general_inverse_wave_kernel<W, T, I><<<dim3(stream_grid(n, isai_block / W)), dim3(isai_block), 0, st>>>(
        n, spd, a_rp, a_ci, a_v, w_rp, w_ci, w_v);
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

template <typename T, typename I>
int generate_general_inverse(gkoc_stream_t s, int64_t n, int spd, const I* a_rp, const I* a_ci, const T* a_v,
                             const I* w_rp, const I* w_ci, T* w_v)
{
    GKOC_REQUIRE(n >= 0, GKOC_E_INVALID, "negative number of rows");
    if (n == 0) return GKOC_OK;
    GKOC_REQUIRE(a_rp && a_ci && a_v && w_rp && w_ci && w_v, GKOC_E_INVALID, "null pointer");
    hipStream_t st = as_stream(s);
    constexpr int words = general_status_words;
    status_words<2 * words> status(st);
    GKOC_TRY(status.init());
    const unsigned grid = stream_grid(n);
    const bool shared = w_rp == a_rp && w_ci == a_ci;
    if (!shared) {
        check_general_kernel<I><<<dim3(grid), dim3(256), 0, st>>>(n, a_rp, a_ci, status.dev);
        GKOC_LAUNCH_OK();
    }
    check_general_kernel<I><<<dim3(grid), dim3(256), 0, st>>>(n, w_rp, w_ci, status.dev + words);
    GKOC_LAUNCH_OK();
    GKOC_TRY(status.read());
    for (int m = shared ? 1 : 0; m < 2; ++m) {
        const int* h = status.host + m * words;
        GKOC_REQUIRE(h[0] == 0, GKOC_E_INVALID,
                     m ? "the pattern's row pointers do not ascend from 0" : "A's row pointers do not ascend from 0");
        GKOC_REQUIRE(h[1] == 0, GKOC_E_INVALID,
                     m ? "the pattern has a column outside the matrix" : "A has a column outside the matrix");
        GKOC_REQUIRE(h[2] == 0, GKOC_E_INVALID,
                     m ? "a pattern row is not sorted by column" : "a row of A is not sorted by column");
    }
    const int* h = status.host + words;
    GKOC_REQUIRE(h[3] == 0, GKOC_E_INVALID, "a pattern row without its diagonal");
    GKOC_REQUIRE(!spd || h[4] == 0, GKOC_E_INVALID, "spd: a pattern entry above the diagonal");
    const int longest = h[5];
    if (longest > general_cap) {
        set_last_error("%s:%d: a pattern row of %d entries; the dense solve takes rows of at most %d", __FILE__,
                       __LINE__, longest, general_cap);
        return GKOC_E_NOT_SUPPORTED;
    }
    GKOC_TRY(with_lanes(longest, general_row_limits, [&](auto w) {
        return general_inverse_wave_launch<decltype(w)::value, T, I>(st, n, spd, a_rp, a_ci, a_v, w_rp, w_ci, w_v);
    }));
    // a second launch for the rows above 64 entries; each kernel skips the other's rows
    if (longest > general_wave_cap) {
        general_inverse_block_kernel<T, I><<<dim3(stream_grid(n, 1)), dim3(general_block), 0, st>>>(
            n, spd, a_rp, a_ci, a_v, w_rp, w_ci, w_v);
        GKOC_LAUNCH_OK();
    }
    return GKOC_OK;
}

}  // namespace
}  // namespace gkoc

using namespace gkoc;

extern "C" int gkoc_isai_row_limits(int* limits_host, int* count_host)
{
    return export_row_limits(isai_row_limits, limits_host, count_host);
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

extern "C" int gkoc_isai_general_row_limits(int* limits_host, int* count_host)
{
    constexpr int count = int(sizeof(general_row_limits) / sizeof(general_row_limits[0]));
    static_assert(general_row_limits[count - 1] == general_cap && general_row_limits[count - 2] == general_wave_cap,
                  "the last limit is the cap, the one before it the last length of the wave path");
    return export_row_limits(general_row_limits, limits_host, count_host);
}

#define GKOC_DEF_ISAI_GENERAL(T, TN, I, IN)                                                                    \
    extern "C" int gkoc_isai_generate_general_inverse_##TN##_##IN(gkoc_stream_t s, int64_t n_rows, int spd,    \
                                                                  const I* a_rp, const I* a_ci, const T* a_v,  \
                                                                  const I* w_rp, const I* w_ci, T* w_v)        \
    {                                                                                                          \
        return generate_general_inverse<T, I>(s, n_rows, spd, a_rp, a_ci, a_v, w_rp, w_ci, w_v);               \
    }
GKOC_DEF_ISAI_GENERAL(double, f64, int32_t, i32)
GKOC_DEF_ISAI_GENERAL(double, f64, int64_t, i64)
GKOC_DEF_ISAI_GENERAL(float, f32, int32_t, i32)
GKOC_DEF_ISAI_GENERAL(float, f32, int64_t, i64)
