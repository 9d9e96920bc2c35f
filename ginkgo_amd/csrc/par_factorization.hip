// ILU(0) / IC(0) by fixed-point sweeps (factorization::ParIlu / ParIc; Chow, Patel, "Fine-grained parallel
// incomplete LU factorization", SIAM J. Sci. Comput. 37, 2015), without a level schedule:
//   par_ilu_sweeps / par_ic_sweeps                  `iterations` row-synchronous sweeps, one launch each
//   par_ilu_sweeps_from / par_ic_sweeps_from        the same from a given iterate v^0 (ParIlut / ParIct)
//
// Contract (include/gko_cdna4.h; -ffp-contract=off keeps multiply and subtract apart), rows sorted: sweep t
// computes EVERY row with the sequential row step of the exact contract (factorization.hip).  Values of other
// rows, pivots included, are the ones of sweep t-1 (`prev`; sweep 1: v^0, which is the input a unless the _from
// entry gives another); the values of the row itself
// start from the input a and are the ones just computed in this sweep.
//   ILU: w = a(row i); for every stored k < i ascending: w_ik = w_ik / prev_kk, then for every stored j > k of
//        row k with (i, j) stored: w_ij = w_ij - w_ik * prev_kj.
//   IC:  lower-triangular input, diagonal last.  For every stored (i, j), columns ascending: s = a_ij; for
//        ascending k < j with (i, k) and (j, k) stored: s = s - w_ik * prev_jk (j = i: s - w_ik * w_ik);
//        w_ij = s / prev_jj (j < i), w_ii = sqrt(s).
// Pivots are not checked and nothing is guarded by "is finite": an entry is a function of a and prev alone.
// After as many sweeps as the lower solve's schedule has levels the result is the exact factorization, bit for
// bit, and stays it (every row of a level < t is computed by the exact row step from finished rows).
//
// A sweep is ONE launch over all rows, grid-stride.  A group of W lanes (16, 32 or 64, from the longest row of
// the matrix, at the limits of the exact kernels) takes one row, lane = stored entry, the value in a register.
// t runs over the row's lower entries: the owner of w_ik divides it by the pivot of row k in prev and the group
// gets it by a shuffle; every lane right of it looks its own column up in row k by a binary search (IC: column
// k in row j; the diagonal lane squares w_ik) and subtracts.  This is factorize_row of factorization.hip with
// two pointers instead of one.  A row longer than 64 entries (W is 64 then) is streamed: lane l owns the
// entries l, l + 64, ..., copies them from a to next first and updates them in next; other rows are read from
// prev only; the finished w_ik still travels by shuffle.  Trip counts per group are bounded by the row's own
// length and the logarithm of another row's.
//
// Invariants:
//   1. every entry of `next` is written by exactly one lane (and read back by that lane alone); no atomics on
//      values - the one atomic adds a wave's count of changed entries to the optional counter;
//   2. no kernel reads a value that another workgroup writes in the same launch: prev and a are
//      const T* __restrict__ and are not written by the sweep, next is not read outside the writing lane; the
//      entry refuses buffers that overlap;
//   3. the dependency between two sweeps is the kernel boundary on the stream;
//   4. no entry writes an index array.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "sparse_rows.hpp"

namespace gkoc {
namespace {

constexpr int sweep_block = 256;

__device__ __forceinline__ bool same_bits(double a, double b)
{
    return __double_as_longlong(a) == __double_as_longlong(b);
}
__device__ __forceinline__ bool same_bits(float a, float b) { return __float_as_int(a) == __float_as_int(b); }

// The update of entry (row, col) of the own row by its finished w_ik of column k, from the previous sweep:
//   ILU: prev_kj of row k right of its diagonal (diag_k = position of the pivot of row k).
//   IC:  prev_jk of row j = col left of its diagonal; on the diagonal lane w_ik itself.
template <bool IC, typename T, typename I>
__device__ __forceinline__ T swept(T v, T w_ik, int64_t row, int64_t col, int64_t k, int64_t diag_k,
                                   const I* __restrict__ rp, const I* __restrict__ ci,
                                   const T* __restrict__ prev)
{
    if (IC) {
        if (col == row) return v - w_ik * w_ik;
        const int64_t pos = find_column(ci, int64_t(rp[col]), int64_t(rp[col + 1]) - 1, k);
        return pos >= 0 ? v - w_ik * prev[pos] : v;
    }
    const int64_t pos = find_column(ci, diag_k + 1, int64_t(rp[k + 1]), col);
    return pos >= 0 ? v - w_ik * prev[pos] : v;
}

// one row by one group of W lanes; `lane` in [0, W).  Returns, with `count`, the number of this lane's entries
// whose bits differ from prev's.
template <bool IC, int W, typename T, typename I>
__device__ __forceinline__ int sweep_row(int64_t row, int lane, const I* __restrict__ rp,
                                         const I* __restrict__ ci, const I* __restrict__ diag,
                                         const T* __restrict__ a, const T* __restrict__ prev,
                                         T* __restrict__ next, bool count)
{
    const int64_t begin = rp[row];
    const int len = int(int64_t(rp[row + 1]) - begin);
    const int n_lower = IC ? len - 1 : int(int64_t(diag[row]) - begin);
    int differs = 0;
    if (len <= W) {
        const bool valid = lane < len;
        const long long col = valid ? (long long)(ci[begin + lane]) : -1LL;
        T v = valid ? a[begin + lane] : T(0);
        for (int t = 0; t < n_lower; ++t) {
            const int64_t k = __shfl(col, t, W);
            const int64_t diag_k = IC ? int64_t(rp[k + 1]) - 1 : int64_t(diag[k]);
            if (lane == t) v = v / prev[diag_k];
            const T w_ik = __shfl(v, t, W);
            if (valid && lane > t) v = swept<IC, T, I>(v, w_ik, row, col, k, diag_k, rp, ci, prev);
        }
        if (IC && lane == len - 1) v = root_of(v);
        if (valid) {
            next[begin + lane] = v;
            if (count) differs = same_bits(v, prev[begin + lane]) ? 0 : 1;
        }
    } else if (W == wave_size) {
        // streamed: lane l owns the entries l, l + W, ... and keeps them in next
        for (int e = lane; e < len; e += W) next[begin + e] = a[begin + e];
        for (int t = 0; t < n_lower; ++t) {
            const int64_t k = ci[begin + t];
            const int64_t diag_k = IC ? int64_t(rp[k + 1]) - 1 : int64_t(diag[k]);
            const int owner = t & (W - 1);
            T v = T(0);
            if (lane == owner) {
                v = next[begin + t] / prev[diag_k];
                next[begin + t] = v;
            }
            const T w_ik = __shfl(v, owner, W);
            for (int e = t + 1 + ((lane - (t + 1)) & (W - 1)); e < len; e += W) {
                next[begin + e] =
                    swept<IC, T, I>(next[begin + e], w_ik, row, int64_t(ci[begin + e]), k, diag_k, rp, ci, prev);
            }
        }
        if (IC && lane == ((len - 1) & (W - 1))) next[begin + len - 1] = root_of(next[begin + len - 1]);
        if (count) {
            for (int e = lane; e < len; e += W) differs += same_bits(next[begin + e], prev[begin + e]) ? 0 : 1;
        }
    }
    return differs;
}

// one sweep: all rows, spread over the grid.  `changed` (null except in the last sweep of a call) receives the
// number of entries that differ from prev.
template <bool IC, int W, typename T, typename I>
__global__ __launch_bounds__(sweep_block) void par_sweep_kernel(int64_t n, const I* __restrict__ rp,
                                                                const I* __restrict__ ci,
                                                                const I* __restrict__ diag,
                                                                const T* __restrict__ a,
                                                                const T* __restrict__ prev, T* __restrict__ next,
                                                                unsigned long long* __restrict__ changed)
{
    constexpr int groups = sweep_block / W;
    const int lane = threadIdx.x % W;
    const int64_t stride = int64_t(gridDim.x) * groups;
    const bool count = changed != nullptr;
    long long differs = 0;
    for (int64_t row = int64_t(blockIdx.x) * groups + threadIdx.x / W; row < n; row += stride) {
        differs += sweep_row<IC, W, T, I>(row, lane, rp, ci, diag, a, prev, next, count);
    }
    if (count) {
        differs = wave_sum(differs);
        if ((threadIdx.x & (wave_size - 1)) == 0 && differs > 0) {
            atomicAdd(changed, static_cast<unsigned long long>(differs));
        }
    }
}

template <bool IC, int W, typename T, typename I>
int sweeps_launch(hipStream_t st, int64_t n, const I* rp, const I* ci, const I* diag, const T* a, const T* v0,
                  int64_t iterations, T* work, T* out, uint64_t* changed)
{
    const unsigned blocks = stream_grid(n, sweep_block / W);
    for (int64_t t = 1; t <= iterations; ++t) {
        // sweep t writes out if iterations - t is even: the last one always does
        const bool to_out = (iterations - t) % 2 == 0;
        T* next = to_out ? out : work;
        const T* prev = t == 1 ? v0 : (to_out ? work : out);
        par_sweep_kernel<IC, W, T, I><<<dim3(blocks), dim3(sweep_block), 0, st>>>(
            n, rp, ci, diag, a, prev, next,
            t == iterations ? reinterpret_cast<unsigned long long*>(changed) : nullptr);
        GKOC_LAUNCH_OK();
    }
    return GKOC_OK;
}

inline bool overlap(const void* p, const void* q, size_t bytes)
{
    const char* a = static_cast<const char*>(p);
    const char* b = static_cast<const char*>(q);
    return a < b ? size_t(b - a) < bytes : size_t(a - b) < bytes;
}

template <bool IC, typename T, typename I>
int par_sweeps(gkoc_stream_t s, int64_t n, int64_t nnz, const I* rp, const I* ci, const T* a, const T* v0,
               int64_t iterations, T* work, T* out, uint64_t* changed)
{
    GKOC_REQUIRE(iterations >= 1, GKOC_E_INVALID, "fewer than one sweep");
    GKOC_REQUIRE(n >= 0 && nnz >= 0, GKOC_E_INVALID, "negative number of rows or of stored entries");
    hipStream_t st = as_stream(s);
    if (n == 0) {
        if (changed) GKOC_HIP(hipMemsetAsync(changed, 0, sizeof(uint64_t), st));
        return GKOC_OK;
    }
    GKOC_REQUIRE(nnz >= n, GKOC_E_INVALID, "fewer stored entries than rows: a row without a stored diagonal");
    GKOC_REQUIRE(rp && ci && a && v0 && out, GKOC_E_INVALID, "null pointer");
    GKOC_REQUIRE(work || iterations == 1, GKOC_E_INVALID, "more than one sweep needs the work buffer");
    const size_t bytes = sizeof(T) * size_t(nnz);
    GKOC_REQUIRE(!overlap(a, out, bytes) && (!work || (!overlap(a, work, bytes) && !overlap(work, out, bytes))),
                 GKOC_E_INVALID, "a_vals, work and out_vals must be three separate buffers");
    GKOC_REQUIRE(v0 == a || (!overlap(v0, out, bytes) && (!work || !overlap(v0, work, bytes))), GKOC_E_INVALID,
                 "v0_vals must not overlap work or out_vals");
    // scratch: 4 status words, then the diagonal positions
    status_words<4> status(st);
    GKOC_TRY(status.init(sizeof(I) * size_t(n)));
    I* diag = status.template behind<I>();
    locate_diagonals_kernel<I><<<dim3(stream_grid(n)), dim3(256), 0, st>>>(n, nnz, rp, ci, diag, status.dev);
    GKOC_LAUNCH_OK();
    GKOC_TRY(status.read());
    GKOC_REQUIRE(status[0] == 0, GKOC_E_INVALID,
                 "row pointers that do not ascend from 0 to nnz, or a column outside the matrix");
    GKOC_REQUIRE(status[1] == 0, GKOC_E_INVALID, "a row without a stored diagonal");
    GKOC_REQUIRE(!IC || status[2] == 0, GKOC_E_INVALID, "a row whose last entry is not its diagonal");
    if (changed) GKOC_HIP(hipMemsetAsync(changed, 0, sizeof(uint64_t), st));
    return with_lanes(status[3], fact_row_limits, [&](auto w) {
        return sweeps_launch<IC, decltype(w)::value, T, I>(st, n, rp, ci, diag, a, v0, iterations, work, out, changed);
    });
}

}  // namespace
}  // namespace gkoc

using namespace gkoc;

// the plain entries are the _from ones with v^0 = a
#define GKOC_DEF_PAR_SWEEPS(KIND, IC, T, TN, I, IN)                                                            \
    extern "C" int gkoc_par_##KIND##_sweeps_##TN##_##IN(gkoc_stream_t s, int64_t n_rows, int64_t nnz,          \
                                                        const I* row_ptrs, const I* col_idxs, const T* a_vals, \
                                                        int64_t iterations, T* work, T* out_vals,              \
                                                        uint64_t* changed_dev)                                 \
    {                                                                                                          \
        return par_sweeps<IC, T, I>(s, n_rows, nnz, row_ptrs, col_idxs, a_vals, a_vals, iterations, work,      \
                                    out_vals, changed_dev);                                                    \
    }                                                                                                          \
    extern "C" int gkoc_par_##KIND##_sweeps_from_##TN##_##IN(                                                  \
        gkoc_stream_t s, int64_t n_rows, int64_t nnz, const I* row_ptrs, const I* col_idxs, const T* a_vals,   \
        const T* v0_vals, int64_t iterations, T* work, T* out_vals, uint64_t* changed_dev)                     \
    {                                                                                                          \
        return par_sweeps<IC, T, I>(s, n_rows, nnz, row_ptrs, col_idxs, a_vals, v0_vals, iterations, work,     \
                                    out_vals, changed_dev);                                                    \
    }
#define GKOC_DEF_PAR_FACTORIZATION(T, TN, I, IN)     \
    GKOC_DEF_PAR_SWEEPS(ilu, false, T, TN, I, IN)    \
    GKOC_DEF_PAR_SWEEPS(ic, true, T, TN, I, IN)
GKOC_DEF_PAR_FACTORIZATION(double, f64, int32_t, i32)
GKOC_DEF_PAR_FACTORIZATION(double, f64, int64_t, i64)
GKOC_DEF_PAR_FACTORIZATION(float, f32, int32_t, i32)
GKOC_DEF_PAR_FACTORIZATION(float, f32, int64_t, i64)
