// Exact incomplete factorizations on the matrix' own pattern, and the split of a factored matrix:
//   ilu_factorize / ic_factorize                    ILU(0) / IC(0) in place (factorization::Ilu / Ic)
//   factorization::initialize_l_u, initialize_l     reference/factorization/factorization_kernels.cpp (values)
//
// Contract (it fixes the rounding; -ffp-contract=off keeps multiply and subtract apart), rows sorted:
//   ILU(0): for i = 0 .. n-1, for every stored k < i ascending: a_ik = a_ik / a_kk, then for every stored
//           j > k of row k with (i, j) stored: a_ij = a_ij - a_ik * a_kj.
//   IC(0):  lower-triangular input, diagonal last.  For every stored (i, j), columns ascending: s = a_ij;
//           for ascending k < j with (i, k) and (j, k) stored: s = s - l_ik * l_jk; l_ij = s / l_jj (j < i),
//           l_ii = sqrt(s).
// Both say the same thing about one entry: it receives its updates in ascending k, and a lower entry is
// divided once, after its last update.  Pivots are not checked (inf / NaN propagate).
//
// Schedule: the one of the lower triangular solve of the same matrix (trs.hip) - row i needs exactly the
// finished rows k < i with (i, k) stored.  wide level = one launch over many workgroups, run of narrow
// levels = one launch of ONE workgroup with __syncthreads() between the levels.
//
// Inside a level a group of W lanes (16, 32 or 64, from the longest row of the matrix) takes one row,
// lane = stored entry, the value in a register.  t runs over the row's lower entries: the owner of a_ik
// divides it by the pivot of row k and the group gets it by a shuffle; every lane right of it looks its own
// column up in row k by a binary search (IC: column k in its own row j; the diagonal lane squares l_ik)
// and subtracts.  A row longer than 64 entries (W is 64 then) is streamed: lane l owns the entries l,
// l + 64, ... and updates them in memory, the finished a_ik still travels by shuffle.
//
// Invariants:
//   1. every entry is written by exactly one lane, no atomics on values;
//   2. an entry's updates happen in ascending k (t ascends, rows are sorted);
//   3. a dependency between workgroups is a kernel boundary - no kernel waits for another workgroup's store;
//   4. `vals` is read (finished rows) and written (own row) in the same kernel, so it is ONE plain pointer,
//      neither const nor __restrict__: no load of it may take the scalar cache or the read-only path.  In
//      the narrow kernel finished rows are handed from wave to wave of one workgroup through global memory
//      exactly like x in trs.hip (one CU, one L1, write-through stores, __syncthreads() around the barrier).
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "sparse_rows.hpp"
#include "trs_struct.hpp"

namespace gkoc {
namespace {

constexpr int fact_narrow_block = 1024;
constexpr int fact_wide_block = 256;

// The update of entry (row, col) by the finished a_ik / l_ik of column k.
//   ILU: a_kj of row k right of its diagonal (diag_k = position of a_kk).
//   IC:  l_jk of row j = col left of its diagonal; on the diagonal lane l_ik itself.
template <bool IC, typename T, typename I>
__device__ __forceinline__ T updated(T v, T a_ik, int64_t row, int64_t col, int64_t k, int64_t diag_k,
                                     const I* __restrict__ rp, const I* __restrict__ ci, T* vals)
{
    if (IC) {
        if (col == row) return v - a_ik * a_ik;
        const int64_t pos = find_column(ci, int64_t(rp[col]), int64_t(rp[col + 1]) - 1, k);
        return pos >= 0 ? v - a_ik * vals[pos] : v;
    }
    const int64_t pos = find_column(ci, diag_k + 1, int64_t(rp[k + 1]), col);
    return pos >= 0 ? v - a_ik * vals[pos] : v;
}

// one row by one group of W lanes; `lane` in [0, W)
template <bool IC, int W, typename T, typename I>
__device__ __forceinline__ void factorize_row(int64_t row, int lane, const I* __restrict__ rp,
                                              const I* __restrict__ ci, const I* __restrict__ diag, T* vals)
{
    const int64_t begin = rp[row];
    const int len = int(int64_t(rp[row + 1]) - begin);
    const int n_lower = IC ? len - 1 : int(int64_t(diag[row]) - begin);
    if (len <= W) {
        const bool valid = lane < len;
        const long long col = valid ? (long long)(ci[begin + lane]) : -1LL;
        T v = valid ? vals[begin + lane] : T(0);
        for (int t = 0; t < n_lower; ++t) {
            const int64_t k = __shfl(col, t, W);
            const int64_t diag_k = IC ? int64_t(rp[k + 1]) - 1 : int64_t(diag[k]);
            if (lane == t) v = v / vals[diag_k];
            const T a_ik = __shfl(v, t, W);
            if (valid && lane > t) v = updated<IC, T, I>(v, a_ik, row, col, k, diag_k, rp, ci, vals);
        }
        if (IC && lane == len - 1) v = root_of(v);
        if (valid) vals[begin + lane] = v;
    } else if (W == wave_size) {
        // streamed: lane l owns the entries l, l + W, ... and keeps them in memory
        for (int t = 0; t < n_lower; ++t) {
            const int64_t k = ci[begin + t];
            const int64_t diag_k = IC ? int64_t(rp[k + 1]) - 1 : int64_t(diag[k]);
            const int owner = t & (W - 1);
            T v = T(0);
            if (lane == owner) {
                v = vals[begin + t] / vals[diag_k];
                vals[begin + t] = v;
            }
            const T a_ik = __shfl(v, owner, W);
            for (int e = t + 1 + ((lane - (t + 1)) & (W - 1)); e < len; e += W) {
                vals[begin + e] =
                    updated<IC, T, I>(vals[begin + e], a_ik, row, int64_t(ci[begin + e]), k, diag_k, rp, ci, vals);
            }
        }
        if (IC && lane == ((len - 1) & (W - 1))) vals[begin + len - 1] = root_of(vals[begin + len - 1]);
    }
}

// one level, rows spread over the grid
template <bool IC, int W, typename T, typename I>
__global__ __launch_bounds__(fact_wide_block) void factorize_wide_kernel(
    int64_t rows, const int64_t* __restrict__ level_rows /* of this level */, const I* __restrict__ rp,
    const I* __restrict__ ci, const I* __restrict__ diag, T* vals)
{
    constexpr int groups = fact_wide_block / W;
    const int lane = threadIdx.x % W;
    const int64_t stride = int64_t(gridDim.x) * groups;
    for (int64_t r = int64_t(blockIdx.x) * groups + threadIdx.x / W; r < rows; r += stride) {
        factorize_row<IC, W, T, I>(level_rows[r], lane, rp, ci, diag, vals);
    }
}

// levels [l0, l1) in ONE workgroup; launched with a grid of 1
template <bool IC, int W, typename T, typename I>
__global__ __launch_bounds__(fact_narrow_block) void factorize_narrow_kernel(
    int64_t l0, int64_t l1, const int64_t* __restrict__ level_ptrs, const int64_t* __restrict__ level_rows,
    const I* __restrict__ rp, const I* __restrict__ ci, const I* __restrict__ diag, T* vals)
{
    constexpr int groups = fact_narrow_block / W;
    const int lane = threadIdx.x % W;
    int64_t first = level_ptrs[l0];
    for (int64_t l = l0; l < l1; ++l) {
        const int64_t next = level_ptrs[l + 1];
        for (int64_t r = first + threadIdx.x / W; r < next; r += groups) {
            factorize_row<IC, W, T, I>(level_rows[r], lane, rp, ci, diag, vals);
        }
        first = next;
        // this level's rows for the next level's groups of this workgroup (uniform: l0, l1 are arguments)
        __syncthreads();
    }
}

template <bool IC, int W, typename T, typename I>
int factorize_launch(hipStream_t st, gkoc_trs_struct_t t, const I* rp, const I* ci, const I* diag, T* vals)
{
    for (const auto& seg : t->schedule) {
        if (seg.rows == 0) continue;
        if (seg.wide) {
            factorize_wide_kernel<IC, W, T, I>
                <<<dim3(stream_grid(seg.rows, fact_wide_block / W)), dim3(fact_wide_block), 0, st>>>(
                seg.rows, t->level_rows + seg.offset, rp, ci, diag, vals);
        } else {
            factorize_narrow_kernel<IC, W, T, I><<<dim3(1), dim3(fact_narrow_block), 0, st>>>(
                seg.first, seg.last, t->level_ptrs, t->level_rows, rp, ci, diag, vals);
        }
        GKOC_LAUNCH_OK();
    }
    return GKOC_OK;
}

template <bool IC, typename T, typename I>
int factorize(gkoc_stream_t s, gkoc_trs_struct_t t, int64_t n, const I* rp, const I* ci, T* vals)
{
    GKOC_REQUIRE(t, GKOC_E_INVALID, "null triangular-solve structure");
    GKOC_REQUIRE(n >= 0, GKOC_E_INVALID, "negative number of rows");
    GKOC_REQUIRE(t->is_upper == 0, GKOC_E_INVALID, "the structure was generated for the upper triangle");
    GKOC_REQUIRE(t->n_rows == n, GKOC_E_INVALID, "the structure was generated for another number of rows");
    if (n == 0) return GKOC_OK;
    GKOC_REQUIRE(t->nnz >= n, GKOC_E_INVALID, "fewer stored entries than rows: a row without a stored diagonal");
    GKOC_REQUIRE(rp && ci && vals, GKOC_E_INVALID, "null pointer");
    hipStream_t st = as_stream(s);
    // scratch: 4 status words, then the diagonal positions
    status_words<4> status(st);
    GKOC_TRY(status.init(sizeof(I) * size_t(n)));
    I* diag = status.template behind<I>();
    locate_diagonals_kernel<I><<<dim3(stream_grid(n)), dim3(256), 0, st>>>(n, t->nnz, rp, ci, diag, status.dev);
    GKOC_LAUNCH_OK();
    GKOC_TRY(status.read());
    GKOC_REQUIRE(status[0] == 0, GKOC_E_INVALID,
                 "row pointers or column indices do not fit the matrix the structure was generated for");
    GKOC_REQUIRE(status[1] == 0, GKOC_E_INVALID, "a row without a stored diagonal");
    GKOC_REQUIRE(!IC || status[2] == 0, GKOC_E_INVALID, "a row whose last entry is not its diagonal");
    return with_lanes(status[3], fact_row_limits, [&](auto w) {
        return factorize_launch<IC, decltype(w)::value, T, I>(st, t, rp, ci, diag, vals);
    });
}


// ------------------------------------------------------------------ the split (one thread per row)
// The VALUES of the split; the index arrays of L and U are those of the Sor set-up (trs.hip: the same
// row pointers, strictly-lower columns then the diagonal, the diagonal then the strictly-upper columns), so
// no entry of this file writes an index array.
// l_v = strictly-lower values in storage order, then the diagonal: 1 (WITH_U) or a_ii / sqrt(a_ii);
// with WITH_U also u_v = a_ii, then the strictly-upper values in storage order.  A missing a_ii counts as 1.
template <bool WITH_U, typename T, typename I>
__global__ __launch_bounds__(256) void split_kernel(int64_t n, const I* __restrict__ rp,
                                                    const I* __restrict__ ci, const T* __restrict__ v,
                                                    const I* __restrict__ l_rp, T* __restrict__ l_v,
                                                    const I* __restrict__ u_rp, T* __restrict__ u_v,
                                                    int diag_sqrt)
{
    const int64_t stride = int64_t(gridDim.x) * 256;
    for (int64_t row = int64_t(blockIdx.x) * 256 + threadIdx.x; row < n; row += stride) {
        const int64_t begin = rp[row], end = rp[row + 1];
        T diag = T(1);
        int64_t lp = l_rp[row];
        int64_t up = WITH_U ? int64_t(u_rp[row]) + 1 : 0;
        for (int64_t k = begin; k < end; ++k) {
            const int64_t col = ci[k];
            if (col < row) {
                l_v[lp++] = v[k];
            } else if (col == row) {
                diag = v[k];
            } else if (WITH_U) {
                u_v[up++] = v[k];
            }
        }
        l_v[lp] = WITH_U ? T(1) : (diag_sqrt ? root_of(diag) : diag);
        if (WITH_U) u_v[u_rp[row]] = diag;
    }
}

template <bool WITH_U, typename T, typename I>
int split(gkoc_stream_t s, int64_t n, const I* rp, const I* ci, const T* v, const I* l_rp, T* l_v,
          const I* u_rp, T* u_v, int diag_sqrt)
{
    GKOC_REQUIRE(n >= 0, GKOC_E_INVALID, "negative number of rows");
    if (n == 0) return GKOC_OK;
    GKOC_REQUIRE(rp && l_rp && l_v, GKOC_E_INVALID, "null pointer");
    GKOC_REQUIRE(!WITH_U || (u_rp && u_v), GKOC_E_INVALID, "null pointer");
    split_kernel<WITH_U, T, I><<<dim3(stream_grid(n)), dim3(256), 0, as_stream(s)>>>(n, rp, ci, v, l_rp, l_v, u_rp,
                                                                                   u_v, diag_sqrt);
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

}  // namespace
}  // namespace gkoc

using namespace gkoc;

extern "C" int gkoc_factorization_row_limits(int* limits_host, int* count_host)
{
    return export_row_limits(fact_row_limits, limits_host, count_host);
}

#define GKOC_DEF_FACTORIZATION(T, TN, I, IN)                                                                   \
    extern "C" int gkoc_ilu_factorize_##TN##_##IN(gkoc_stream_t s, gkoc_trs_struct_t t, int64_t n_rows,        \
                                                  const I* row_ptrs, const I* col_idxs, T* vals)               \
    {                                                                                                          \
        return factorize<false, T, I>(s, t, n_rows, row_ptrs, col_idxs, vals);                                 \
    }                                                                                                          \
    extern "C" int gkoc_ic_factorize_##TN##_##IN(gkoc_stream_t s, gkoc_trs_struct_t t, int64_t n_rows,         \
                                                 const I* row_ptrs, const I* col_idxs, T* vals)                \
    {                                                                                                          \
        return factorize<true, T, I>(s, t, n_rows, row_ptrs, col_idxs, vals);                                  \
    }                                                                                                          \
    extern "C" int gkoc_factorization_initialize_l_u_##TN##_##IN(                                              \
        gkoc_stream_t s, int64_t n_rows, const I* rp, const I* ci, const T* v, const I* l_rp, T* l_v,          \
        const I* u_rp, T* u_v)                                                                                 \
    {                                                                                                          \
        return split<true, T, I>(s, n_rows, rp, ci, v, l_rp, l_v, u_rp, u_v, 0);                               \
    }                                                                                                          \
    extern "C" int gkoc_factorization_initialize_l_##TN##_##IN(gkoc_stream_t s, int64_t n_rows, const I* rp,   \
                                                               const I* ci, const T* v, const I* l_rp,         \
                                                               T* l_v, int diag_sqrt)                          \
    {                                                                                                          \
        return split<false, T, I>(s, n_rows, rp, ci, v, l_rp, l_v, nullptr, nullptr, diag_sqrt);               \
    }
GKOC_DEF_FACTORIZATION(double, f64, int32_t, i32)
GKOC_DEF_FACTORIZATION(double, f64, int64_t, i64)
GKOC_DEF_FACTORIZATION(float, f32, int32_t, i32)
GKOC_DEF_FACTORIZATION(float, f32, int64_t, i64)
