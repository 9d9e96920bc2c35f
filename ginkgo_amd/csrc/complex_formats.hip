// ELL and SELL-P products on complex values (ell::{spmv, advanced_spmv}, sellp::{spmv, advanced_spmv}
// for complex<float> / complex<double>; core/matrix/ell_kernels.hpp:20-34, sellp_kernels.hpp:20-31;
// semantics reference/matrix/ell_kernels.cpp:29-120, sellp_kernels.cpp:27-100).  Same argument lists
// as the real entries of formats.hip.  One lane per (row, right-hand side); consecutive lanes read
// consecutive rows of the column-major value / index arrays, i.e. coalesced - a complex product moves
// 16 + 4 bytes per stored entry and is bound by HBM with this layout as it stands (no LDS staging, no
// fragments: the tuned kernels of formats.hip exist for the real types the configurations use).
// A row's entries are added in storage order with the textbook complex product: the reference's
// result to rounding.  Padding (column -1) is skipped.  beta == 0 does not read c.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "fmt_rows.hpp"

namespace gkoc {
namespace {

template <typename T>
__device__ __forceinline__ void cx_store(T* __restrict__ c, bool adv, T alpha, T beta, T sum)
{
    if (!adv) {
        *c = sum;
    } else {
        const T ax = alpha * sum;
        *c = beta == T(0) ? ax : ax + beta * *c;
    }
}

// L: where a row's slots live (ell_rows or sellp_rows, fmt_rows.hpp)
template <typename T, typename I, typename L>
__global__ __launch_bounds__(256) void cx_fmt_spmv_kernel(int64_t rows, int64_t nrhs, L lay,
                                                         const I* __restrict__ cols,
                                                         const T* __restrict__ vals,
                                                         const T* __restrict__ alpha_p,
                                                         const T* __restrict__ b, int64_t ldb,
                                                         const T* __restrict__ beta_p, T* __restrict__ c,
                                                         int64_t ldc)
{
    const bool adv = alpha_p != nullptr;
    const T alpha = adv ? alpha_p[0] : T(1), beta = adv ? beta_p[0] : T(0);
    const int64_t total = rows * nrhs, grid_step = int64_t(gridDim.x) * 256;
    for (int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x; idx < total; idx += grid_step) {
        // rows fastest: the lanes of a wave read one contiguous run of every stored column
        const int64_t j = idx / rows, row = idx - j * rows;
        int64_t len, first, step;
        lay.locate(row, len, first, step);
        T sum = T(0);
        for (int64_t k = 0; k < len; ++k) {
            const I col = cols[first + k * step];
            if (col != I(-1)) sum += vals[first + k * step] * b[int64_t(col) * ldb + j];
        }
        cx_store(c + row * ldc + j, adv, alpha, beta, sum);
    }
}

inline unsigned blocks_for(int64_t n) { return capped_grid(n, 256, 8 * max_stream_blocks); }

// the one launcher; the entry points below have checked their arguments (alpha == nullptr: the plain product)
template <typename T, typename I, typename L>
int launch_cx_fmt(gkoc_stream_t s, int64_t n_rows, L lay, const T* alpha, const I* cols, const T* vals,
                  const T* b, int64_t ldb, const T* beta, T* c, int64_t ldc, int64_t nrhs)
{
    cx_fmt_spmv_kernel<T, I, L><<<dim3(blocks_for(n_rows * nrhs)), dim3(256), 0, as_stream(s)>>>(
        n_rows, nrhs, lay, cols, vals, alpha, b, ldb, beta, c, ldc);
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

}  // namespace
}  // namespace gkoc

using namespace gkoc;

#define GKOC_DEF_CFMT(T, TN, I, IN)                                                                       \
    extern "C" int gkoc_ell_spmv_##TN##_##IN(gkoc_stream_t s, int64_t n_rows, int64_t n_cols,             \
                                             int64_t per_row, int64_t stride, const I* col_idxs,          \
                                             const T* vals, const T* b, int64_t ldb, T* c, int64_t ldc,   \
                                             int64_t nrhs)                                                \
    {                                                                                                     \
        if (n_rows <= 0 || nrhs <= 0) return GKOC_OK;                                                     \
        GKOC_REQUIRE(per_row >= 0 && stride >= n_rows && c && (per_row == 0 || (col_idxs && vals && b)),  \
                     GKOC_E_INVALID, "bad argument");                                                     \
        return launch_cx_fmt<T, I>(s, n_rows, ell_rows{per_row, stride}, nullptr, col_idxs, vals, b, ldb, \
                                   nullptr, c, ldc, nrhs);                                                \
    }                                                                                                     \
    extern "C" int gkoc_ell_advanced_spmv_##TN##_##IN(                                                    \
        gkoc_stream_t s, int64_t n_rows, int64_t n_cols, int64_t per_row, int64_t stride, const T* alpha, \
        const I* col_idxs, const T* vals, const T* b, int64_t ldb, const T* beta, T* c, int64_t ldc,      \
        int64_t nrhs)                                                                                     \
    {                                                                                                     \
        if (n_rows <= 0 || nrhs <= 0) return GKOC_OK;                                                     \
        GKOC_REQUIRE(per_row >= 0 && stride >= n_rows && c && alpha && beta &&                            \
                         (per_row == 0 || (col_idxs && vals && b)),                                       \
                     GKOC_E_INVALID, "bad argument");                                                     \
        return launch_cx_fmt<T, I>(s, n_rows, ell_rows{per_row, stride}, alpha, col_idxs, vals, b, ldb,   \
                                   beta, c, ldc, nrhs);                                                   \
    }                                                                                                     \
    extern "C" int gkoc_sellp_spmv_##TN##_##IN(gkoc_stream_t s, int64_t n_rows, int64_t n_cols,           \
                                               int64_t slice_size, const uint64_t* slice_sets,            \
                                               const uint64_t* slice_lengths, const I* col_idxs,          \
                                               const T* vals, const T* b, int64_t ldb, T* c, int64_t ldc, \
                                               int64_t nrhs)                                              \
    {                                                                                                     \
        if (n_rows <= 0 || nrhs <= 0) return GKOC_OK;                                                     \
        GKOC_REQUIRE(slice_size > 0 && slice_sets && slice_lengths && c, GKOC_E_INVALID, "bad argument"); \
        return launch_cx_fmt<T, I>(s, n_rows, sellp_rows{slice_size, slice_sets, slice_lengths}, nullptr, \
                                   col_idxs, vals, b, ldb, nullptr, c, ldc, nrhs);                        \
    }                                                                                                     \
    extern "C" int gkoc_sellp_advanced_spmv_##TN##_##IN(                                                  \
        gkoc_stream_t s, int64_t n_rows, int64_t n_cols, int64_t slice_size, const T* alpha,              \
        const uint64_t* slice_sets, const uint64_t* slice_lengths, const I* col_idxs, const T* vals,      \
        const T* b, int64_t ldb, const T* beta, T* c, int64_t ldc, int64_t nrhs)                          \
    {                                                                                                     \
        if (n_rows <= 0 || nrhs <= 0) return GKOC_OK;                                                     \
        GKOC_REQUIRE(slice_size > 0 && slice_sets && slice_lengths && c && alpha && beta,                 \
                     GKOC_E_INVALID, "bad argument");                                                     \
        return launch_cx_fmt<T, I>(s, n_rows, sellp_rows{slice_size, slice_sets, slice_lengths}, alpha,   \
                                   col_idxs, vals, b, ldb, beta, c, ldc, nrhs);                           \
    }
GKOC_DEF_CFMT(gkoc_c128, c128, int32_t, i32)
GKOC_DEF_CFMT(gkoc_c128, c128, int64_t, i64)
GKOC_DEF_CFMT(gkoc_c64, c64, int32_t, i32)
GKOC_DEF_CFMT(gkoc_c64, c64, int64_t, i64)
