// Per-row work on the index arrays of a CSR matrix: csr::extract_diagonal, is_sorted_by_column_index and
// sort_by_column_index (decl core/matrix/csr_kernels.hpp; semantics reference/matrix/csr_kernels.cpp).
#include "common.hpp"

namespace gkoc {
namespace {

// ---- diagonal extraction / sortedness / per-row sort ---------------------

// One wave per 64 rows: the rows' contiguous column-index (and value) range is
// staged in LDS with coalesced loads, lane = row then works on its row there.
// Segments longer than the stage fall back to walking global memory per lane.
constexpr int row_stage_cap = 2048;

template <typename I>
struct row_segment {
    int64_t row, rs, re, K0, K1;
    bool valid;
};

template <typename I>
__device__ __forceinline__ row_segment<I> load_row_segment(int64_t n_rows, const I* row_ptrs)
{
    row_segment<I> g;
    const int64_t first = int64_t(blockIdx.x) * 64;
    g.row = first + threadIdx.x;
    g.valid = g.row < n_rows;
    const int64_t last = first + 64 < n_rows ? first + 64 : n_rows;
    g.rs = row_ptrs[g.valid ? g.row : last];
    g.re = row_ptrs[g.valid ? g.row + 1 : last];
    g.K0 = row_ptrs[first];
    g.K1 = row_ptrs[last];
    return g;
}

template <typename T, typename I>
__global__ __launch_bounds__(64) void extract_diag_kernel(int64_t n_diag, const I* __restrict__ row_ptrs,
                                                          const I* __restrict__ cols, const T* __restrict__ vals,
                                                          T* __restrict__ diag)
{
    __shared__ I lc[row_stage_cap];
    const row_segment<I> g = load_row_segment<I>(n_diag, row_ptrs);
    const bool staged = g.K1 - g.K0 <= row_stage_cap;
    if (staged) {
        for (int i = threadIdx.x; i < int(g.K1 - g.K0); i += 64) lc[i] = cols[g.K0 + i];
        wave_lds_sync();
    }
    if (!g.valid) return;
    T d = T(0);
    for (int64_t k = g.rs; k < g.re; ++k) {
        const I c = staged ? lc[k - g.K0] : cols[k];
        if (int64_t(c) == g.row) {
            d = vals[k];
            break;
        }
    }
    diag[g.row] = d;
}

template <typename I>
__global__ __launch_bounds__(64) void is_sorted_kernel(int64_t n_rows, const I* __restrict__ row_ptrs,
                                                       const I* __restrict__ cols, int* __restrict__ flag)
{
    __shared__ I lc[row_stage_cap];
    const row_segment<I> g = load_row_segment<I>(n_rows, row_ptrs);
    const bool staged = g.K1 - g.K0 <= row_stage_cap;
    if (staged) {
        for (int i = threadIdx.x; i < int(g.K1 - g.K0); i += 64) lc[i] = cols[g.K0 + i];
        wave_lds_sync();
    }
    bool ok = true;
    if (g.valid) {
        for (int64_t k = g.rs + 1; k < g.re; ++k) {
            const I a = staged ? lc[k - 1 - g.K0] : cols[k - 1];
            const I b = staged ? lc[k - g.K0] : cols[k];
            if (a > b) {
                ok = false;
                break;
            }
        }
    }
    if (__any(!ok) && threadIdx.x == 0) atomicAnd(flag, 0);
}

// stable insertion sort per row (rows are short on this path; Ginkgo only
// calls it when is_sorted_by_column_index returned false)
template <typename T, typename I>
__global__ __launch_bounds__(64) void sort_rows_kernel(int64_t n_rows, const I* __restrict__ row_ptrs,
                                                       I* __restrict__ cols, T* __restrict__ vals)
{
    __shared__ I lc[row_stage_cap];
    __shared__ T lv[row_stage_cap];
    const row_segment<I> g = load_row_segment<I>(n_rows, row_ptrs);
    const bool staged = g.K1 - g.K0 <= row_stage_cap;
    if (staged) {
        const int seg = int(g.K1 - g.K0);
        for (int i = threadIdx.x; i < seg; i += 64) {
            lc[i] = cols[g.K0 + i];
            lv[i] = vals[g.K0 + i];
        }
        wave_lds_sync();
        if (g.valid) {
            const int a = int(g.rs - g.K0), e = int(g.re - g.K0);
            for (int i = a + 1; i < e; ++i) {
                const I ci = lc[i];
                const T vi = lv[i];
                int k = i - 1;
                while (k >= a && lc[k] > ci) {
                    lc[k + 1] = lc[k];
                    lv[k + 1] = lv[k];
                    --k;
                }
                lc[k + 1] = ci;
                lv[k + 1] = vi;
            }
        }
        wave_lds_sync();
        for (int i = threadIdx.x; i < seg; i += 64) {
            cols[g.K0 + i] = lc[i];
            vals[g.K0 + i] = lv[i];
        }
        return;
    }
    if (!g.valid) return;
    for (int64_t i = g.rs + 1; i < g.re; ++i) {
        const I ci = cols[i];
        const T vi = vals[i];
        int64_t k = i - 1;
        while (k >= g.rs && cols[k] > ci) {
            cols[k + 1] = cols[k];
            vals[k + 1] = vals[k];
            --k;
        }
        cols[k + 1] = ci;
        vals[k + 1] = vi;
    }
}

}  // namespace
}  // namespace gkoc

using namespace gkoc;

// csr::sort_by_column_index: defined once, for the real types by GKOC_DEF_CSR_ROWS below, for complex values (pairs;
// the kernel only moves them) here
#define GKOC_DEF_CSR_SORT_ROWS(T, TN, I, IN)                                                                         \
    extern "C" int gkoc_csr_sort_by_column_index_##TN##_##IN(gkoc_stream_t s, int64_t n_rows, const I* row_ptrs,     \
                                                             I* col_idxs, T* vals)                                   \
    {                                                                                                                \
        if (n_rows <= 0) return GKOC_OK;                                                                             \
        gkoc::csr_structure_written(col_idxs);                                                                       \
        sort_rows_kernel<T, I><<<dim3(unsigned(ceildiv(n_rows, 64))), dim3(64), 0, as_stream(s)>>>(n_rows, row_ptrs, \
                                                                                                   col_idxs, vals);  \
        GKOC_LAUNCH_OK();                                                                                            \
        return GKOC_OK;                                                                                              \
    }
GKOC_DEF_CSR_SORT_ROWS(gkoc_c128, c128, int32_t, i32)
GKOC_DEF_CSR_SORT_ROWS(gkoc_c128, c128, int64_t, i64)
GKOC_DEF_CSR_SORT_ROWS(gkoc_c64, c64, int32_t, i32)
GKOC_DEF_CSR_SORT_ROWS(gkoc_c64, c64, int64_t, i64)

#define GKOC_DEF_CSR_ROWS(T, TN, I, IN)                                                                              \
    extern "C" int gkoc_csr_extract_diagonal_##TN##_##IN(gkoc_stream_t s, int64_t n_rows, int64_t n_cols,            \
                                                         const I* row_ptrs, const I* col_idxs, const T* vals,        \
                                                         T* diag)                                                    \
    {                                                                                                                \
        const int64_t nd = n_rows < n_cols ? n_rows : n_cols;                                                        \
        if (nd <= 0) return GKOC_OK;                                                                                 \
        extract_diag_kernel<T, I><<<dim3(unsigned(ceildiv(nd, 64))), dim3(64), 0, as_stream(s)>>>(                   \
            nd, row_ptrs, col_idxs, vals, diag);                                                                     \
        GKOC_LAUNCH_OK();                                                                                            \
        return GKOC_OK;                                                                                              \
    }                                                                                                                \
    extern "C" int gkoc_csr_is_sorted_by_column_index_##TN##_##IN(gkoc_stream_t s, int64_t n_rows, const I* row_ptrs, \
                                                                  const I* col_idxs, int* is_sorted_host)            \
    {                                                                                                                \
        GKOC_REQUIRE(is_sorted_host, GKOC_E_INVALID, "null result");                                                 \
        *is_sorted_host = 1;                                                                                         \
        if (n_rows <= 0) return GKOC_OK;                                                                             \
        int* flag = nullptr;                                                                                         \
        GKOC_TRY(scratch_malloc(as_stream(s), reinterpret_cast<void**>(&flag), sizeof(int)));                        \
        /* any non-zero pattern = sorted; set on the device (an asynchronous copy from pageable host memory is */    \
        /* not ordered with the kernel) */                                                                           \
        GKOC_HIP(hipMemsetAsync(flag, 1, sizeof(int), as_stream(s)));                                                \
        is_sorted_kernel<I><<<dim3(unsigned(ceildiv(n_rows, 64))), dim3(64), 0, as_stream(s)>>>(n_rows, row_ptrs,    \
                                                                                                col_idxs, flag);     \
        GKOC_LAUNCH_OK();                                                                                            \
        GKOC_HIP(hipMemcpyAsync(is_sorted_host, flag, sizeof(int), hipMemcpyDeviceToHost, as_stream(s)));            \
        GKOC_HIP(hipStreamSynchronize(as_stream(s)));                                                                \
        GKOC_TRY(scratch_free(as_stream(s), flag));                                                                  \
        *is_sorted_host = *is_sorted_host != 0;                                                                      \
        return GKOC_OK;                                                                                              \
    }                                                                                                                \
    GKOC_DEF_CSR_SORT_ROWS(T, TN, I, IN)
GKOC_DEF_CSR_ROWS(double, f64, int32_t, i32)
GKOC_DEF_CSR_ROWS(double, f64, int64_t, i64)
GKOC_DEF_CSR_ROWS(float, f32, int32_t, i32)
GKOC_DEF_CSR_ROWS(float, f32, int64_t, i64)
