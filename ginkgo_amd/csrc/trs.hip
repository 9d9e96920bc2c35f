// Sparse triangular solves on a level schedule, and the set-up kernels of the Sor / SSOR preconditioner:
//   lower_trs / upper_trs ::{generate, solve}   core/solver/{lower,upper}_trs_kernels.hpp,
//                                               reference/solver/{lower,upper}_trs_kernels.cpp
//   factorization::initialize_row_ptrs_l_u      reference/factorization/factorization_kernels.cpp
//   sor::initialize_weighted_l{,_u}             reference/preconditioner/sor_kernels.cpp
//
// Contract of a solve (the reference's loop; it fixes the rounding): for every right-hand side j and
// row = 0 .. n-1 (upper: n-1 .. 0), t = b(row, j); for k ascending over the row's entries in STORAGE
// order: col < row (upper: col > row) gives t = t - vals[k] * x(col, j) as a separate multiply and
// subtract, col == row remembers diag = vals[k]; x(row, j) = unit_diag ? t : t / diag.  Columns need
// not be sorted, entries on the other side of the diagonal are ignored (by the analysis as well), a
// missing diagonal counts as 1.  One lane accumulates one (row, rhs) sequentially, so f64 and f32
// results are bit-identical to that loop.
//
// generate: level[row] = 1 + max(level[col]) over the row's dependencies (0 without any); rows grouped
// by level, ascending inside a level, in level_ptrs / level_rows on the device.  The levels are
// computed on the HOST (one D2H copy of the structure, one sequential pass, a counting sort, one H2D
// copy): set-up, not the hot path (DESIGN.md 8 keeps the device version open).
//
// solve: a host-side schedule of two kinds of segments.
//   wide   = one level with more than trs_wide_threshold rows: one launch over many workgroups, one
//            lane per (row, rhs); no dependencies exist inside a level.
//   narrow = a maximal run of consecutive levels with <= trs_wide_threshold rows each: one launch of
//            ONE workgroup that walks the levels with __syncthreads() between them.
// No kernel ever waits for a store of another workgroup: a dependency across workgroups is always a
// kernel boundary on the stream.  Inside the narrow kernel x is handed over through global memory
// between waves of one workgroup, i.e. of one CU: they share that CU's L1, the stores are write-through
// and __syncthreads() is a workgroup-scope release/acquire around the barrier, which is all that is
// needed there (and nothing more would help across CUs without a kernel boundary).
// solve only enqueues launches: no allocation, no synchronisation, no copy - it can be captured.
#include <hip/hip_runtime.h>

#include <vector>

#include "common.hpp"
#include "scan.hpp"
#include "trs_struct.hpp"

namespace gkoc {
namespace {

constexpr int trs_wide_threshold = 1024;   // W: rows one workgroup takes per level
constexpr int trs_narrow_block = 1024;
constexpr int trs_wide_block = 256;

template <bool UPPER, typename T, typename I>
__device__ __forceinline__ void trs_row(int64_t row, int64_t j, bool unit_diag,
                                        const I* __restrict__ row_ptrs, const I* __restrict__ col_idxs,
                                        const T* __restrict__ vals, const T* b, int64_t ldb, T* x,
                                        int64_t ldx)
{
    T t = b[row * ldb + j];
    T diag = T(1);
    const int64_t end = row_ptrs[row + 1];
    for (int64_t k = row_ptrs[row]; k < end; ++k) {
        const int64_t col = col_idxs[k];
        if (UPPER ? col > row : col < row) {
            t = t - vals[k] * x[col * ldx + j];
        } else if (col == row) {
            diag = vals[k];
        }
    }
    x[row * ldx + j] = unit_diag ? t : t / diag;
}

// one level, rows spread over the grid
template <bool UPPER, typename T, typename I>
__global__ __launch_bounds__(trs_wide_block) void trs_wide_kernel(
    int64_t rows, int64_t nrhs, int unit_diag, const int64_t* __restrict__ level_rows /* of this level */,
    const I* __restrict__ row_ptrs, const I* __restrict__ col_idxs, const T* __restrict__ vals, const T* b,
    int64_t ldb, T* x, int64_t ldx)
{
    const int64_t items = rows * nrhs;
    const int64_t stride = int64_t(gridDim.x) * trs_wide_block;
    for (int64_t t = int64_t(blockIdx.x) * trs_wide_block + threadIdx.x; t < items; t += stride) {
        const int64_t r = nrhs == 1 ? t : t / nrhs;
        const int64_t j = nrhs == 1 ? 0 : t - r * nrhs;
        trs_row<UPPER, T, I>(level_rows[r], j, unit_diag != 0, row_ptrs, col_idxs, vals, b, ldb, x, ldx);
    }
}

// levels [l0, l1) in ONE workgroup; launched with a grid of 1
template <bool UPPER, typename T, typename I>
__global__ __launch_bounds__(trs_narrow_block) void trs_narrow_kernel(
    int64_t l0, int64_t l1, int64_t nrhs, int unit_diag, const int64_t* __restrict__ level_ptrs,
    const int64_t* __restrict__ level_rows, const I* __restrict__ row_ptrs, const I* __restrict__ col_idxs,
    const T* __restrict__ vals, const T* b, int64_t ldb, T* x, int64_t ldx)
{
    int64_t first = level_ptrs[l0];
    for (int64_t l = l0; l < l1; ++l) {
        const int64_t next = level_ptrs[l + 1];
        const int64_t items = (next - first) * nrhs;
        for (int64_t t = threadIdx.x; t < items; t += trs_narrow_block) {
            const int64_t r = nrhs == 1 ? t : t / nrhs;
            const int64_t j = nrhs == 1 ? 0 : t - r * nrhs;
            trs_row<UPPER, T, I>(level_rows[first + r], j, unit_diag != 0, row_ptrs, col_idxs, vals, b, ldb,
                                 x, ldx);
        }
        first = next;
        // this level's x for the next level's lanes of this workgroup (uniform: l0, l1 are arguments)
        __syncthreads();
    }
}

template <typename I>
int trs_generate(gkoc_stream_t s, bool upper, int64_t n, const I* row_ptrs, const I* col_idxs,
                 gkoc_trs_struct_t* out)
{
    GKOC_REQUIRE(out, GKOC_E_INVALID, "null pointer for the result");
    *out = nullptr;
    GKOC_REQUIRE(n >= 0, GKOC_E_INVALID, "negative number of rows");
    GKOC_REQUIRE(n == 0 || row_ptrs, GKOC_E_INVALID, "null row pointers");
    hipStream_t st = as_stream(s);
    std::vector<I> rp(size_t(n) + 1, I(0)), ci;
    if (n > 0) {
        GKOC_HIP(hipMemcpyAsync(rp.data(), row_ptrs, sizeof(I) * size_t(n + 1), hipMemcpyDeviceToHost, st));
        GKOC_HIP(hipStreamSynchronize(st));
    }
    for (int64_t r = 0; r < n; ++r) {
        GKOC_REQUIRE(rp[r] >= 0 && rp[r] <= rp[r + 1], GKOC_E_INVALID, "row pointers do not ascend");
    }
    const int64_t nnz = int64_t(rp[n]);
    GKOC_REQUIRE(nnz == 0 || col_idxs, GKOC_E_INVALID, "null column indices");
    if (nnz > 0) {
        ci.resize(size_t(nnz));
        GKOC_HIP(hipMemcpyAsync(ci.data(), col_idxs, sizeof(I) * size_t(nnz), hipMemcpyDeviceToHost, st));
        GKOC_HIP(hipStreamSynchronize(st));
    }
    // levels: one sequential pass in the order of the solve
    std::vector<int64_t> level(size_t(n), 0);
    int64_t n_levels = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t row = upper ? n - 1 - i : i;
        int64_t lv = 0;
        for (int64_t k = rp[row]; k < rp[row + 1]; ++k) {
            const int64_t col = ci[k];
            GKOC_REQUIRE(col >= 0 && col < n, GKOC_E_INVALID, "column index outside the matrix");
            if (upper ? col > row : col < row) {
                lv = level[col] + 1 > lv ? level[col] + 1 : lv;
            }
        }
        level[row] = lv;
        n_levels = lv + 1 > n_levels ? lv + 1 : n_levels;
    }
    // counting sort, ascending row index inside a level
    std::vector<int64_t> level_ptrs(size_t(n_levels) + 1, 0), level_rows(size_t(n), 0);
    for (int64_t r = 0; r < n; ++r) ++level_ptrs[level[r] + 1];
    for (int64_t l = 0; l < n_levels; ++l) level_ptrs[l + 1] += level_ptrs[l];
    {
        std::vector<int64_t> pos(level_ptrs.begin(), level_ptrs.end() - 1);
        for (int64_t r = 0; r < n; ++r) level_rows[pos[level[r]]++] = r;
    }
    auto* t = new gkoc_trs_struct_s{};
    t->n_rows = n;
    t->nnz = nnz;
    t->is_upper = upper ? 1 : 0;
    t->n_levels = n_levels;
    // launch schedule
    for (int64_t l = 0; l < n_levels; ++l) {
        const int64_t rows = level_ptrs[l + 1] - level_ptrs[l];
        if (rows > trs_wide_threshold) {
            t->schedule.push_back({l, l + 1, level_ptrs[l], rows, true});
        } else if (!t->schedule.empty() && !t->schedule.back().wide && t->schedule.back().last == l) {
            auto& seg = t->schedule.back();
            seg.last = l + 1;
            seg.rows = rows > seg.rows ? rows : seg.rows;
        } else {
            t->schedule.push_back({l, l + 1, level_ptrs[l], rows, false});
        }
    }
    int rc = arena_malloc(reinterpret_cast<void**>(&t->level_ptrs), sizeof(int64_t) * size_t(n_levels + 1),
                          GKOC_MEM_INDICES);
    if (rc == GKOC_OK && n > 0) {
        rc = arena_malloc(reinterpret_cast<void**>(&t->level_rows), sizeof(int64_t) * size_t(n),
                          GKOC_MEM_INDICES);
    }
    hipError_t e = hipSuccess;
    if (rc == GKOC_OK) {
        e = hipMemcpyAsync(t->level_ptrs, level_ptrs.data(), sizeof(int64_t) * size_t(n_levels + 1),
                           hipMemcpyHostToDevice, st);
    }
    if (rc == GKOC_OK && e == hipSuccess && n > 0) {
        e = hipMemcpyAsync(t->level_rows, level_rows.data(), sizeof(int64_t) * size_t(n), hipMemcpyHostToDevice,
                           st);
    }
    // the host vectors go away on return
    if (rc == GKOC_OK && e == hipSuccess) e = hipStreamSynchronize(st);
    if (rc != GKOC_OK || e != hipSuccess) {
        if (t->level_ptrs) (void)arena_free(t->level_ptrs);
        if (t->level_rows) (void)arena_free(t->level_rows);
        delete t;
        if (rc != GKOC_OK) return rc;
        GKOC_HIP(e);
    }
    *out = t;
    return GKOC_OK;
}

template <bool UPPER, typename T, typename I>
int trs_solve(gkoc_stream_t s, gkoc_trs_struct_t t, int unit_diag, int64_t n, int64_t nrhs, const I* row_ptrs,
              const I* col_idxs, const T* vals, const T* b, int64_t ldb, T* x, int64_t ldx)
{
    GKOC_REQUIRE(t, GKOC_E_INVALID, "null triangular-solve structure");
    GKOC_REQUIRE(n >= 0 && nrhs >= 0, GKOC_E_INVALID, "negative dimension");
    GKOC_REQUIRE(t->is_upper == (UPPER ? 1 : 0), GKOC_E_INVALID,
                 "the structure was generated for the other triangle");
    GKOC_REQUIRE(t->n_rows == n, GKOC_E_INVALID, "the structure was generated for another number of rows");
    GKOC_REQUIRE(ldb >= nrhs && ldx >= nrhs, GKOC_E_INVALID, "stride smaller than the number of right-hand sides");
    if (n == 0 || nrhs == 0) return GKOC_OK;
    GKOC_REQUIRE(row_ptrs && b && x, GKOC_E_INVALID, "null pointer");
    GKOC_REQUIRE(t->nnz == 0 || (col_idxs && vals), GKOC_E_INVALID, "null pointer");
    hipStream_t st = as_stream(s);
    for (const auto& seg : t->schedule) {
        if (seg.rows == 0) continue;
        if (seg.wide) {
            trs_wide_kernel<UPPER, T, I>
                <<<dim3(stream_grid(seg.rows * nrhs, trs_wide_block)), dim3(trs_wide_block), 0, st>>>(
                seg.rows, nrhs, unit_diag, t->level_rows + seg.offset, row_ptrs, col_idxs, vals, b, ldb, x, ldx);
        } else {
            trs_narrow_kernel<UPPER, T, I><<<dim3(1), dim3(trs_narrow_block), 0, st>>>(
                seg.first, seg.last, nrhs, unit_diag, t->level_ptrs, t->level_rows, row_ptrs, col_idxs, vals, b,
                ldb, x, ldx);
        }
        GKOC_LAUNCH_OK();
    }
    return GKOC_OK;
}


// ------------------------------------------------------------------ Sor set-up (one thread per row)
// counts of strictly-lower + 1 and strictly-upper + 1 entries per row; entry n_rows = 0 for the scan
template <typename I>
__global__ __launch_bounds__(256) void count_l_u_kernel(int64_t n, const I* __restrict__ rp,
                                                        const I* __restrict__ ci, I* __restrict__ l_rp,
                                                        I* __restrict__ u_rp)
{
    const int64_t stride = int64_t(gridDim.x) * 256;
    for (int64_t row = int64_t(blockIdx.x) * 256 + threadIdx.x; row <= n; row += stride) {
        I l = 0, u = 0;
        if (row < n) {
            l = u = 1;
            for (int64_t k = rp[row]; k < rp[row + 1]; ++k) {
                const int64_t col = ci[k];
                l += col < row ? I(1) : I(0);
                u += col > row ? I(1) : I(0);
            }
        }
        l_rp[row] = l;
        if (u_rp) u_rp[row] = u;
    }
}

// L = strictly-lower entries of A in storage order, then a_ii / w; with WITH_U also
// U = 1 / (2 - w), then (w * a_ij) / ((2 - w) * a_ii) for the strictly-upper entries in storage order
template <bool WITH_U, typename T, typename I>
__global__ __launch_bounds__(256) void weighted_l_u_kernel(int64_t n, const I* __restrict__ rp,
                                                           const I* __restrict__ ci, const T* __restrict__ v,
                                                           T w, const I* __restrict__ l_rp, I* __restrict__ l_ci,
                                                           T* __restrict__ l_v, const I* __restrict__ u_rp,
                                                           I* __restrict__ u_ci, T* __restrict__ u_v)
{
    const int64_t stride = int64_t(gridDim.x) * 256;
    for (int64_t row = int64_t(blockIdx.x) * 256 + threadIdx.x; row < n; row += stride) {
        const int64_t begin = rp[row], end = rp[row + 1];
        T diag = T(1);   // a missing a_ii counts as 1
        int64_t lp = l_rp[row];
        for (int64_t k = begin; k < end; ++k) {
            const int64_t col = ci[k];
            if (col < row) {
                l_ci[lp] = I(col);
                l_v[lp] = v[k];
                ++lp;
            } else if (col == row) {
                diag = v[k];
            }
        }
        l_ci[lp] = I(row);
        l_v[lp] = diag / w;
        if (WITH_U) {
            const T two_minus_w = T(2) - w;
            const T scale = two_minus_w * diag;
            int64_t up = u_rp[row];
            u_ci[up] = I(row);
            u_v[up] = T(1) / two_minus_w;
            ++up;
            for (int64_t k = begin; k < end; ++k) {
                const int64_t col = ci[k];
                if (col > row) {
                    u_ci[up] = I(col);
                    u_v[up] = (w * v[k]) / scale;
                    ++up;
                }
            }
        }
    }
}

template <typename I>
int row_ptrs_l_u(gkoc_stream_t s, int64_t n, const I* rp, const I* ci, I* l_rp, I* u_rp)
{
    GKOC_REQUIRE(n >= 0, GKOC_E_INVALID, "negative number of rows");
    GKOC_REQUIRE(l_rp && (n == 0 || rp), GKOC_E_INVALID, "null pointer");
    hipStream_t st = as_stream(s);
    count_l_u_kernel<I><<<dim3(stream_grid(n + 1)), dim3(256), 0, st>>>(n, rp, ci, l_rp, u_rp);
    GKOC_LAUNCH_OK();
    GKOC_TRY(device_exclusive_scan<I>(st, l_rp, n + 1));
    if (u_rp) GKOC_TRY(device_exclusive_scan<I>(st, u_rp, n + 1));
    return GKOC_OK;
}

template <bool WITH_U, typename T, typename I>
int weighted_l_u(gkoc_stream_t s, int64_t n, const I* rp, const I* ci, const T* v, double weight, const I* l_rp,
                 I* l_ci, T* l_v, const I* u_rp, I* u_ci, T* u_v)
{
    GKOC_REQUIRE(n >= 0, GKOC_E_INVALID, "negative number of rows");
    GKOC_REQUIRE(weight > 0.0 && weight < 2.0, GKOC_E_INVALID, "relaxation factor outside (0, 2)");
    if (n == 0) return GKOC_OK;
    GKOC_REQUIRE(rp && l_rp && l_ci && l_v, GKOC_E_INVALID, "null pointer");
    GKOC_REQUIRE(!WITH_U || (u_rp && u_ci && u_v), GKOC_E_INVALID, "null pointer");
    weighted_l_u_kernel<WITH_U, T, I><<<dim3(stream_grid(n)), dim3(256), 0, as_stream(s)>>>(
        n, rp, ci, v, T(weight), l_rp, l_ci, l_v, u_rp, u_ci, u_v);
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

}  // namespace
}  // namespace gkoc

using namespace gkoc;

extern "C" int gkoc_trs_struct_destroy(gkoc_trs_struct_t t)
{
    if (!t) return GKOC_OK;
    int rc = GKOC_OK;
    if (t->level_ptrs) rc = arena_free(t->level_ptrs);
    if (t->level_rows) {
        const int rc2 = arena_free(t->level_rows);
        rc = rc == GKOC_OK ? rc2 : rc;
    }
    delete t;
    return rc;
}

extern "C" int gkoc_trs_struct_info(gkoc_trs_struct_t t, int64_t* n_rows, int* is_upper, int64_t* n_levels,
                                    int64_t* n_launches, int64_t* wide_threshold)
{
    GKOC_REQUIRE(t, GKOC_E_INVALID, "null triangular-solve structure");
    if (n_rows) *n_rows = t->n_rows;
    if (is_upper) *is_upper = t->is_upper;
    if (n_levels) *n_levels = t->n_levels;
    if (n_launches) *n_launches = int64_t(t->schedule.size());
    if (wide_threshold) *wide_threshold = trs_wide_threshold;
    return GKOC_OK;
}

extern "C" int gkoc_trs_struct_levels(gkoc_trs_struct_t t, int64_t* level_ptrs_host, int64_t* level_rows_host)
{
    GKOC_REQUIRE(t, GKOC_E_INVALID, "null triangular-solve structure");
    GKOC_REQUIRE(level_ptrs_host && (t->n_rows == 0 || level_rows_host), GKOC_E_INVALID, "null pointer");
    GKOC_HIP(hipMemcpy(level_ptrs_host, t->level_ptrs, sizeof(int64_t) * size_t(t->n_levels + 1),
                       hipMemcpyDeviceToHost));
    if (t->n_rows > 0) {
        GKOC_HIP(hipMemcpy(level_rows_host, t->level_rows, sizeof(int64_t) * size_t(t->n_rows),
                           hipMemcpyDeviceToHost));
    }
    return GKOC_OK;
}

#define GKOC_DEF_TRS_I(I, IN)                                                                                  \
    extern "C" int gkoc_lower_trs_generate_##IN(gkoc_stream_t s, int64_t n_rows, const I* row_ptrs,            \
                                                const I* col_idxs, gkoc_trs_struct_t* out)                     \
    {                                                                                                          \
        return trs_generate<I>(s, false, n_rows, row_ptrs, col_idxs, out);                                     \
    }                                                                                                          \
    extern "C" int gkoc_upper_trs_generate_##IN(gkoc_stream_t s, int64_t n_rows, const I* row_ptrs,            \
                                                const I* col_idxs, gkoc_trs_struct_t* out)                     \
    {                                                                                                          \
        return trs_generate<I>(s, true, n_rows, row_ptrs, col_idxs, out);                                      \
    }                                                                                                          \
    extern "C" int gkoc_factorization_initialize_row_ptrs_l_u_##IN(gkoc_stream_t s, int64_t n_rows,            \
                                                                   const I* row_ptrs, const I* col_idxs,       \
                                                                   I* l_row_ptrs, I* u_row_ptrs)               \
    {                                                                                                          \
        gkoc::csr_structure_written(l_row_ptrs); gkoc::csr_structure_written(u_row_ptrs);                      \
        return row_ptrs_l_u<I>(s, n_rows, row_ptrs, col_idxs, l_row_ptrs, u_row_ptrs);                         \
    }
GKOC_DEF_TRS_I(int32_t, i32)
GKOC_DEF_TRS_I(int64_t, i64)

#define GKOC_DEF_TRS(T, TN, I, IN)                                                                             \
    extern "C" int gkoc_lower_trs_solve_##TN##_##IN(                                                           \
        gkoc_stream_t s, gkoc_trs_struct_t t, int unit_diag, int64_t n_rows, int64_t nrhs, const I* row_ptrs,  \
        const I* col_idxs, const T* vals, const T* b, int64_t ldb, T* x, int64_t ldx)                          \
    {                                                                                                          \
        return trs_solve<false, T, I>(s, t, unit_diag, n_rows, nrhs, row_ptrs, col_idxs, vals, b, ldb, x,      \
                                      ldx);                                                                    \
    }                                                                                                          \
    extern "C" int gkoc_upper_trs_solve_##TN##_##IN(                                                           \
        gkoc_stream_t s, gkoc_trs_struct_t t, int unit_diag, int64_t n_rows, int64_t nrhs, const I* row_ptrs,  \
        const I* col_idxs, const T* vals, const T* b, int64_t ldb, T* x, int64_t ldx)                          \
    {                                                                                                          \
        return trs_solve<true, T, I>(s, t, unit_diag, n_rows, nrhs, row_ptrs, col_idxs, vals, b, ldb, x,       \
                                     ldx);                                                                     \
    }                                                                                                          \
    extern "C" int gkoc_sor_initialize_weighted_l_##TN##_##IN(                                                 \
        gkoc_stream_t s, int64_t n_rows, const I* rp, const I* ci, const T* v, double weight, const I* l_rp,   \
        I* l_ci, T* l_v)                                                                                       \
    {                                                                                                          \
        gkoc::csr_structure_written(l_ci);                                                                     \
        return weighted_l_u<false, T, I>(s, n_rows, rp, ci, v, weight, l_rp, l_ci, l_v, nullptr, nullptr,      \
                                         nullptr);                                                             \
    }                                                                                                          \
    extern "C" int gkoc_sor_initialize_weighted_l_u_##TN##_##IN(                                               \
        gkoc_stream_t s, int64_t n_rows, const I* rp, const I* ci, const T* v, double weight, const I* l_rp,   \
        I* l_ci, T* l_v, const I* u_rp, I* u_ci, T* u_v)                                                       \
    {                                                                                                          \
        gkoc::csr_structure_written(l_ci); gkoc::csr_structure_written(u_ci);                                  \
        return weighted_l_u<true, T, I>(s, n_rows, rp, ci, v, weight, l_rp, l_ci, l_v, u_rp, u_ci, u_v);       \
    }
GKOC_DEF_TRS(double, f64, int32_t, i32)
GKOC_DEF_TRS(double, f64, int64_t, i64)
GKOC_DEF_TRS(float, f32, int32_t, i32)
GKOC_DEF_TRS(float, f32, int64_t, i64)
