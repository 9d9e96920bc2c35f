// Fbcsr (fixed-block CSR): block SpMV, CSR <-> Fbcsr conversions, fill_in_dense,
// extract_diagonal and is_sorted_by_column_index.
//
// Replaces gko::kernels::hip::fbcsr::{spmv, advanced_spmv, convert_to_csr, fill_in_dense,
// extract_diagonal, is_sorted_by_column_index} and csr::convert_to_fbcsr
// (decl core/matrix/fbcsr_kernels.hpp, core/matrix/csr_kernels.hpp).
//
// Storage is Ginkgo's matrix::Fbcsr (include/ginkgo/core/matrix/fbcsr.hpp): row_ptrs has
// n_block_rows + 1 entries and counts BLOCKS, col_idxs holds one block column per block,
// values holds the blocks in storage order, each bs x bs block column-major - entry (i, j)
// of block k at k bs^2 + j bs + i (acc::block_col_major<V, 3> of core/matrix/fbcsr.cpp and
// reference/matrix/fbcsr_kernels.cpp).  The layout follows that documented accessor; it was
// not re-read from a Ginkgo source tree when this file was written.
//
// SpMV semantics (bit-identical to the CSR reference loop on the expanded matrix): scalar
// row r = brow bs + i sums val(k, i, j) * b[col_idxs[k] bs + j] over the blocks k of its
// block row in storage order and over j ascending inside each block, multiply and add
// rounded separately (-ffp-contract=off).  Advanced: sum = (beta == 0 ? 0 : c beta), then
// sum += (alpha val) b in the same order; beta == 0 never reads c.  No chunking: every row
// is summed by one lane, whatever its length.
//
// Kernels (docs/KERNELS.md section 34), one per block size:
//  - bs <= 3, fbcsr_spmv_entry_kernel: lane = (block row, entry of the block), bs^2 lanes per
//    block row read a block with ONE load instruction; products added in order through wave
//    shuffles by the lane of (i, 0).
//  - bs >= 4, fbcsr_spmv_kernel: lane = (block row, row inside the block), 64 / bs block rows
//    per wave; the bs lanes of a block row read a block with bs loads of bs contiguous values.
// col_idxs[k] and the b entries are the same addresses for a block row's lanes.  U blocks are
// loaded before they are added (loads in flight, order kept).
// Algorithmic HBM bytes: 8 nnz + 4 nbnz + 4 (nbrows + 1) + 16 n (f64 / i32).
#include "common.hpp"
#include "scan.hpp"

namespace gkoc {
namespace {

constexpr int fbcsr_max_bs = 8;
constexpr int fbcsr_block = 256;    // 4 waves per workgroup

template <int BS>
constexpr int fbcsr_unroll()
{
    return BS <= 2 ? 8 : (BS <= 4 ? 4 : 2);
}

template <int BS, typename T, typename I, bool ADV>
__global__ __launch_bounds__(fbcsr_block) void fbcsr_spmv_kernel(
    int64_t n_brows, const I* __restrict__ row_ptrs, const I* __restrict__ cols,
    const T* __restrict__ vals, const T* __restrict__ b, int64_t ldb, T* __restrict__ c,
    int64_t ldc, int64_t nrhs, const T* __restrict__ alpha_p, const T* __restrict__ beta_p)
{
    constexpr int G = wave_size / BS;          // block rows per wave
    constexpr int U = fbcsr_unroll<BS>();
    constexpr int64_t BS2 = int64_t(BS) * BS;
    const int lane = threadIdx.x & (wave_size - 1);
    const int grp = lane / BS;
    const int i = lane - grp * BS;
    if (grp >= G) return;                      // the 64 % bs lanes left over
    const int64_t brow = (int64_t(blockIdx.x) * (fbcsr_block / wave_size) +
                          (threadIdx.x / wave_size)) * G + grp;
    if (brow >= n_brows) return;
    T alpha = T(1), beta = T(0);
    if (ADV) {
        alpha = alpha_p[0];
        beta = beta_p[0];
    }
    const int64_t k0 = row_ptrs[brow], k1 = row_ptrs[brow + 1];
    const int64_t row = brow * BS + i;
    for (int64_t col = 0; col < nrhs; ++col) {
        T sum = T(0);
        if (ADV && beta != T(0)) sum = c[row * ldc + col] * beta;
        int64_t k = k0;
        for (; k + U <= k1; k += U) {
            I bc[U];
            T v[U][BS], x[U][BS];
#pragma unroll
            for (int u = 0; u < U; ++u) bc[u] = cols[k + u];
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int j = 0; j < BS; ++j) v[u][j] = vals[(k + u) * BS2 + j * BS + i];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int j = 0; j < BS; ++j) x[u][j] = b[(int64_t(bc[u]) * BS + j) * ldb + col];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int j = 0; j < BS; ++j) sum += ADV ? (alpha * v[u][j]) * x[u][j] : v[u][j] * x[u][j];
            }
        }
        for (; k < k1; ++k) {
            const int64_t bc = cols[k];
            T v[BS], x[BS];
#pragma unroll
            for (int j = 0; j < BS; ++j) v[j] = vals[k * BS2 + j * BS + i];
#pragma unroll
            for (int j = 0; j < BS; ++j) x[j] = b[(bc * BS + j) * ldb + col];
#pragma unroll
            for (int j = 0; j < BS; ++j) sum += ADV ? (alpha * v[j]) * x[j] : v[j] * x[j];
        }
        c[row * ldc + col] = sum;
    }
}

// lane = (block row, entry e = j bs + i of the block): bs^2 lanes per block row, so ONE load
// instruction reads a whole block as one contiguous run of bs^2 values.  Lane e forms the
// product val(k, i, j) * b[col bs + j]; the lane of (i, j = 0) adds the products of row i in
// j order, fetched from its group by wave shuffles - the same operations in the same order
// as one lane per row.
template <int BS, typename T, typename I, bool ADV>
__global__ __launch_bounds__(fbcsr_block) void fbcsr_spmv_entry_kernel(
    int64_t n_brows, const I* __restrict__ row_ptrs, const I* __restrict__ cols,
    const T* __restrict__ vals, const T* __restrict__ b, int64_t ldb, T* __restrict__ c,
    int64_t ldc, int64_t nrhs, const T* __restrict__ alpha_p, const T* __restrict__ beta_p)
{
    constexpr int BS2 = BS * BS;
    constexpr int G = wave_size / BS2;         // block rows per wave (>= 1 for bs <= 8)
    constexpr int U = 8;
    const int lane = threadIdx.x & (wave_size - 1);
    const int grp = lane / BS2;
    const int e = lane - grp * BS2;
    const int j = e / BS, i = e - j * BS;
    if (grp >= G) return;                      // the 64 % bs^2 lanes left over
    const int64_t brow = (int64_t(blockIdx.x) * (fbcsr_block / wave_size) +
                          (threadIdx.x / wave_size)) * G + grp;
    if (brow >= n_brows) return;               // whole groups leave: shuffles stay inside one
    T alpha = T(1), beta = T(0);
    if (ADV) {
        alpha = alpha_p[0];
        beta = beta_p[0];
    }
    const int64_t k0 = row_ptrs[brow], k1 = row_ptrs[brow + 1];
    const int64_t row = brow * BS + i;
    const int src = grp * BS2 + i;             // lane of (i, 0); (i, jj) is src + jj bs
    for (int64_t col = 0; col < nrhs; ++col) {
        T sum = T(0);
        if (ADV && j == 0 && beta != T(0)) sum = c[row * ldc + col] * beta;
        int64_t k = k0;
        for (; k + U <= k1; k += U) {
            I bc[U];
            T p[U];
#pragma unroll
            for (int u = 0; u < U; ++u) bc[u] = cols[k + u];
#pragma unroll
            for (int u = 0; u < U; ++u) p[u] = vals[(k + u) * BS2 + e];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const T x = b[(int64_t(bc[u]) * BS + j) * ldb + col];
                p[u] = ADV ? (alpha * p[u]) * x : p[u] * x;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                sum += p[u];
#pragma unroll
                for (int jj = 1; jj < BS; ++jj) sum += __shfl(p[u], src + jj * BS, wave_size);
            }
        }
        for (; k < k1; ++k) {
            const T x = b[(int64_t(cols[k]) * BS + j) * ldb + col];
            const T v = vals[k * BS2 + e];
            const T p = ADV ? (alpha * v) * x : v * x;
            sum += p;
#pragma unroll
            for (int jj = 1; jj < BS; ++jj) sum += __shfl(p, src + jj * BS, wave_size);
        }
        if (j == 0) c[row * ldc + col] = sum;
    }
}

template <int BS, typename T, typename I, bool ADV>
int fbcsr_spmv_launch(hipStream_t st, int64_t n_brows, const I* row_ptrs, const I* cols,
                      const T* vals, const T* b, int64_t ldb, T* c, int64_t ldc, int64_t nrhs,
                      const T* alpha, const T* beta)
{
    // entry lanes up to bs = 3, row lanes from bs = 4 on (measured: docs/KERNELS.md section 34)
    constexpr bool entry = BS <= 3;
    const int64_t g = entry ? wave_size / (BS * BS) : wave_size / BS;
    const int64_t rows_per_block = g * (fbcsr_block / wave_size);
    const int64_t blocks = ceildiv(n_brows, rows_per_block);
    GKOC_REQUIRE(blocks <= int64_t(0x7fffffff), GKOC_E_INVALID, "Fbcsr: too many block rows");
    if constexpr (entry) {
        fbcsr_spmv_entry_kernel<BS, T, I, ADV><<<dim3(unsigned(blocks)), dim3(fbcsr_block), 0, st>>>(
            n_brows, row_ptrs, cols, vals, b, ldb, c, ldc, nrhs, alpha, beta);
    } else {
        fbcsr_spmv_kernel<BS, T, I, ADV><<<dim3(unsigned(blocks)), dim3(fbcsr_block), 0, st>>>(
            n_brows, row_ptrs, cols, vals, b, ldb, c, ldc, nrhs, alpha, beta);
    }
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

template <typename T, typename I, bool ADV>
int fbcsr_spmv(hipStream_t st, int64_t n_brows, int64_t bs, const I* row_ptrs, const I* cols,
               const T* vals, const T* b, int64_t ldb, T* c, int64_t ldc, int64_t nrhs,
               const T* alpha, const T* beta)
{
    switch (bs) {
#define GKOC_FBCSR_CASE(B)                                                                        \
    case B:                                                                                       \
        return fbcsr_spmv_launch<B, T, I, ADV>(st, n_brows, row_ptrs, cols, vals, b, ldb, c, ldc, \
                                               nrhs, alpha, beta);
        GKOC_FBCSR_CASE(1)
        GKOC_FBCSR_CASE(2)
        GKOC_FBCSR_CASE(3)
        GKOC_FBCSR_CASE(4)
        GKOC_FBCSR_CASE(5)
        GKOC_FBCSR_CASE(6)
        GKOC_FBCSR_CASE(7)
        GKOC_FBCSR_CASE(8)
#undef GKOC_FBCSR_CASE
    }
    set_last_error("Fbcsr: block size %lld is not one of 1..8", (long long)bs);
    return GKOC_E_NOT_SUPPORTED;
}

// ---- csr::convert_to_fbcsr: thread = block row, a bs-way walk over the (sorted) scalar
// rows.  Each step takes the smallest block column still ahead of any row cursor and moves
// every cursor past its entries in that block column: block columns come out ascending.
// FILL = false counts the blocks, FILL = true writes them (values zeroed first: entries the
// CSR does not hold stay explicit zeros).
template <typename T, typename I, bool FILL>
__global__ __launch_bounds__(256) void csr_to_fbcsr_kernel(
    int64_t n_brows, int bs, const I* __restrict__ rp, const I* __restrict__ cols,
    const T* __restrict__ vals, const I* __restrict__ out_ptrs, I* __restrict__ counts,
    I* __restrict__ out_cols, T* __restrict__ out_vals)
{
    for (int64_t br = int64_t(blockIdx.x) * 256 + threadIdx.x; br < n_brows;
         br += int64_t(gridDim.x) * 256) {
        int64_t pos[fbcsr_max_bs], end[fbcsr_max_bs];
#pragma unroll
        for (int i = 0; i < fbcsr_max_bs; ++i) {
            pos[i] = i < bs ? int64_t(rp[br * bs + i]) : 0;
            end[i] = i < bs ? int64_t(rp[br * bs + i + 1]) : 0;
        }
        int64_t out = FILL ? int64_t(out_ptrs[br]) : 0;
        const int64_t bs2 = int64_t(bs) * bs;
        while (true) {
            int64_t cur = -1;
#pragma unroll
            for (int i = 0; i < fbcsr_max_bs; ++i) {
                if (pos[i] < end[i]) {
                    const int64_t bc = int64_t(cols[pos[i]]) / bs;
                    cur = (cur < 0 || bc < cur) ? bc : cur;
                }
            }
            if (cur < 0) break;
            if (FILL) {
                out_cols[out] = I(cur);
                for (int64_t e = 0; e < bs2; ++e) out_vals[out * bs2 + e] = T(0);
            }
#pragma unroll
            for (int i = 0; i < fbcsr_max_bs; ++i) {
                while (pos[i] < end[i]) {
                    const int64_t cc = cols[pos[i]];
                    if (cc / bs != cur) break;
                    if (FILL) out_vals[out * bs2 + (cc - cur * bs) * bs + i] = vals[pos[i]];
                    ++pos[i];
                }
            }
            ++out;
        }
        if (!FILL) counts[br] = I(out);
    }
}

// ---- fbcsr::convert_to_csr: thread = scalar row r = br bs + i.  Every stored block gives
// bs^2 entries (explicit zeros included); inside a row: block order, then column in block.
template <typename T, typename I>
__global__ __launch_bounds__(256) void fbcsr_to_csr_kernel(
    int64_t n_rows, int bs, const I* __restrict__ rp, const I* __restrict__ bcols,
    const T* __restrict__ bvals, I* __restrict__ out_ptrs, I* __restrict__ out_cols,
    T* __restrict__ out_vals)
{
    const int64_t bs2 = int64_t(bs) * bs;
    for (int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x; r < n_rows;
         r += int64_t(gridDim.x) * 256) {
        const int64_t br = r / bs, i = r - br * bs;
        const int64_t k0 = rp[br], k1 = rp[br + 1];
        const int64_t base = k0 * bs2 + i * (k1 - k0) * bs;
        out_ptrs[r] = I(base);
        if (r == n_rows - 1) out_ptrs[n_rows] = I(k1 * bs2);
        for (int64_t k = k0; k < k1; ++k) {
            const int64_t bc = bcols[k];
            const int64_t o = base + (k - k0) * bs;
            for (int j = 0; j < bs; ++j) {
                out_cols[o + j] = I(bc * bs + j);
                out_vals[o + j] = bvals[k * bs2 + j * bs + i];
            }
        }
    }
}

// ---- fbcsr::fill_in_dense: out (zeroed by the caller, row-major, stride ld) gets every
// stored entry; thread = scalar row
template <typename T, typename I>
__global__ __launch_bounds__(256) void fbcsr_fill_in_dense_kernel(
    int64_t n_rows, int bs, const I* __restrict__ rp, const I* __restrict__ bcols,
    const T* __restrict__ bvals, T* __restrict__ out, int64_t ld)
{
    const int64_t bs2 = int64_t(bs) * bs;
    for (int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x; r < n_rows;
         r += int64_t(gridDim.x) * 256) {
        const int64_t br = r / bs, i = r - br * bs;
        for (int64_t k = rp[br]; k < int64_t(rp[br + 1]); ++k) {
            const int64_t bc = bcols[k];
            for (int j = 0; j < bs; ++j) out[r * ld + bc * bs + j] = bvals[k * bs2 + j * bs + i];
        }
    }
}

// ---- fbcsr::extract_diagonal: diag[r] = A(r, r) from the first block (br, br) of the
// block row, 0 if there is none; r < min(rows, cols)
template <typename T, typename I>
__global__ __launch_bounds__(256) void fbcsr_extract_diagonal_kernel(
    int64_t n_diag, int bs, const I* __restrict__ rp, const I* __restrict__ bcols,
    const T* __restrict__ bvals, T* __restrict__ diag)
{
    const int64_t bs2 = int64_t(bs) * bs;
    for (int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x; r < n_diag;
         r += int64_t(gridDim.x) * 256) {
        const int64_t br = r / bs, i = r - br * bs;
        T d = T(0);
        for (int64_t k = rp[br]; k < int64_t(rp[br + 1]); ++k) {
            if (int64_t(bcols[k]) == br) {
                d = bvals[k * bs2 + i * bs + i];
                break;
            }
        }
        diag[r] = d;
    }
}

// ---- fbcsr::is_sorted_by_column_index: *flag = 0 if a block row has a descending pair
template <typename I>
__global__ __launch_bounds__(256) void fbcsr_is_sorted_kernel(
    int64_t n_brows, const I* __restrict__ rp, const I* __restrict__ bcols, int* __restrict__ flag)
{
    for (int64_t br = int64_t(blockIdx.x) * 256 + threadIdx.x; br < n_brows;
         br += int64_t(gridDim.x) * 256) {
        for (int64_t k = int64_t(rp[br]) + 1; k < int64_t(rp[br + 1]); ++k) {
            if (bcols[k - 1] > bcols[k]) {
                flag[0] = 0;
                break;
            }
        }
    }
}

inline unsigned fb_grid(int64_t n) { return capped_grid(n, 256, max_stream_blocks); }

// the argument checks every entry makes before it touches HIP
#define FB_CHECK_BS(bs)                                                                        \
    do {                                                                                       \
        GKOC_REQUIRE((bs) >= 1, GKOC_E_INVALID, "Fbcsr: block size must be positive");         \
        GKOC_REQUIRE((bs) <= fbcsr_max_bs, GKOC_E_NOT_SUPPORTED,                               \
                     "Fbcsr: block sizes 1..8 only");                                          \
    } while (0)
#define FB_CHECK_DIMS(rows, cols, bs)                                                          \
    do {                                                                                       \
        GKOC_REQUIRE((rows) >= 0 && (cols) >= 0, GKOC_E_INVALID, "Fbcsr: negative size");      \
        GKOC_REQUIRE((rows) % (bs) == 0 && (cols) % (bs) == 0, GKOC_E_INVALID,                 \
                     "Fbcsr: sizes must be divisible by the block size");                      \
    } while (0)
#define FB_CHECK_PTR(p, need) \
    GKOC_REQUIRE((p) != nullptr || !(need), GKOC_E_INVALID, "Fbcsr: null array " #p)

}  // namespace
}  // namespace gkoc

using namespace gkoc;

#define GKOC_DEF_FBCSR(T, TN, I, IN)                                                              \
    extern "C" int gkoc_fbcsr_spmv_##TN##_##IN(                                                   \
        gkoc_stream_t s, int64_t n_block_rows, int64_t n_block_cols, int64_t block_size,          \
        const I* row_ptrs, const I* col_idxs, const T* vals, const T* b, int64_t ldb, T* c,       \
        int64_t ldc, int64_t nrhs)                                                                \
    {                                                                                             \
        FB_CHECK_BS(block_size);                                                                  \
        GKOC_REQUIRE(n_block_rows >= 0 && n_block_cols >= 0 && nrhs >= 0, GKOC_E_INVALID,         \
                     "Fbcsr: negative size");                                                     \
        GKOC_REQUIRE(ldb >= nrhs && ldc >= nrhs, GKOC_E_INVALID, "Fbcsr: stride below nrhs");     \
        const bool work = n_block_rows > 0 && nrhs > 0;                                           \
        FB_CHECK_PTR(row_ptrs, work);                                                             \
        FB_CHECK_PTR(c, work);                                                                    \
        FB_CHECK_PTR(b, work && n_block_cols > 0);                                                \
        if (!work) return GKOC_OK;                                                                \
        return fbcsr_spmv<T, I, false>(as_stream(s), n_block_rows, block_size, row_ptrs,          \
                                       col_idxs, vals, b, ldb, c, ldc, nrhs, nullptr, nullptr);   \
    }                                                                                             \
    extern "C" int gkoc_fbcsr_advanced_spmv_##TN##_##IN(                                          \
        gkoc_stream_t s, int64_t n_block_rows, int64_t n_block_cols, int64_t block_size,          \
        const T* alpha, const I* row_ptrs, const I* col_idxs, const T* vals, const T* b,          \
        int64_t ldb, const T* beta, T* c, int64_t ldc, int64_t nrhs)                              \
    {                                                                                             \
        FB_CHECK_BS(block_size);                                                                  \
        GKOC_REQUIRE(n_block_rows >= 0 && n_block_cols >= 0 && nrhs >= 0, GKOC_E_INVALID,         \
                     "Fbcsr: negative size");                                                     \
        GKOC_REQUIRE(ldb >= nrhs && ldc >= nrhs, GKOC_E_INVALID, "Fbcsr: stride below nrhs");     \
        const bool work = n_block_rows > 0 && nrhs > 0;                                           \
        FB_CHECK_PTR(row_ptrs, work);                                                             \
        FB_CHECK_PTR(c, work);                                                                    \
        FB_CHECK_PTR(alpha, work);                                                                \
        FB_CHECK_PTR(beta, work);                                                                 \
        FB_CHECK_PTR(b, work && n_block_cols > 0);                                                \
        if (!work) return GKOC_OK;                                                                \
        return fbcsr_spmv<T, I, true>(as_stream(s), n_block_rows, block_size, row_ptrs,           \
                                      col_idxs, vals, b, ldb, c, ldc, nrhs, alpha, beta);         \
    }                                                                                             \
    extern "C" int gkoc_csr_convert_to_fbcsr_##TN##_##IN(                                         \
        gkoc_stream_t s, int64_t n_rows, int64_t n_cols, int64_t block_size, const I* row_ptrs,   \
        const I* col_idxs, const T* vals, const I* fb_row_ptrs, I* fb_col_idxs, T* fb_vals)       \
    {                                                                                             \
        FB_CHECK_BS(block_size);                                                                  \
        FB_CHECK_DIMS(n_rows, n_cols, block_size);                                                \
        FB_CHECK_PTR(row_ptrs, n_rows > 0);                                                       \
        FB_CHECK_PTR(fb_row_ptrs, n_rows > 0);                                                    \
        if (n_rows == 0) return GKOC_OK;                                                          \
        const int64_t nbr = n_rows / block_size;                                                  \
        csr_to_fbcsr_kernel<T, I, true><<<dim3(fb_grid(nbr)), dim3(256), 0, as_stream(s)>>>(      \
            nbr, int(block_size), row_ptrs, col_idxs, vals, fb_row_ptrs, nullptr, fb_col_idxs,    \
            fb_vals);                                                                             \
        GKOC_LAUNCH_OK();                                                                         \
        return GKOC_OK;                                                                           \
    }                                                                                             \
    extern "C" int gkoc_fbcsr_convert_to_csr_##TN##_##IN(                                         \
        gkoc_stream_t s, int64_t n_block_rows, int64_t block_size, const I* row_ptrs,             \
        const I* col_idxs, const T* vals, I* csr_row_ptrs, I* csr_col_idxs, T* csr_vals)          \
    {                                                                                             \
        gkoc::csr_structure_written(csr_row_ptrs); gkoc::csr_structure_written(csr_col_idxs);     \
        FB_CHECK_BS(block_size);                                                                  \
        GKOC_REQUIRE(n_block_rows >= 0, GKOC_E_INVALID, "Fbcsr: negative size");                  \
        FB_CHECK_PTR(csr_row_ptrs, true);                                                         \
        FB_CHECK_PTR(row_ptrs, n_block_rows > 0);                                                 \
        const int64_t n = n_block_rows * block_size;                                              \
        if (n == 0) {                                                                             \
            GKOC_HIP(hipMemsetAsync(csr_row_ptrs, 0, sizeof(I), as_stream(s)));                   \
            return GKOC_OK;                                                                       \
        }                                                                                         \
        fbcsr_to_csr_kernel<T, I><<<dim3(fb_grid(n)), dim3(256), 0, as_stream(s)>>>(              \
            n, int(block_size), row_ptrs, col_idxs, vals, csr_row_ptrs, csr_col_idxs, csr_vals);  \
        GKOC_LAUNCH_OK();                                                                         \
        return GKOC_OK;                                                                           \
    }                                                                                             \
    extern "C" int gkoc_fbcsr_fill_in_dense_##TN##_##IN(                                          \
        gkoc_stream_t s, int64_t n_block_rows, int64_t n_block_cols, int64_t block_size,          \
        const I* row_ptrs, const I* col_idxs, const T* vals, T* out, int64_t ld)                  \
    {                                                                                             \
        FB_CHECK_BS(block_size);                                                                  \
        GKOC_REQUIRE(n_block_rows >= 0 && n_block_cols >= 0, GKOC_E_INVALID,                      \
                     "Fbcsr: negative size");                                                     \
        GKOC_REQUIRE(ld >= n_block_cols * block_size, GKOC_E_INVALID,                             \
                     "Fbcsr: stride below the number of columns");                                \
        FB_CHECK_PTR(row_ptrs, n_block_rows > 0);                                                 \
        FB_CHECK_PTR(out, n_block_rows > 0);                                                      \
        const int64_t n = n_block_rows * block_size;                                              \
        if (n == 0) return GKOC_OK;                                                               \
        fbcsr_fill_in_dense_kernel<T, I><<<dim3(fb_grid(n)), dim3(256), 0, as_stream(s)>>>(       \
            n, int(block_size), row_ptrs, col_idxs, vals, out, ld);                               \
        GKOC_LAUNCH_OK();                                                                         \
        return GKOC_OK;                                                                           \
    }                                                                                             \
    extern "C" int gkoc_fbcsr_extract_diagonal_##TN##_##IN(                                       \
        gkoc_stream_t s, int64_t n_rows, int64_t n_cols, int64_t block_size, const I* row_ptrs,   \
        const I* col_idxs, const T* vals, T* diag)                                                \
    {                                                                                             \
        FB_CHECK_BS(block_size);                                                                  \
        FB_CHECK_DIMS(n_rows, n_cols, block_size);                                                \
        const int64_t nd = n_rows < n_cols ? n_rows : n_cols;                                     \
        FB_CHECK_PTR(row_ptrs, nd > 0);                                                           \
        FB_CHECK_PTR(diag, nd > 0);                                                               \
        if (nd == 0) return GKOC_OK;                                                              \
        fbcsr_extract_diagonal_kernel<T, I><<<dim3(fb_grid(nd)), dim3(256), 0, as_stream(s)>>>(   \
            nd, int(block_size), row_ptrs, col_idxs, vals, diag);                                 \
        GKOC_LAUNCH_OK();                                                                         \
        return GKOC_OK;                                                                           \
    }                                                                                             \
    extern "C" int gkoc_fbcsr_is_sorted_by_column_index_##TN##_##IN(                              \
        gkoc_stream_t s, int64_t n_block_rows, const I* row_ptrs, const I* col_idxs,              \
        int* is_sorted_host)                                                                      \
    {                                                                                             \
        GKOC_REQUIRE(is_sorted_host, GKOC_E_INVALID, "null result");                              \
        GKOC_REQUIRE(n_block_rows >= 0, GKOC_E_INVALID, "Fbcsr: negative size");                  \
        FB_CHECK_PTR(row_ptrs, n_block_rows > 0);                                                 \
        *is_sorted_host = 1;                                                                      \
        if (n_block_rows == 0) return GKOC_OK;                                                    \
        int* flag = nullptr;                                                                      \
        GKOC_TRY(scratch_malloc(as_stream(s), reinterpret_cast<void**>(&flag), sizeof(int)));     \
        GKOC_HIP(hipMemsetAsync(flag, 1, sizeof(int), as_stream(s)));                             \
        fbcsr_is_sorted_kernel<I><<<dim3(fb_grid(n_block_rows)), dim3(256), 0, as_stream(s)>>>(   \
            n_block_rows, row_ptrs, col_idxs, flag);                                              \
        GKOC_LAUNCH_OK();                                                                         \
        GKOC_HIP(hipMemcpyAsync(is_sorted_host, flag, sizeof(int), hipMemcpyDeviceToHost,         \
                                as_stream(s)));                                                   \
        GKOC_HIP(hipStreamSynchronize(as_stream(s)));                                             \
        GKOC_TRY(scratch_free(as_stream(s), flag));                                               \
        *is_sorted_host = *is_sorted_host != 0;                                                   \
        return GKOC_OK;                                                                           \
    }

// csr::convert_to_fbcsr, first pass (index type only): fb_row_ptrs (n_rows / bs + 1 entries)
// gets the number of distinct block columns of every block row, scanned in place; the number
// of blocks is returned in HOST memory (synchronises the stream)
#define GKOC_DEF_FBCSR_IDX(I, IN)                                                                 \
    extern "C" int gkoc_csr_convert_to_fbcsr_row_ptrs_##IN(                                       \
        gkoc_stream_t s, int64_t n_rows, int64_t n_cols, int64_t block_size, const I* row_ptrs,   \
        const I* col_idxs, I* fb_row_ptrs, int64_t* num_blocks_host)                              \
    {                                                                                             \
        FB_CHECK_BS(block_size);                                                                  \
        FB_CHECK_DIMS(n_rows, n_cols, block_size);                                                \
        GKOC_REQUIRE(num_blocks_host, GKOC_E_INVALID, "null result");                             \
        FB_CHECK_PTR(fb_row_ptrs, true);                                                          \
        FB_CHECK_PTR(row_ptrs, n_rows > 0);                                                       \
        *num_blocks_host = 0;                                                                     \
        const int64_t nbr = n_rows / block_size;                                                  \
        if (nbr == 0) {                                                                           \
            GKOC_HIP(hipMemsetAsync(fb_row_ptrs, 0, sizeof(I), as_stream(s)));                    \
            return GKOC_OK;                                                                       \
        }                                                                                         \
        csr_to_fbcsr_kernel<double, I, false><<<dim3(fb_grid(nbr)), dim3(256), 0, as_stream(s)>>>( \
            nbr, int(block_size), row_ptrs, col_idxs, nullptr, nullptr, fb_row_ptrs, nullptr,     \
            nullptr);                                                                             \
        GKOC_LAUNCH_OK();                                                                         \
        GKOC_TRY(device_exclusive_scan<I>(as_stream(s), fb_row_ptrs, nbr + 1));                   \
        I total = 0;                                                                              \
        GKOC_HIP(hipMemcpyAsync(&total, fb_row_ptrs + nbr, sizeof(I), hipMemcpyDeviceToHost,      \
                                as_stream(s)));                                                   \
        GKOC_HIP(hipStreamSynchronize(as_stream(s)));                                             \
        *num_blocks_host = int64_t(total);                                                        \
        return GKOC_OK;                                                                           \
    }

GKOC_DEF_FBCSR(double, f64, int32_t, i32)
GKOC_DEF_FBCSR(double, f64, int64_t, i64)
GKOC_DEF_FBCSR(float, f32, int32_t, i32)
GKOC_DEF_FBCSR(float, f32, int64_t, i64)
GKOC_DEF_FBCSR_IDX(int32_t, i32)
GKOC_DEF_FBCSR_IDX(int64_t, i64)
