// Kernels on complex value types (gkoc_c128 / gkoc_c64 = gkoc_cplx<double / float>, complex_type.hpp) that
// Ginkgo's distributed solvers and their tests need around REAL systems - a real solver applied to complex
// vectors works on their real views, but residual checks, updates and reductions of the complex vectors
// themselves come here - and two real entries that share their kernels.  In this order:
//   Dense, element-wise: scale, inv_scale, add_scaled, sub_scaled with a complex or a real scalar (ValueType /
//     ScalarType of core/matrix/dense_kernels.hpp:34-61); make_complex, get_real, get_imag, conj_transpose;
//     row_gather, fill_in_matrix_data; absolute (in place / outplace)
//   Dense, per column: compute_dot, compute_conj_dot, compute_squared_norm2, compute_sum, compute_mean,
//     compute_norm1, and compute_mean for REAL values (the one real reduction dense.hip does not have)
//   Csr: the thread-per-row SpMV (simple / advanced), extract_diagonal and row_wise_absolute_sum (the latter
//     for REAL values too: gkoc_csr_row_wise_absolute_sum_*), scale_by_diagonal (diagonal::apply_to_csr,
//     right_apply_to_csr and the inverse)
//   scalar Jacobi: invert_diagonal, simple_scalar_apply / scalar_apply
//   Dense -> Csr: count_nonzeros_per_row, convert_to_csr
//   Coo: spmv2 / advanced_spmv2 with atomic adds
// Semantics: reference/matrix/dense_kernels.cpp (:184-300 element-wise, :300-440 reductions, :832-841, :916-925,
// :1208-1250).  Plain 2-D indexed kernels (strided views, per-column scalars), reductions as a fixed two-level
// tree per column (reduce_columns); the complex arithmetic is complex_type.hpp's: products as (ac - bd, ad + bc)
// with separate multiplies and adds, quotients by Smith's scaled method.
#include <hip/hip_runtime.h>

#include "common.hpp"

namespace gkoc {
namespace {

#define GKOC_FOR2(idx, total)                                                                          \
    for (int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x, idx##_s = int64_t(gridDim.x) * 256;     \
         idx < (total); idx += idx##_s)

// op: 0 scale, 1 inv_scale, 2 add_scaled (y += a x), 3 sub_scaled (y -= a x); S = scalar type (T or real_t<T>)
template <typename T, typename S, int OP>
__global__ __launch_bounds__(256) void cx_axpy_kernel(int64_t rows, int64_t cols, const S* __restrict__ alpha,
                                                     int64_t alpha_cols, const T* __restrict__ x, int64_t ldx,
                                                     T* __restrict__ y, int64_t ldy)
{
    GKOC_FOR2(i, rows * cols)
    {
        const int64_t r = i / cols, c = i - r * cols;
        const S a = alpha[alpha_cols == 1 ? 0 : c];
        T& yy = y[r * ldy + c];
        if (OP == 0) {
            // (the reference scales by an exact zero like by any value; NaN * 0 stays NaN)
            yy = yy * a;
        } else if (OP == 1) {
            yy = yy / a;
        } else if (OP == 2) {
            yy = yy + x[r * ldx + c] * a;
        } else {
            yy = yy - x[r * ldx + c] * a;
        }
    }
}

// reductions over the rows of one column: kind 0 x*y, 1 conj(x)*y, 2 |x|^2 (real), 3 x (sum, mean)
template <typename T, int KIND>
__global__ __launch_bounds__(256) void cx_reduce_stage1(int64_t rows, int64_t cols, const T* __restrict__ x,
                                                       int64_t ldx, const T* __restrict__ y, int64_t ldy,
                                                       T* __restrict__ partial)
{
    using R = real_t<T>;
    __shared__ R lds[4];
    const int64_t col = blockIdx.y;
    R are = R(0), aim = R(0);
    for (int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x; r < rows; r += int64_t(gridDim.x) * 256) {
        const T a = x[r * ldx + col];
        T t;
        if (KIND == 0) {
            t = a * y[r * ldy + col];
        } else if (KIND == 1) {
            t = conj_v(a) * y[r * ldy + col];
        } else if (KIND == 2) {
            t = {squared_norm_v(a), R(0)};
        } else {
            t = a;
        }
        are += t.re;
        aim += t.im;
    }
    // the two parts one after the other through the same four words of LDS
    const R sre = block_sum<256>(are, lds);
    __syncthreads();
    const R sim = block_sum<256>(aim, lds);
    if (threadIdx.x == 0) partial[col * gridDim.x + blockIdx.x] = {sre, sim};
}

// mode 0: complex result; 1: real part only (squared norm); 2: complex result / rows (mean)
template <typename T>
__global__ __launch_bounds__(256) void cx_reduce_stage2(int n_partials, const T* __restrict__ partial,
                                                       void* __restrict__ result, int mode, int64_t rows)
{
    using R = real_t<T>;
    __shared__ R lds[4];
    const int64_t col = blockIdx.x;
    R are = R(0), aim = R(0);
    for (int i = threadIdx.x; i < n_partials; i += 256) {
        are += partial[col * n_partials + i].re;
        aim += partial[col * n_partials + i].im;
    }
    const R sre = block_sum<256>(are, lds);
    __syncthreads();
    const R sim = block_sum<256>(aim, lds);
    if (threadIdx.x == 0) {
        if (mode == 1) {
            static_cast<R*>(result)[col] = sre;
        } else if (mode == 2) {
            static_cast<T*>(result)[col] = {sre / R(rows), sim / R(rows)};
        } else {
            static_cast<T*>(result)[col] = {sre, sim};
        }
    }
}

// The host side of every two-stage column reduction of this file: up to 256 blocks of 256 threads per column,
// 2048 rows each before they stride, write one partial (of type P) per block and column; one block per column
// folds them.  stage1(grid, stream, partial) and stage2(grid, stream, n_partials, partial) are the two launches.
// No rows: result (result_bytes_per_col per column) is zeroed, also where the result is a mean.
template <typename P, typename Stage1, typename Stage2>
int reduce_columns(gkoc_stream_t s, int64_t rows, int64_t cols, void* result, size_t result_bytes_per_col,
                   Stage1 stage1, Stage2 stage2)
{
    GKOC_REQUIRE(rows >= 0 && cols >= 0, GKOC_E_INVALID, "negative dimension");
    if (cols == 0) return GKOC_OK;
    hipStream_t st = as_stream(s);
    if (rows == 0) {
        GKOC_HIP(hipMemsetAsync(result, 0, size_t(cols) * result_bytes_per_col, st));
        return GKOC_OK;
    }
    int64_t nb = ceildiv(rows, 2048);
    if (nb > 256) nb = 256;
    void* raw = nullptr;
    GKOC_TRY(scratch_malloc(st, &raw, size_t(nb * cols) * sizeof(P)));
    scratch_guard guard{st, raw};
    stage1(dim3(unsigned(nb), unsigned(cols)), st, static_cast<P*>(raw));
    stage2(dim3(unsigned(cols)), st, int(nb), static_cast<const P*>(raw));
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

template <typename T, int KIND>
int cx_reduce(gkoc_stream_t s, int64_t rows, int64_t cols, const T* x, int64_t ldx, const T* y, int64_t ldy,
              void* result, int mode)
{
    return reduce_columns<T>(
        s, rows, cols, result, mode == 1 ? sizeof(real_t<T>) : sizeof(T),
        [&](dim3 grid, hipStream_t st, T* partial) {
            cx_reduce_stage1<T, KIND><<<grid, dim3(256), 0, st>>>(rows, cols, x, ldx, y, ldy, partial);
        },
        [&](dim3 grid, hipStream_t st, int nb, const T* partial) {
            cx_reduce_stage2<T><<<grid, dim3(256), 0, st>>>(nb, partial, result, mode, rows);
        });
}

// real columns: mean (the only real reduction that was missing)
template <typename R>
__global__ __launch_bounds__(256) void real_mean_stage1(int64_t rows, const R* __restrict__ x, int64_t ldx,
                                                       R* __restrict__ partial)
{
    __shared__ R lds[4];
    const int64_t col = blockIdx.y;
    R acc = R(0);
    for (int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x; r < rows; r += int64_t(gridDim.x) * 256) {
        acc += x[r * ldx + col];
    }
    const R sum = block_sum<256>(acc, lds);
    if (threadIdx.x == 0) partial[col * gridDim.x + blockIdx.x] = sum;
}

template <typename R>
__global__ __launch_bounds__(256) void real_mean_stage2(int n_partials, const R* __restrict__ partial,
                                                       R* __restrict__ result, int64_t rows)
{
    __shared__ R lds[4];
    R acc = R(0);
    for (int i = threadIdx.x; i < n_partials; i += 256) acc += partial[int64_t(blockIdx.x) * n_partials + i];
    const R sum = block_sum<256>(acc, lds);
    if (threadIdx.x == 0) result[blockIdx.x] = sum / R(rows);
}

template <typename R>
int real_mean(gkoc_stream_t s, int64_t rows, int64_t cols, const R* x, int64_t ldx, R* result)
{
    return reduce_columns<R>(
        s, rows, cols, result, sizeof(R),
        [&](dim3 grid, hipStream_t st, R* partial) {
            real_mean_stage1<R><<<grid, dim3(256), 0, st>>>(rows, x, ldx, partial);
        },
        [&](dim3 grid, hipStream_t st, int nb, const R* partial) {
            real_mean_stage2<R><<<grid, dim3(256), 0, st>>>(nb, partial, result, rows);
        });
}

// mode 0: make_complex (real in), 1: get_real, 2: get_imag (real out), 3: conj transpose
template <typename T>
__global__ __launch_bounds__(256) void cx_convert_kernel(int64_t rows, int64_t cols, const void* __restrict__ in,
                                                        int64_t ld_in, void* __restrict__ out, int64_t ld_out,
                                                        int mode)
{
    using R = real_t<T>;
    GKOC_FOR2(i, rows * cols)
    {
        const int64_t r = i / cols, c = i - r * cols;
        if (mode == 0) {
            static_cast<T*>(out)[r * ld_out + c] = {static_cast<const R*>(in)[r * ld_in + c], R(0)};
        } else if (mode == 1) {
            static_cast<R*>(out)[r * ld_out + c] = static_cast<const T*>(in)[r * ld_in + c].re;
        } else if (mode == 2) {
            static_cast<R*>(out)[r * ld_out + c] = static_cast<const T*>(in)[r * ld_in + c].im;
        } else {
            // out is cols x rows
            static_cast<T*>(out)[c * ld_out + r] = conj_v(static_cast<const T*>(in)[r * ld_in + c]);
        }
    }
}

template <typename T, typename I>
__global__ __launch_bounds__(256) void cx_row_gather_kernel(int64_t n_gather, int64_t cols, const I* __restrict__ rows,
                                                           const T* __restrict__ orig, int64_t ld_orig,
                                                           T* __restrict__ out, int64_t ld_out)
{
    GKOC_FOR2(i, n_gather * cols)
    {
        const int64_t r = i / cols, c = i - r * cols;
        out[r * ld_out + c] = orig[int64_t(rows[r]) * ld_orig + c];
    }
}

template <typename T, typename I>
__global__ __launch_bounds__(256) void cx_fill_in_kernel(int64_t nnz, const I* __restrict__ rows,
                                                        const I* __restrict__ cols, const T* __restrict__ vals,
                                                        T* __restrict__ out, int64_t ld)
{
    GKOC_FOR2(i, nnz) out[int64_t(rows[i]) * ld + int64_t(cols[i])] = vals[i];
}

// mode 0: x = |x| + 0i in place; 1: out (reals) = |x|, |x| as hypot (what std::abs of a complex value computes)
template <typename T>
__global__ __launch_bounds__(256) void cx_abs_kernel(int64_t rows, int64_t cols, T* __restrict__ x, int64_t ldx,
                                                    real_t<T>* __restrict__ out, int64_t ld_out, int mode)
{
    using R = real_t<T>;
    GKOC_FOR2(i, rows * cols)
    {
        const int64_t r = i / cols, c = i - r * cols;
        const R a = abs_v(x[r * ldx + c]);
        if (mode == 0) {
            x[r * ldx + c] = {a, R(0)};
        } else {
            out[r * ld_out + c] = a;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void cx_norm1_stage1(int64_t rows, const T* __restrict__ x, int64_t ldx,
                                                      real_t<T>* __restrict__ partial)
{
    using R = real_t<T>;
    __shared__ R lds[4];
    const int64_t col = blockIdx.y;
    R acc = R(0);
    for (int64_t r = int64_t(blockIdx.x) * 256 + threadIdx.x; r < rows; r += int64_t(gridDim.x) * 256) {
        acc += abs_v(x[r * ldx + col]);
    }
    const R sum = block_sum<256>(acc, lds);
    if (threadIdx.x == 0) partial[col * gridDim.x + blockIdx.x] = sum;
}

template <typename T>
int cx_norm1(gkoc_stream_t s, int64_t rows, int64_t cols, const T* x, int64_t ldx, real_t<T>* result)
{
    using R = real_t<T>;
    return reduce_columns<R>(
        s, rows, cols, result, sizeof(R),
        [&](dim3 grid, hipStream_t st, R* partial) {
            cx_norm1_stage1<T><<<grid, dim3(256), 0, st>>>(rows, x, ldx, partial);
        },
        [&](dim3 grid, hipStream_t st, int nb, const R* partial) {
            // the second stage of the mean with a divisor of 1
            real_mean_stage2<R><<<grid, dim3(256), 0, st>>>(nb, partial, result, 1);
        });
}

// CSR with complex values, one thread per (row, right-hand side): y = A x, or y = alpha A x + beta y
template <typename T, typename I, bool ADVANCED>
__global__ __launch_bounds__(256) void cx_csr_spmv_kernel(int64_t rows, int64_t nrhs, const I* __restrict__ row_ptrs,
                                                         const I* __restrict__ col_idxs, const T* __restrict__ vals,
                                                         const T* __restrict__ alpha, const T* __restrict__ x,
                                                         int64_t ldx, const T* __restrict__ beta, T* __restrict__ y,
                                                         int64_t ldy)
{
    GKOC_FOR2(i, rows * nrhs)
    {
        const int64_t r = i / nrhs, c = i - r * nrhs;
        T acc = T(0);
        for (I k = row_ptrs[r]; k < row_ptrs[r + 1]; ++k) acc = acc + vals[k] * x[int64_t(col_idxs[k]) * ldx + c];
        if (ADVANCED) {
            const T b = beta[0];
            const T ax = alpha[0] * acc;
            // (zero is spelled T{} in this file: against T(0) the float kernels compile to two float compares
            // instead of one integer test of both parts)
            y[r * ldy + c] = b == T{} ? ax : ax + b * y[r * ldy + c];
        } else {
            y[r * ldy + c] = acc;
        }
    }
}

// |a| as the row scan sums it: abs_v, except that real values keep the sign flip these kernels have always had
// (it leaves -0 alone where abs_v's fabs does not, so the four real kernels would compile to other code)
template <typename R>
__device__ __forceinline__ R abs_of(R a) { return a < R(0) ? -a : a; }
template <typename R>
__device__ __forceinline__ R abs_of(gkoc_cplx<R> a) { return abs_v(a); }

// mode 0: diag[row] = a(row,row) where stored; 1: sum[row] = sum_k |a_k| (+ 0i); V real or complex
template <typename V, typename I>
__global__ __launch_bounds__(256) void csr_row_scan_kernel(int64_t rows, const I* __restrict__ row_ptrs,
                                                          const I* __restrict__ col_idxs,
                                                          const V* __restrict__ vals, V* __restrict__ out, int mode)
{
    GKOC_FOR2(r, rows)
    {
        if (mode == 0) {
            for (I k = row_ptrs[r]; k < row_ptrs[r + 1]; ++k) {
                if (int64_t(col_idxs[k]) == r) {
                    out[r] = vals[k];
                    break;
                }
            }
        } else {
            real_t<V> acc = 0;
            for (I k = row_ptrs[r]; k < row_ptrs[r + 1]; ++k) acc += abs_of(vals[k]);
            out[r] = V{acc};
        }
    }
}

// scalar Jacobi and Diagonal products on complex values (jacobi::{invert_diagonal,
// simple_scalar_apply, scalar_apply}, diagonal::{apply_to_csr, right_apply_to_csr};
// reference/preconditioner/jacobi_kernels.cpp:535-592, reference/matrix/diagonal_kernels.cpp:60-102)
template <typename T>
__global__ __launch_bounds__(256) void cx_invert_kernel(int64_t n, const T* __restrict__ d, T* __restrict__ inv)
{
    GKOC_FOR2(i, n)
    {
        // a zero entry inverts as one: (1, +0), written as such
        const T one = T(1);
        inv[i] = d[i] == T{} ? one : one / d[i];
    }
}

// x(i,j) = b(i,j) d[i], or beta x(i,j) + (alpha b(i,j)) d[i]
template <typename T, bool ADVANCED>
__global__ __launch_bounds__(256) void cx_row_scale_kernel(int64_t rows, int64_t cols, const T* __restrict__ d,
                                                          const T* __restrict__ alpha, const T* __restrict__ b,
                                                          int64_t ldb, const T* __restrict__ beta,
                                                          T* __restrict__ x, int64_t ldx)
{
    GKOC_FOR2(i, rows * cols)
    {
        const int64_t r = i / cols, c = i - r * cols;
        if (ADVANCED) {
            x[r * ldx + c] = beta[0] * x[r * ldx + c] + (alpha[0] * b[r * ldb + c]) * d[r];
        } else {
            x[r * ldx + c] = b[r * ldb + c] * d[r];
        }
    }
}

// mode 0: vals[k] *= d[row]; 1: vals[k] *= 1 / d[row]; 2: vals[k] *= d[col[k]]
template <typename T, typename I>
__global__ __launch_bounds__(256) void cx_csr_scale_kernel(int64_t n_rows, const I* __restrict__ row_ptrs,
                                                          const I* __restrict__ cols, const T* __restrict__ d,
                                                          int mode, T* __restrict__ vals)
{
    GKOC_FOR2(r, n_rows)
    {
        const T s = mode == 1 ? T(1) / d[r] : d[r];
        for (I k = row_ptrs[r]; k < row_ptrs[r + 1]; ++k) {
            vals[k] = vals[k] * (mode == 2 ? d[cols[k]] : s);
        }
    }
}

// Dense -> Csr with complex values (dense::count_nonzeros_per_row / convert_to_csr): one lane per
// row; the entries of a row keep their column order
template <typename T>
__global__ __launch_bounds__(256) void cx_dense_count_kernel(int64_t rows, int64_t cols, const T* __restrict__ in,
                                                            int64_t ld, void* __restrict__ out, int out_bytes)
{
    GKOC_FOR2(r, rows)
    {
        int64_t n = 0;
        for (int64_t c = 0; c < cols; ++c) n += in[r * ld + c] != T{};
        if (out_bytes == 4) {
            static_cast<int32_t*>(out)[r] = int32_t(n);
        } else {
            static_cast<int64_t*>(out)[r] = n;
        }
    }
}

template <typename T, typename I>
__global__ __launch_bounds__(256) void cx_dense_to_csr_kernel(int64_t rows, int64_t cols, const T* __restrict__ in,
                                                             int64_t ld, const I* __restrict__ row_ptrs,
                                                             I* __restrict__ out_cols, T* __restrict__ out_vals)
{
    GKOC_FOR2(r, rows)
    {
        int64_t k = row_ptrs[r];
        for (int64_t c = 0; c < cols; ++c) {
            const T v = in[r * ld + c];
            if (v != T{}) {
                out_cols[k] = I(c);
                out_vals[k] = v;
                ++k;
            }
        }
    }
}

// Coo with complex values: c(row, j) += [alpha] val b(col, j), entry by entry with atomic adds of the
// real and imaginary parts (the only kernels of this library whose summation order is not fixed:
// the complex instantiations exist so that Ginkgo's distributed Matrix runs with a Coo non-local
// part on complex data, they are not a tuned path)
template <typename T, typename I>
__global__ __launch_bounds__(256) void cx_coo_spmv2_kernel(int64_t nnz, int64_t nrhs, const I* __restrict__ rows,
                                                          const I* __restrict__ cols, const T* __restrict__ vals,
                                                          const T* __restrict__ alpha, const T* __restrict__ b,
                                                          int64_t ldb, T* __restrict__ c, int64_t ldc)
{
    GKOC_FOR2(i, nnz * nrhs)
    {
        const int64_t k = i / nrhs, j = i - k * nrhs;
        T t = vals[k] * b[int64_t(cols[k]) * ldb + j];
        if (alpha) t = alpha[0] * t;
        T* dst = c + int64_t(rows[k]) * ldc + j;
        atomicAdd(&dst->re, t.re);
        atomicAdd(&dst->im, t.im);
    }
}

// alpha: alpha_cols values of T, or of real_t<T> where scalar_is_real (a matrix of remove_complex<ValueType>)
template <typename T, int OP>
int cx_axpy(gkoc_stream_t s, int64_t rows, int64_t cols, const void* alpha, int64_t alpha_cols, int scalar_is_real,
            const T* x, int64_t ldx, T* y, int64_t ldy)
{
    using R = real_t<T>;
    if (rows <= 0 || cols <= 0) return GKOC_OK;
    GKOC_REQUIRE(alpha && (alpha_cols == 1 || alpha_cols == cols), GKOC_E_INVALID, "bad alpha");
    const dim3 g(stream_grid(rows * cols));
    if (scalar_is_real) {
        cx_axpy_kernel<T, R, OP><<<g, dim3(256), 0, as_stream(s)>>>(rows, cols, static_cast<const R*>(alpha),
                                                                    alpha_cols, x, ldx, y, ldy);
    } else {
        cx_axpy_kernel<T, T, OP><<<g, dim3(256), 0, as_stream(s)>>>(rows, cols, static_cast<const T*>(alpha),
                                                                    alpha_cols, x, ldx, y, ldy);
    }
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

}  // namespace
}  // namespace gkoc

using namespace gkoc;

#define GKOC_DEF_CBLAS(T, TN)                                                                               \
    extern "C" int gkoc_cdense_scale_##TN(gkoc_stream_t s, int64_t rows, int64_t cols, const void* alpha,   \
                                          int64_t alpha_cols, int scalar_is_real, T* x, int64_t ldx)        \
    {                                                                                                       \
        return cx_axpy<T, 0>(s, rows, cols, alpha, alpha_cols, scalar_is_real, nullptr, 0, x, ldx);         \
    }                                                                                                       \
    extern "C" int gkoc_cdense_inv_scale_##TN(gkoc_stream_t s, int64_t rows, int64_t cols,                  \
                                              const void* alpha, int64_t alpha_cols, int scalar_is_real,    \
                                              T* x, int64_t ldx)                                            \
    {                                                                                                       \
        return cx_axpy<T, 1>(s, rows, cols, alpha, alpha_cols, scalar_is_real, nullptr, 0, x, ldx);         \
    }                                                                                                       \
    extern "C" int gkoc_cdense_add_scaled_##TN(gkoc_stream_t s, int64_t rows, int64_t cols,                 \
                                               const void* alpha, int64_t alpha_cols, int scalar_is_real,   \
                                               const T* x, int64_t ldx, T* y, int64_t ldy)                  \
    {                                                                                                       \
        return cx_axpy<T, 2>(s, rows, cols, alpha, alpha_cols, scalar_is_real, x, ldx, y, ldy);             \
    }                                                                                                       \
    extern "C" int gkoc_cdense_sub_scaled_##TN(gkoc_stream_t s, int64_t rows, int64_t cols,                 \
                                               const void* alpha, int64_t alpha_cols, int scalar_is_real,   \
                                               const T* x, int64_t ldx, T* y, int64_t ldy)                  \
    {                                                                                                       \
        return cx_axpy<T, 3>(s, rows, cols, alpha, alpha_cols, scalar_is_real, x, ldx, y, ldy);             \
    }                                                                                                       \
    extern "C" int gkoc_cdense_compute_dot_##TN(gkoc_stream_t s, int64_t rows, int64_t cols, const T* x,    \
                                                int64_t ldx, const T* y, int64_t ldy, T* result,            \
                                                int conjugate_x)                                            \
    {                                                                                                       \
        return conjugate_x ? cx_reduce<T, 1>(s, rows, cols, x, ldx, y, ldy, result, 0)                      \
                           : cx_reduce<T, 0>(s, rows, cols, x, ldx, y, ldy, result, 0);                     \
    }                                                                                                       \
    extern "C" int gkoc_cdense_compute_squared_norm2_##TN(gkoc_stream_t s, int64_t rows, int64_t cols,      \
                                                          const T* x, int64_t ldx, real_t<T>* result)       \
    {                                                                                                       \
        return cx_reduce<T, 2>(s, rows, cols, x, ldx, nullptr, 0, result, 1);                               \
    }                                                                                                       \
    extern "C" int gkoc_cdense_compute_sum_##TN(gkoc_stream_t s, int64_t rows, int64_t cols, const T* x,    \
                                                int64_t ldx, T* result)                                     \
    {                                                                                                       \
        return cx_reduce<T, 3>(s, rows, cols, x, ldx, nullptr, 0, result, 0);                               \
    }                                                                                                       \
    extern "C" int gkoc_cdense_compute_mean_##TN(gkoc_stream_t s, int64_t rows, int64_t cols, const T* x,   \
                                                 int64_t ldx, T* result)                                    \
    {                                                                                                       \
        return cx_reduce<T, 3>(s, rows, cols, x, ldx, nullptr, 0, result, 2);                               \
    }                                                                                                       \
    /* mode 0 make_complex (in: reals), 1 get_real, 2 get_imag (out: reals), 3 conj_transpose (out cols x   \
       rows) */                                                                                             \
    extern "C" int gkoc_cdense_convert_##TN(gkoc_stream_t s, int64_t rows, int64_t cols, const void* in,    \
                                            int64_t ld_in, void* out, int64_t ld_out, int mode)             \
    {                                                                                                       \
        GKOC_REQUIRE(mode >= 0 && mode <= 3, GKOC_E_INVALID, "mode");                                       \
        if (rows <= 0 || cols <= 0) return GKOC_OK;                                                         \
        cx_convert_kernel<T><<<dim3(stream_grid(rows * cols)), dim3(256), 0, as_stream(s)>>>(               \
            rows, cols, in, ld_in, out, ld_out, mode);                                                      \
        GKOC_LAUNCH_OK();                                                                                   \
        return GKOC_OK;                                                                                     \
    }
GKOC_DEF_CBLAS(gkoc_c128, c128)
GKOC_DEF_CBLAS(gkoc_c64, c64)

#define GKOC_DEF_CABS(T, TN)                                                                                \
    /* mode 0: x = |x| in place (imaginary parts 0); 1: out (reals, ld_out) = |x| */                        \
    extern "C" int gkoc_cdense_absolute_##TN(gkoc_stream_t s, int64_t rows, int64_t cols, T* x,             \
                                             int64_t ldx, real_t<T>* out, int64_t ld_out, int mode)         \
    {                                                                                                       \
        GKOC_REQUIRE(mode == 0 || mode == 1, GKOC_E_INVALID, "mode");                                       \
        if (rows <= 0 || cols <= 0) return GKOC_OK;                                                         \
        cx_abs_kernel<T><<<dim3(stream_grid(rows * cols)), dim3(256), 0, as_stream(s)>>>(rows, cols, x,     \
                                                                                         ldx, out, ld_out,  \
                                                                                         mode);             \
        GKOC_LAUNCH_OK();                                                                                   \
        return GKOC_OK;                                                                                     \
    }                                                                                                       \
    extern "C" int gkoc_cdense_compute_norm1_##TN(gkoc_stream_t s, int64_t rows, int64_t cols, const T* x,  \
                                                  int64_t ldx, real_t<T>* result)                           \
    {                                                                                                       \
        return cx_norm1<T>(s, rows, cols, x, ldx, result);                                                  \
    }
GKOC_DEF_CABS(gkoc_c128, c128)
GKOC_DEF_CABS(gkoc_c64, c64)

#define GKOC_DEF_CBLAS_I(T, TN, I, IN)                                                                      \
    extern "C" int gkoc_cdense_row_gather_##TN##_##IN(gkoc_stream_t s, int64_t n_gather, int64_t cols,      \
                                                      const I* rows, const T* orig, int64_t ld_orig,        \
                                                      T* gathered, int64_t ld_gathered)                     \
    {                                                                                                       \
        if (n_gather <= 0 || cols <= 0) return GKOC_OK;                                                     \
        cx_row_gather_kernel<T, I><<<dim3(stream_grid(n_gather * cols)), dim3(256), 0, as_stream(s)>>>(     \
            n_gather, cols, rows, orig, ld_orig, gathered, ld_gathered);                                    \
        GKOC_LAUNCH_OK();                                                                                   \
        return GKOC_OK;                                                                                     \
    }                                                                                                       \
    extern "C" int gkoc_cdense_fill_in_matrix_data_##TN##_##IN(gkoc_stream_t s, int64_t nnz, const I* rows, \
                                                               const I* cols, const T* vals, T* out,        \
                                                               int64_t ld)                                  \
    {                                                                                                       \
        if (nnz <= 0) return GKOC_OK;                                                                       \
        cx_fill_in_kernel<T, I><<<dim3(stream_grid(nnz)), dim3(256), 0, as_stream(s)>>>(nnz, rows, cols,    \
                                                                                        vals, out, ld);     \
        GKOC_LAUNCH_OK();                                                                                   \
        return GKOC_OK;                                                                                     \
    }
GKOC_DEF_CBLAS_I(gkoc_c128, c128, int32_t, i32)
GKOC_DEF_CBLAS_I(gkoc_c128, c128, int64_t, i64)
GKOC_DEF_CBLAS_I(gkoc_c64, c64, int32_t, i32)
GKOC_DEF_CBLAS_I(gkoc_c64, c64, int64_t, i64)

#define GKOC_DEF_MEAN(R, RN)                                                                                \
    extern "C" int gkoc_dense_compute_mean_##RN(gkoc_stream_t s, int64_t rows, int64_t cols, const R* x,    \
                                                int64_t ldx, R* result)                                     \
    {                                                                                                       \
        return real_mean<R>(s, rows, cols, x, ldx, result);                                                 \
    }
GKOC_DEF_MEAN(double, f64)
GKOC_DEF_MEAN(float, f32)

#define GKOC_DEF_CCSR(T, TN, I, IN)                                                                         \
    /* alpha == NULL: y = A x; else y = alpha[0] A x + beta[0] y (scalars on the device) */                 \
    extern "C" int gkoc_ccsr_spmv_##TN##_##IN(gkoc_stream_t s, int64_t rows, int64_t nrhs,                  \
                                              const I* row_ptrs, const I* col_idxs, const T* vals,          \
                                              const T* alpha, const T* x, int64_t ldx, const T* beta, T* y, \
                                              int64_t ldy)                                                  \
    {                                                                                                       \
        if (rows <= 0 || nrhs <= 0) return GKOC_OK;                                                         \
        GKOC_REQUIRE((alpha == nullptr) == (beta == nullptr), GKOC_E_INVALID, "alpha and beta go together");\
        /* the row-segment kernel of the real types (csr_spmv.hip) unless the arrays are not aligned for   \
           it or GKOC_TUNE_CCSR_THREAD_PER_ROW asks for round 5's kernel (A/B runs) */                      \
        if (tune_value(GKOC_TUNE_CCSR_THREAD_PER_ROW) == 0) {                                               \
            const int rc_ = csr_spmv_complex<T, I>(s, rows, nrhs, row_ptrs, col_idxs, vals, alpha, x, ldx,  \
                                                   beta, y, ldy);                                           \
            if (rc_ != GKOC_E_NOT_SUPPORTED) return rc_;                                                    \
        }                                                                                                   \
        const dim3 g(stream_grid(rows * nrhs));                                                             \
        if (alpha) {                                                                                        \
            cx_csr_spmv_kernel<T, I, true><<<g, dim3(256), 0, as_stream(s)>>>(                              \
                rows, nrhs, row_ptrs, col_idxs, vals, alpha, x, ldx, beta, y, ldy);                         \
        } else {                                                                                            \
            cx_csr_spmv_kernel<T, I, false><<<g, dim3(256), 0, as_stream(s)>>>(                             \
                rows, nrhs, row_ptrs, col_idxs, vals, nullptr, x, ldx, nullptr, y, ldy);                    \
        }                                                                                                   \
        GKOC_LAUNCH_OK();                                                                                   \
        return GKOC_OK;                                                                                     \
    }                                                                                                       \
    /* mode 0: diag[row] = a(row, row) where it is stored (rows of the diagonal); 1: sums[row] = sum |a| */ \
    extern "C" int gkoc_ccsr_row_scan_##TN##_##IN(gkoc_stream_t s, int64_t rows, const I* row_ptrs,         \
                                                  const I* col_idxs, const T* vals, T* out, int mode)       \
    {                                                                                                       \
        GKOC_REQUIRE(mode == 0 || mode == 1, GKOC_E_INVALID, "mode");                                       \
        if (rows <= 0) return GKOC_OK;                                                                      \
        csr_row_scan_kernel<T, I><<<dim3(stream_grid(rows)), dim3(256), 0, as_stream(s)>>>(                 \
            rows, row_ptrs, col_idxs, vals, out, mode);                                                     \
        GKOC_LAUNCH_OK();                                                                                   \
        return GKOC_OK;                                                                                     \
    }
GKOC_DEF_CCSR(gkoc_c128, c128, int32_t, i32)
GKOC_DEF_CCSR(gkoc_c128, c128, int64_t, i64)
GKOC_DEF_CCSR(gkoc_c64, c64, int32_t, i32)
GKOC_DEF_CCSR(gkoc_c64, c64, int64_t, i64)

#define GKOC_DEF_CCSR_SCALE(T, TN, I, IN)                                                                   \
    /* mode 0: vals *= diag[row]; 1: vals *= 1 / diag[row]; 2: vals *= diag[col] */                         \
    extern "C" int gkoc_ccsr_scale_by_diagonal_##TN##_##IN(gkoc_stream_t s, int64_t n_rows,                 \
                                                           const I* row_ptrs, const I* col_idxs,            \
                                                           const T* diag, int mode, T* vals)                \
    {                                                                                                       \
        GKOC_REQUIRE(mode >= 0 && mode <= 2, GKOC_E_INVALID, "mode");                                       \
        if (n_rows <= 0) return GKOC_OK;                                                                    \
        cx_csr_scale_kernel<T, I><<<dim3(stream_grid(n_rows)), dim3(256), 0, as_stream(s)>>>(               \
            n_rows, row_ptrs, col_idxs, diag, mode, vals);                                                  \
        GKOC_LAUNCH_OK();                                                                                   \
        return GKOC_OK;                                                                                     \
    }
GKOC_DEF_CCSR_SCALE(gkoc_c128, c128, int32_t, i32)
GKOC_DEF_CCSR_SCALE(gkoc_c128, c128, int64_t, i64)
GKOC_DEF_CCSR_SCALE(gkoc_c64, c64, int32_t, i32)
GKOC_DEF_CCSR_SCALE(gkoc_c64, c64, int64_t, i64)

// csr::row_wise_absolute_sum for real values (core/matrix/csr_kernels.hpp:287-290): the L1 smoother
// of the Schwarz preconditioner
#define GKOC_DEF_RWAS(T, TN, I, IN)                                                                         \
    extern "C" int gkoc_csr_row_wise_absolute_sum_##TN##_##IN(gkoc_stream_t s, int64_t rows,                \
                                                              const I* row_ptrs, const T* vals, T* sums)    \
    {                                                                                                       \
        if (rows <= 0) return GKOC_OK;                                                                      \
        csr_row_scan_kernel<T, I><<<dim3(stream_grid(rows)), dim3(256), 0, as_stream(s)>>>(rows, row_ptrs,  \
                                                                                      nullptr, vals, sums,  \
                                                                                      1);                   \
        GKOC_LAUNCH_OK();                                                                                   \
        return GKOC_OK;                                                                                     \
    }
GKOC_DEF_RWAS(double, f64, int32_t, i32)
GKOC_DEF_RWAS(double, f64, int64_t, i64)
GKOC_DEF_RWAS(float, f32, int32_t, i32)
GKOC_DEF_RWAS(float, f32, int64_t, i64)

#define GKOC_DEF_CJAC(T, TN)                                                                                \
    extern "C" int gkoc_cjacobi_invert_diagonal_##TN(gkoc_stream_t s, int64_t n, const T* diag, T* inv)     \
    {                                                                                                       \
        if (n <= 0) return GKOC_OK;                                                                         \
        cx_invert_kernel<T><<<dim3(stream_grid(n)), dim3(256), 0, as_stream(s)>>>(n, diag, inv);            \
        GKOC_LAUNCH_OK();                                                                                   \
        return GKOC_OK;                                                                                     \
    }                                                                                                       \
    /* alpha == NULL: x = diag b (row-wise); else x = beta x + alpha b diag */                              \
    extern "C" int gkoc_cjacobi_scalar_apply_##TN(gkoc_stream_t s, int64_t rows, int64_t cols,              \
                                                  const T* diag, const T* alpha, const T* b, int64_t ldb,   \
                                                  const T* beta, T* x, int64_t ldx)                         \
    {                                                                                                       \
        if (rows <= 0 || cols <= 0) return GKOC_OK;                                                         \
        GKOC_REQUIRE((alpha == nullptr) == (beta == nullptr), GKOC_E_INVALID, "alpha and beta go together");\
        const dim3 g(stream_grid(rows * cols));                                                             \
        if (alpha) {                                                                                        \
            cx_row_scale_kernel<T, true><<<g, dim3(256), 0, as_stream(s)>>>(rows, cols, diag, alpha, b,     \
                                                                            ldb, beta, x, ldx);             \
        } else {                                                                                            \
            cx_row_scale_kernel<T, false><<<g, dim3(256), 0, as_stream(s)>>>(rows, cols, diag, nullptr, b,  \
                                                                             ldb, nullptr, x, ldx);         \
        }                                                                                                   \
        GKOC_LAUNCH_OK();                                                                                   \
        return GKOC_OK;                                                                                     \
    }
GKOC_DEF_CJAC(gkoc_c128, c128)
GKOC_DEF_CJAC(gkoc_c64, c64)

#define GKOC_DEF_CDENSE_CSR(T, TN)                                                                          \
    /* out: int32 / int64 / uint64 counts (out_bytes 4 or 8) */                                             \
    extern "C" int gkoc_cdense_count_nonzeros_per_row_##TN(gkoc_stream_t s, int64_t rows, int64_t cols,     \
                                                           const T* in, int64_t ld, void* out,              \
                                                           int out_bytes)                                   \
    {                                                                                                       \
        GKOC_REQUIRE(out_bytes == 4 || out_bytes == 8, GKOC_E_INVALID, "out_bytes");                        \
        if (rows <= 0) return GKOC_OK;                                                                      \
        cx_dense_count_kernel<T><<<dim3(stream_grid(rows)), dim3(256), 0, as_stream(s)>>>(rows, cols, in,   \
                                                                                          ld, out,          \
                                                                                          out_bytes);       \
        GKOC_LAUNCH_OK();                                                                                   \
        return GKOC_OK;                                                                                     \
    }
GKOC_DEF_CDENSE_CSR(gkoc_c128, c128)
GKOC_DEF_CDENSE_CSR(gkoc_c64, c64)
#define GKOC_DEF_CDENSE_CSR_I(T, TN, I, IN)                                                                 \
    extern "C" int gkoc_cdense_to_csr_##TN##_##IN(gkoc_stream_t s, int64_t rows, int64_t cols, const T* in, \
                                                  int64_t ld, const I* row_ptrs, I* out_cols, T* out_vals)  \
    {                                                                                                       \
        gkoc::csr_structure_written(out_cols);                                                              \
        if (rows <= 0) return GKOC_OK;                                                                      \
        cx_dense_to_csr_kernel<T, I><<<dim3(stream_grid(rows)), dim3(256), 0, as_stream(s)>>>(              \
            rows, cols, in, ld, row_ptrs, out_cols, out_vals);                                              \
        GKOC_LAUNCH_OK();                                                                                   \
        return GKOC_OK;                                                                                     \
    }
GKOC_DEF_CDENSE_CSR_I(gkoc_c128, c128, int32_t, i32)
GKOC_DEF_CDENSE_CSR_I(gkoc_c128, c128, int64_t, i64)
GKOC_DEF_CDENSE_CSR_I(gkoc_c64, c64, int32_t, i32)
GKOC_DEF_CDENSE_CSR_I(gkoc_c64, c64, int64_t, i64)

#define GKOC_DEF_CCOO(T, TN, I, IN)                                                                         \
    /* c += [alpha] A b (alpha == NULL: 1); for c = A b clear c first, for c = alpha A b + beta c scale it */ \
    extern "C" int gkoc_ccoo_spmv2_##TN##_##IN(gkoc_stream_t s, int64_t nnz, int64_t nrhs, const I* rows,   \
                                               const I* cols, const T* vals, const T* alpha, const T* b,    \
                                               int64_t ldb, T* c, int64_t ldc)                              \
    {                                                                                                       \
        if (nnz <= 0 || nrhs <= 0) return GKOC_OK;                                                          \
        cx_coo_spmv2_kernel<T, I><<<dim3(stream_grid(nnz * nrhs)), dim3(256), 0, as_stream(s)>>>(           \
            nnz, nrhs, rows, cols, vals, alpha, b, ldb, c, ldc);                                            \
        GKOC_LAUNCH_OK();                                                                                   \
        return GKOC_OK;                                                                                     \
    }
GKOC_DEF_CCOO(gkoc_c128, c128, int32_t, i32)
GKOC_DEF_CCOO(gkoc_c128, c128, int64_t, i64)
GKOC_DEF_CCOO(gkoc_c64, c64, int32_t, i32)
GKOC_DEF_CCOO(gkoc_c64, c64, int64_t, i64)
