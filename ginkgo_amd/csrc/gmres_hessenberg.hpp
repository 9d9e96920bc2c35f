// The two per-column steps the GMRES family shares (device only): the Givens update of a new
// Hessenberg column and the back substitution y = H^-1 * residual_norm_collection.  One thread
// per right-hand side, the reference's operation order, for real and complex T alike (conj_v /
// abs_v / real_t are the identity for real T).  The kernels of gmres.hip, cb_gmres.hip and
// cb_gmres_complex.hip are their own guard (bounds, stopping status) plus one call.
#pragma once
#include "common.hpp"

namespace gkoc {

// Column `col` of step `iter`: apply the iter earlier rotations to h(0 .. iter + 1), form the new
// one, rotate, and move the residual norm on.  h is the step's Hessenberg column, (iter + 2) x cols.
template <typename T>
__device__ __forceinline__ void hessenberg_column_step(
    int64_t col, int64_t iter, T* __restrict__ gsin, int64_t ld_sin, T* __restrict__ gcos,
    int64_t ld_cos, T* __restrict__ h, int64_t ldh, T* __restrict__ rnc, int64_t ld_rnc,
    real_t<T>* __restrict__ residual_norm)
{
    using R = real_t<T>;
    const int64_t i = col;
    // givens_rotation (common_gmres_kernels.cpp:52-90; conj_v is the identity for real T)
    for (int64_t j = 0; j < iter; ++j) {
        const T c = gcos[j * ld_cos + i], s = gsin[j * ld_sin + i];
        const T hj = h[j * ldh + i], hj1 = h[(j + 1) * ldh + i];
        const T temp = c * hj + s * hj1;
        h[(j + 1) * ldh + i] = -conj_v(s) * hj + conj_v(c) * hj1;
        h[j * ldh + i] = temp;
    }
    // calculate_sin_and_cos (:29-48)
    const T this_h = h[iter * ldh + i];
    const T next_h = h[(iter + 1) * ldh + i];
    T c, s;
    if (this_h == T(0)) {
        c = T(0);
        s = T(1);
    } else {
        const R scale = abs_v(this_h) + abs_v(next_h);
        const R hyp = scale * sqrt(abs_v(this_h / scale) * abs_v(this_h / scale) +
                                   abs_v(next_h / scale) * abs_v(next_h / scale));
        c = conj_v(this_h) / hyp;
        s = conj_v(next_h) / hyp;
    }
    gcos[iter * ld_cos + i] = c;
    gsin[iter * ld_sin + i] = s;
    h[iter * ldh + i] = c * this_h + s * next_h;
    h[(iter + 1) * ldh + i] = T(0);
    // calculate_next_residual_norm (:93-113)
    const T r = rnc[iter * ld_rnc + i];
    const T rn = -conj_v(s) * r;
    rnc[(iter + 1) * ld_rnc + i] = rn;
    rnc[iter * ld_rnc + i] = c * r;
    residual_norm[i] = abs_v(rn);
}

// Where entry (i, j) of right-hand side k's upper triangular H lives in the Hessenberg array.
// Gmres stores a step's column as one ROW of the array (row j holds h(0 .. j + 1) of every column,
// so the step's hessenberg_iter is a contiguous (j + 2) x cols block that multi_dot writes as a
// Dense); CbGmres keeps the reference's (krylov_dim + 1) x (krylov_dim * cols) matrix, a step's
// column a strided block of it (reference/solver/cb_gmres_kernels.cpp:234-253).
enum class hessenberg_layout { row_per_step /* gmres.hip */, matrix /* cb_gmres*.hip */ };

// y(0 .. m - 1, k) = H^-1 rnc(0 .. m - 1, k), m = final_iter_nums[k]; rows of y past m stay
template <typename T, hessenberg_layout Layout>
__device__ __forceinline__ void upper_solve_column(int64_t k, int64_t cols, int64_t m,
                                                   const T* __restrict__ rnc, int64_t ld_rnc,
                                                   const T* __restrict__ h, int64_t ldh,
                                                   T* __restrict__ y, int64_t ldy)
{
    constexpr bool by_step = Layout == hessenberg_layout::row_per_step;
    for (int64_t i = m - 1; i >= 0; --i) {
        T temp = rnc[i * ld_rnc + k];
        for (int64_t j = i + 1; j < m; ++j) {
            temp -= (by_step ? h[j * ldh + i * cols + k] : h[i * ldh + j * cols + k]) * y[j * ldy + k];
        }
        y[i * ldy + k] = temp / h[i * ldh + i * cols + k];  // the diagonal: either layout
    }
}

}  // namespace gkoc
