// What the exact factorizations (factorization.hip) and the fixed-point sweeps (par_factorization.hip) share:
// the row-length limits of the lanes-per-row choice, the column search, and the checking pass that locates the
// diagonals.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>

#include "common.hpp"

namespace gkoc {
namespace {

constexpr int fact_row_limits[] = {16, 32, 64};

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

__device__ __forceinline__ double root_of(double v) { return ::sqrt(v); }
__device__ __forceinline__ float root_of(float v) { return ::sqrtf(v); }

// status[0]: row pointers or columns out of range, [1]: a row without a diagonal, [2]: a diagonal that is not
// the last entry of its row, [3]: the longest row.  diag[row] = position of the diagonal (-1 without one).
template <typename I>
__global__ __launch_bounds__(256) void locate_diagonals_kernel(int64_t n, int64_t nnz,
                                                               const I* __restrict__ rp,
                                                               const I* __restrict__ ci, I* __restrict__ diag,
                                                               int* __restrict__ status)
{
    const int64_t stride = int64_t(gridDim.x) * 256;
    int longest = 0;
    for (int64_t row = int64_t(blockIdx.x) * 256 + threadIdx.x; row < n; row += stride) {
        const int64_t begin = rp[row], end = rp[row + 1];
        int64_t pos = -1;
        if (begin < 0 || end < begin || end > nnz || (row == 0 && begin != 0) || (row == n - 1 && end != nnz)) {
            status[0] = 1;
        } else {
            for (int64_t k = begin; k < end; ++k) {
                const int64_t col = ci[k];
                if (col < 0 || col >= n) status[0] = 1;
                if (col == row && pos < 0) pos = k;
            }
            if (pos < 0) {
                status[1] = 1;
            } else if (pos != end - 1) {
                status[2] = 1;
            }
            const int64_t len = end - begin;
            longest = len > longest ? int(len > INT_MAX ? INT_MAX : len) : longest;
        }
        diag[row] = I(pos);
    }
    longest = wave_max(longest);
    if ((threadIdx.x & (wave_size - 1)) == 0 && longest > 0) atomicMax(&status[3], longest);
}

struct scratch_guard {
    hipStream_t st;
    void* ptr;
    ~scratch_guard()
    {
        if (ptr) (void)scratch_free(st, ptr);
    }
};

}  // namespace
}  // namespace gkoc
