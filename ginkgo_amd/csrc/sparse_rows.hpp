// What the set-up kernels that give a group of lanes a row of a sparse matrix share (trs.hip, factorization.hip,
// par_factorization.hip, par_ilut.hip, symbolic.hip, isai.hip, pgm.hip): the column search, reductions over a
// group of lanes, the checking pass that locates the diagonals, the status words a check reports through, and
// the export of a table of row-length limits.  The lanes-per-row choice and the grids are in launch_shape.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>

#include "common.hpp"

namespace gkoc {
namespace {

// the row-length limits of the lanes-per-row choice of the factorizations (exact, sweeps, threshold)
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
__device__ __forceinline__ bool is_finite(double v) { return ::isfinite(v); }
__device__ __forceinline__ bool is_finite(float v) { return ::isfinite(v); }

// ---- over the group of W lanes this lane belongs to, the result in every lane of the group ----
template <int W, typename T>
__device__ __forceinline__ T group_sum(T v)
{
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, W);
    return v;
}

template <int W>
__device__ __forceinline__ int group_any(int flag)
{
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) {
        flag |= __shfl_xor(flag, off, W);
    }
    return flag;
}

template <int W, typename T>
__device__ __forceinline__ T group_max(T v)
{
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) {
        const T o = __shfl_xor(v, off, W);
        v = o > v ? o : v;
    }
    return v;
}

// the tail of a check kernel: the longest row that a lane of this wave saw, into the status word
__device__ __forceinline__ void note_longest(int longest, int* __restrict__ word)
{
    longest = wave_max(longest);
    if ((threadIdx.x & (wave_size - 1)) == 0 && longest > 0) atomicMax(word, longest);
}

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
    note_longest(longest, &status[3]);
}

// N zeroed status words in stream-ordered scratch, and behind them (on a 16-byte boundary) whatever else the
// entry keeps there for as long as the words live.  The kernels of a check write the words through dev;
// read() brings all of them to the host in one copy and synchronises the stream.
template <int N>
struct status_words {
    static constexpr size_t bytes = (sizeof(int) * N + 15) / 16 * 16;
    hipStream_t st;
    int* dev = nullptr;
    int host[N] = {};

    explicit status_words(hipStream_t stream) : st{stream} {}
    status_words(const status_words&) = delete;
    status_words& operator=(const status_words&) = delete;
    ~status_words()
    {
        if (dev) (void)scratch_free(st, dev);
    }

    int init(size_t bytes_behind = 0)
    {
        void* raw = nullptr;
        GKOC_TRY(scratch_malloc(st, &raw, bytes + bytes_behind));
        dev = static_cast<int*>(raw);
        GKOC_HIP(hipMemsetAsync(dev, 0, bytes, st));
        return GKOC_OK;
    }
    template <typename U>
    U* behind() const
    {
        return reinterpret_cast<U*>(reinterpret_cast<char*>(dev) + bytes);
    }
    int read()
    {
        GKOC_HIP(hipMemcpyAsync(host, dev, sizeof(int) * N, hipMemcpyDeviceToHost, st));
        GKOC_HIP(hipStreamSynchronize(st));
        return GKOC_OK;
    }
    int operator[](int word) const { return host[word]; }
};

// the body of a gkoc_*_row_limits entry
template <size_t N>
int export_row_limits(const int (&limits)[N], int* limits_host, int* count_host)
{
    GKOC_REQUIRE(limits_host && count_host, GKOC_E_INVALID, "null pointer");
    for (size_t p = 0; p < N; ++p) limits_host[p] = limits[p];
    *count_host = int(N);
    return GKOC_OK;
}

}  // namespace
}  // namespace gkoc
