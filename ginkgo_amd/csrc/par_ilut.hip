// Threshold ILU / IC by fixed-point sweeps (factorization::ParIlut / ParIct; Anzt, Chow, Dongarra, "ParILUT - a
// new parallel threshold ILU factorization", SIAM J. Sci. Comput. 40, 2018): what one iteration needs on top of
// the sweeps of par_factorization.hip and the triplet pipeline.
//   par_ilut_gather                                  values of a sorted matrix at the positions of a pattern
//   par_ilut_candidate_values / par_ict_...          the factor's values, and the residual-based start values
//                                                    of the candidates, on the pattern of L U (L L^T) + A
//   par_ilut_threshold_select                        the exact magnitude of a given rank among the strictly-lower
//                                                    (-upper) entries: radix select, result on the device
//   par_ilut_keep_mask                               1 / 0 per entry from the thresholds
//
// Contract: include/gko_cdna4.h (-ffp-contract=off keeps multiply and subtract apart).  Every entry writes
// VALUES (a T array), the threshold (one T) or its opaque work buffer; no entry writes an index array: the new
// patterns are made by the triplet pipeline from the mask.
//
// Kernels.  gather, candidate_values, keep_mask and the select's histogram pass share one layout: a group of W
// lanes takes a row of the pattern, lane = position, rows spread over the grid; a row longer than W is streamed
// by its group in rounds of W positions.  W is 16, 32 or 64 from the longest row at the limits of the
// factorization kernels for candidate_values (whose lanes walk a row of the factor each) and 16 for the plain
// streaming kernels.  A position depends on no other position: every output is written by exactly one lane, no
// shuffles, no atomics on values.  A candidate walks row i of the factor in storage order = ascending k, so its
// subtractions come in the stated order; it stops at the first k >= min(i, j).
// threshold_select is a most-significant-digit radix select over u(v) = the bits of |v|: per pass one streaming
// read that counts the next 8 bits of the entries whose higher bits equal the prefix found so far (256 bins per
// workgroup in LDS, merged into the pass' global table by integer atomics - order independent, the only atomics)
// and one single-workgroup kernel that narrows prefix and rank.  Passes are separated by kernel boundaries, no
// kernel waits for another workgroup, nothing is read back: the entry does not synchronise.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "sparse_rows.hpp"

namespace gkoc {
namespace {

constexpr int ilut_block = 256;
constexpr int stream_lanes = 16;

template <typename T>
struct bits_of;
template <>
struct bits_of<double> {
    using type = unsigned long long;
    static constexpr int passes = 8;
    static __device__ __forceinline__ type magnitude(double v)
    {
        return static_cast<type>(__double_as_longlong(v)) & 0x7fffffffffffffffULL;
    }
    static __device__ __forceinline__ double value(type u) { return __longlong_as_double(static_cast<long long>(u)); }
};
template <>
struct bits_of<float> {
    using type = unsigned int;
    static constexpr int passes = 4;
    static __device__ __forceinline__ type magnitude(float v)
    {
        return static_cast<type>(__float_as_int(v)) & 0x7fffffffU;
    }
    static __device__ __forceinline__ float value(type u) { return __int_as_float(static_cast<int>(u)); }
};

// ---------------------------------------------------------------------------------------------- gather
template <typename T, typename I>
__global__ __launch_bounds__(ilut_block) void gather_kernel(int64_t n, const I* __restrict__ p_rp,
                                                            const I* __restrict__ p_ci,
                                                            const I* __restrict__ s_rp,
                                                            const I* __restrict__ s_ci,
                                                            const T* __restrict__ s_v, T* __restrict__ out)
{
    constexpr int groups = ilut_block / stream_lanes;
    const int lane = threadIdx.x % stream_lanes;
    const int64_t stride = int64_t(gridDim.x) * groups;
    for (int64_t row = int64_t(blockIdx.x) * groups + threadIdx.x / stream_lanes; row < n; row += stride) {
        const int64_t lo = s_rp[row], hi = s_rp[row + 1];
        for (int64_t p = int64_t(p_rp[row]) + lane; p < int64_t(p_rp[row + 1]); p += stream_lanes) {
            const int64_t pos = find_column(s_ci, lo, hi, int64_t(p_ci[p]));
            out[p] = pos >= 0 ? s_v[pos] : T(0);
        }
    }
}

// status[0] = 1 if some row of the pattern lacks a column that the same row of m stores
template <typename I>
__global__ __launch_bounds__(ilut_block) void contains_kernel(int64_t n, const I* __restrict__ p_rp,
                                                              const I* __restrict__ p_ci,
                                                              const I* __restrict__ m_rp,
                                                              const I* __restrict__ m_ci, int* __restrict__ status)
{
    constexpr int groups = ilut_block / stream_lanes;
    const int lane = threadIdx.x % stream_lanes;
    const int64_t stride = int64_t(gridDim.x) * groups;
    for (int64_t row = int64_t(blockIdx.x) * groups + threadIdx.x / stream_lanes; row < n; row += stride) {
        const int64_t lo = p_rp[row], hi = p_rp[row + 1];
        for (int64_t q = int64_t(m_rp[row]) + lane; q < int64_t(m_rp[row + 1]); q += stream_lanes) {
            if (find_column(p_ci, lo, hi, int64_t(m_ci[q])) < 0) status[0] = 1;
        }
    }
}

// ---------------------------------------------------------------------------------------------- candidates
// the value at position (row, col) of the pattern.  m_diag[k]: position of the diagonal of row k of m.
template <bool IC, typename T, typename I>
__device__ __forceinline__ T candidate(int64_t row, int64_t col, const I* __restrict__ a_rp,
                                       const I* __restrict__ a_ci, const T* __restrict__ a_v,
                                       const I* __restrict__ m_rp, const I* __restrict__ m_ci,
                                       const T* __restrict__ m_v, const I* __restrict__ m_diag)
{
    const int64_t m_lo = m_rp[row], m_hi = m_rp[row + 1];
    const int64_t own = find_column(m_ci, m_lo, m_hi, col);
    if (own >= 0) return m_v[own];
    const int64_t in_a = find_column(a_ci, int64_t(a_rp[row]), int64_t(a_rp[row + 1]), col);
    T s = in_a >= 0 ? a_v[in_a] : T(0);
    const int64_t bound = col < row ? col : row;
    // ILU: (k, col) right of the diagonal of row k.  IC: (col, k) left of the diagonal of row col.
    const int64_t ic_lo = IC ? int64_t(m_rp[col]) : 0, ic_hi = IC ? int64_t(m_diag[col]) : 0;
    for (int64_t q = m_lo; q < m_hi; ++q) {
        const int64_t k = m_ci[q];
        if (k >= bound) break;
        const int64_t pos = IC ? find_column(m_ci, ic_lo, ic_hi, k)
                               : find_column(m_ci, int64_t(m_diag[k]) + 1, int64_t(m_rp[k + 1]), col);
        if (pos >= 0) s = s - m_v[q] * m_v[pos];
    }
    return col < row ? s / m_v[m_diag[col]] : s;
}

template <bool IC, int W, typename T, typename I>
__global__ __launch_bounds__(ilut_block) void candidate_kernel(int64_t n, const I* __restrict__ p_rp,
                                                               const I* __restrict__ p_ci,
                                                               const I* __restrict__ a_rp,
                                                               const I* __restrict__ a_ci,
                                                               const T* __restrict__ a_v,
                                                               const I* __restrict__ m_rp,
                                                               const I* __restrict__ m_ci,
                                                               const T* __restrict__ m_v,
                                                               const I* __restrict__ m_diag, T* __restrict__ out)
{
    constexpr int groups = ilut_block / W;
    const int lane = threadIdx.x % W;
    const int64_t stride = int64_t(gridDim.x) * groups;
    for (int64_t row = int64_t(blockIdx.x) * groups + threadIdx.x / W; row < n; row += stride) {
        // one round for a row of at most W positions; a longer one (W is 64 then) is streamed
        for (int64_t p = int64_t(p_rp[row]) + lane; p < int64_t(p_rp[row + 1]); p += W) {
            out[p] = candidate<IC, T, I>(row, int64_t(p_ci[p]), a_rp, a_ci, a_v, m_rp, m_ci, m_v, m_diag);
        }
    }
}

template <bool IC, int W, typename T, typename I>
int candidate_launch(hipStream_t st, int64_t n, const I* p_rp, const I* p_ci, const I* a_rp, const I* a_ci,
                     const T* a_v, const I* m_rp, const I* m_ci, const T* m_v, const I* m_diag, T* out)
{
    candidate_kernel<IC, W, T, I><<<dim3(stream_grid(n, ilut_block / W)), dim3(ilut_block), 0, st>>>(
        n, p_rp, p_ci, a_rp, a_ci, a_v, m_rp, m_ci, m_v, m_diag, out);
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

// the grid of the plain streaming kernels
inline unsigned stream_blocks(int64_t n) { return capped_grid(n, ilut_block / stream_lanes, max_stream_blocks); }

// the checking pass of the sweeps on one matrix: status (4 ints) and diag (n_rows entries) in scratch
template <typename I>
int locate(hipStream_t st, int64_t n, int64_t nnz, const I* rp, const I* ci, I* diag, int* status)
{
    locate_diagonals_kernel<I><<<dim3(stream_grid(n)), dim3(256), 0, st>>>(n, nnz, rp, ci, diag, status);
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

constexpr const char* bad_structure =
    "row pointers that do not ascend from 0 to nnz, or a column outside the matrix";

template <typename T, typename I>
int gather(gkoc_stream_t s, int64_t n, int64_t p_nnz, const I* p_rp, const I* p_ci, int64_t s_nnz,
           const I* s_rp, const I* s_ci, const T* s_v, T* out)
{
    GKOC_REQUIRE(n >= 0 && p_nnz >= 0 && s_nnz >= 0, GKOC_E_INVALID,
                 "negative number of rows or of stored entries");
    if (n == 0) return GKOC_OK;
    GKOC_REQUIRE(p_rp && s_rp && (p_ci || p_nnz == 0) && (out || p_nnz == 0) && ((s_ci && s_v) || s_nnz == 0),
                 GKOC_E_INVALID, "null pointer");
    hipStream_t st = as_stream(s);
    // scratch: 2 x 4 status words, then one array of diagonal positions that both checks write (not used)
    status_words<8> status(st);
    GKOC_TRY(status.init(sizeof(I) * size_t(n)));
    I* diag = status.template behind<I>();
    GKOC_TRY(locate(st, n, p_nnz, p_rp, p_ci, diag, status.dev));
    GKOC_TRY(locate(st, n, s_nnz, s_rp, s_ci, diag, status.dev + 4));
    GKOC_TRY(status.read());
    GKOC_REQUIRE(status[0] == 0 && status[4] == 0, GKOC_E_INVALID, bad_structure);
    if (p_nnz == 0) return GKOC_OK;
    gather_kernel<T, I><<<dim3(stream_blocks(n)), dim3(ilut_block), 0, st>>>(n, p_rp, p_ci, s_rp, s_ci, s_v, out);
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

template <bool IC, typename T, typename I>
int candidate_values(gkoc_stream_t s, int64_t n, int64_t p_nnz, const I* p_rp, const I* p_ci, int64_t a_nnz,
                     const I* a_rp, const I* a_ci, const T* a_v, int64_t m_nnz, const I* m_rp, const I* m_ci,
                     const T* m_v, T* out)
{
    GKOC_REQUIRE(n >= 0 && p_nnz >= 0 && a_nnz >= 0 && m_nnz >= 0, GKOC_E_INVALID,
                 "negative number of rows or of stored entries");
    if (n == 0) return GKOC_OK;
    GKOC_REQUIRE(p_nnz >= n && m_nnz >= n, GKOC_E_INVALID,
                 "fewer stored entries than rows: a row without a stored diagonal");
    GKOC_REQUIRE(p_rp && p_ci && a_rp && (a_nnz == 0 || (a_ci && a_v)) && m_rp && m_ci && m_v && out,
                 GKOC_E_INVALID, "null pointer");
    hipStream_t st = as_stream(s);
    // scratch: 4 x 4 status words (pattern, a, m, containment), the diagonal positions of m, and an array for
    // the positions of the other two, which nothing reads
    status_words<16> status(st);
    GKOC_TRY(status.init(2 * sizeof(I) * size_t(n)));
    I* m_diag = status.template behind<I>();
    I* unused = m_diag + n;
    GKOC_TRY(locate(st, n, p_nnz, p_rp, p_ci, unused, status.dev));
    GKOC_TRY(locate(st, n, a_nnz, a_rp, a_ci, unused, status.dev + 4));
    GKOC_TRY(locate(st, n, m_nnz, m_rp, m_ci, m_diag, status.dev + 8));
    GKOC_TRY(status.read());
    GKOC_REQUIRE(status[0] == 0 && status[4] == 0 && status[8] == 0, GKOC_E_INVALID, bad_structure);
    GKOC_REQUIRE(status[1] == 0 && status[9] == 0, GKOC_E_INVALID, "a row without a stored diagonal");
    GKOC_REQUIRE(!IC || (status[2] == 0 && status[10] == 0), GKOC_E_INVALID,
                 "a row whose last entry is not its diagonal");
    // the rows are valid now: the containment check may search them
    contains_kernel<I><<<dim3(stream_blocks(n)), dim3(ilut_block), 0, st>>>(n, p_rp, p_ci, m_rp, m_ci,
                                                                           status.dev + 12);
    GKOC_LAUNCH_OK();
    GKOC_TRY(status.read());
    GKOC_REQUIRE(status[12] == 0, GKOC_E_INVALID, "the pattern does not contain the pattern of the factor");
    return with_lanes(status[3], fact_row_limits, [&](auto w) {
        return candidate_launch<IC, decltype(w)::value, T, I>(st, n, p_rp, p_ci, a_rp, a_ci, a_v, m_rp, m_ci, m_v,
                                                              m_diag, out);
    });
}

// ---------------------------------------------------------------------------------------------- select
// work: select_state, then one table of 256 counts per pass
struct select_state {
    unsigned long long prefix;      // the digits found so far, as the high bits of u shifted down
    unsigned long long rank;        // 0-based ascending rank among the entries that carry the prefix
    unsigned long long done;        // != 0: the part has at most `keep` entries, the threshold is +0
    unsigned long long unused;
};
constexpr int max_passes = 8;
constexpr size_t select_bytes = sizeof(select_state) + size_t(max_passes) * 256 * sizeof(unsigned long long);

// pass `pass` (0 = the most significant 8 bits): counts digit `pass` of the entries of the part whose digits
// 0 .. pass-1 equal state->prefix
template <typename T, typename I>
__global__ __launch_bounds__(ilut_block) void select_count_kernel(int64_t n, const I* __restrict__ rp,
                                                                  const I* __restrict__ ci,
                                                                  const T* __restrict__ v, int part, int pass,
                                                                  const select_state* __restrict__ state,
                                                                  unsigned long long* __restrict__ table)
{
    using B = bits_of<T>;
    using U = typename B::type;
    __shared__ unsigned long long bins[256];
    if (state->done != 0) return;       // uniform over the grid: written by an earlier kernel
    bins[threadIdx.x] = 0;
    __syncthreads();
    constexpr int total_bits = 8 * B::passes;
    const int shift = total_bits - 8 * (pass + 1);
    const U prefix = static_cast<U>(state->prefix);
    constexpr int groups = ilut_block / stream_lanes;
    const int lane = threadIdx.x % stream_lanes;
    const int64_t stride = int64_t(gridDim.x) * groups;
    for (int64_t row = int64_t(blockIdx.x) * groups + threadIdx.x / stream_lanes; row < n; row += stride) {
        for (int64_t p = int64_t(rp[row]) + lane; p < int64_t(rp[row + 1]); p += stream_lanes) {
            const int64_t col = ci[p];
            if (part == 0 ? col < row : col > row) {
                const U u = B::magnitude(v[p]);
                // (u >> shift) >> 8 without a shift by the type's width in pass 0
                if (pass == 0 || ((u >> shift) >> 8) == prefix) {
                    atomicAdd(&bins[(u >> shift) & 0xff], 1ULL);
                }
            }
        }
    }
    __syncthreads();
    if (bins[threadIdx.x] != 0) atomicAdd(&table[threadIdx.x], bins[threadIdx.x]);
}

// one workgroup: from the table of pass `pass`, the digit that holds the rank; after the last pass the threshold
template <typename T>
__global__ __launch_bounds__(256) void select_narrow_kernel(int pass, unsigned long long keep,
                                                            select_state* __restrict__ state,
                                                            const unsigned long long* __restrict__ table,
                                                            T* __restrict__ threshold)
{
    using B = bits_of<T>;
    __shared__ unsigned long long counts[256];
    counts[threadIdx.x] = table[threadIdx.x];
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (state->done != 0) return;
    unsigned long long rank = state->rank;
    if (pass == 0) {
        unsigned long long count = 0;
        for (int d = 0; d < 256; ++d) count += counts[d];
        if (count <= keep) {
            state->done = 1;
            *threshold = T(0);
            return;
        }
        rank = count - keep;
    }
    int digit = 0;
    while (digit < 255 && rank >= counts[digit]) {
        rank -= counts[digit];
        ++digit;
    }
    const unsigned long long prefix = (state->prefix << 8) | static_cast<unsigned long long>(digit);
    state->prefix = prefix;
    state->rank = rank;
    if (pass == B::passes - 1) *threshold = B::value(static_cast<typename B::type>(prefix));
}

template <typename T, typename I>
int threshold_select(gkoc_stream_t s, int64_t n, const I* rp, const I* ci, const T* v, int part, int64_t keep,
                     void* work, size_t work_bytes, T* threshold)
{
    GKOC_REQUIRE(n >= 0, GKOC_E_INVALID, "negative number of rows");
    GKOC_REQUIRE(part == 0 || part == 1, GKOC_E_INVALID, "part is 0 (strictly lower) or 1 (strictly upper)");
    GKOC_REQUIRE(keep >= 1, GKOC_E_INVALID, "keep must be at least 1");
    GKOC_REQUIRE(threshold, GKOC_E_INVALID, "null pointer");
    hipStream_t st = as_stream(s);
    if (n == 0) {
        GKOC_HIP(hipMemsetAsync(threshold, 0, sizeof(T), st));
        return GKOC_OK;
    }
    GKOC_REQUIRE(rp && ci && v && work, GKOC_E_INVALID, "null pointer");
    GKOC_REQUIRE(work_bytes >= select_bytes && reinterpret_cast<uintptr_t>(work) % 8 == 0, GKOC_E_INVALID,
                 "the work buffer is smaller than gkoc_par_ilut_select_workspace_bytes or not 8-byte aligned");
    select_state* state = static_cast<select_state*>(work);
    unsigned long long* tables = reinterpret_cast<unsigned long long*>(state + 1);
    GKOC_HIP(hipMemsetAsync(work, 0, select_bytes, st));
    const unsigned blocks = stream_blocks(n);
    for (int pass = 0; pass < bits_of<T>::passes; ++pass) {
        select_count_kernel<T, I><<<dim3(blocks), dim3(ilut_block), 0, st>>>(n, rp, ci, v, part, pass, state,
                                                                             tables + 256 * pass);
        GKOC_LAUNCH_OK();
        select_narrow_kernel<T><<<dim3(1), dim3(256), 0, st>>>(pass, static_cast<unsigned long long>(keep), state,
                                                               tables + 256 * pass, threshold);
        GKOC_LAUNCH_OK();
    }
    return GKOC_OK;
}

// ---------------------------------------------------------------------------------------------- keep mask
template <typename T, typename I>
__global__ __launch_bounds__(ilut_block) void keep_mask_kernel(int64_t n, const I* __restrict__ rp,
                                                               const I* __restrict__ ci,
                                                               const T* __restrict__ v,
                                                               const T* __restrict__ thr_lower,
                                                               const T* __restrict__ thr_upper,
                                                               T* __restrict__ mask)
{
    using B = bits_of<T>;
    const auto lower = B::magnitude(*thr_lower);
    const auto upper = thr_upper ? B::magnitude(*thr_upper) : lower;
    constexpr int groups = ilut_block / stream_lanes;
    const int lane = threadIdx.x % stream_lanes;
    const int64_t stride = int64_t(gridDim.x) * groups;
    for (int64_t row = int64_t(blockIdx.x) * groups + threadIdx.x / stream_lanes; row < n; row += stride) {
        for (int64_t p = int64_t(rp[row]) + lane; p < int64_t(rp[row + 1]); p += stream_lanes) {
            const int64_t col = ci[p];
            bool keep = true;
            if (col < row) {
                keep = B::magnitude(v[p]) >= lower;
            } else if (col > row) {
                keep = thr_upper != nullptr && B::magnitude(v[p]) >= upper;
            }
            mask[p] = keep ? T(1) : T(0);
        }
    }
}

template <typename T, typename I>
int keep_mask(gkoc_stream_t s, int64_t n, int64_t nnz, const I* rp, const I* ci, const T* v, const T* thr_lower,
              const T* thr_upper, T* mask)
{
    GKOC_REQUIRE(n >= 0 && nnz >= 0, GKOC_E_INVALID, "negative number of rows or of stored entries");
    if (n == 0) return GKOC_OK;
    GKOC_REQUIRE(rp && thr_lower && (nnz == 0 || (ci && v && mask)), GKOC_E_INVALID, "null pointer");
    hipStream_t st = as_stream(s);
    // scratch: 4 status words, then the diagonal positions (not used)
    status_words<4> status(st);
    GKOC_TRY(status.init(sizeof(I) * size_t(n)));
    GKOC_TRY(locate(st, n, nnz, rp, ci, status.template behind<I>(), status.dev));
    GKOC_TRY(status.read());
    GKOC_REQUIRE(status[0] == 0, GKOC_E_INVALID, bad_structure);
    if (nnz == 0) return GKOC_OK;
    keep_mask_kernel<T, I><<<dim3(stream_blocks(n)), dim3(ilut_block), 0, st>>>(n, rp, ci, v, thr_lower, thr_upper,
                                                                               mask);
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

}  // namespace
}  // namespace gkoc

using namespace gkoc;

extern "C" size_t gkoc_par_ilut_select_workspace_bytes(void) { return select_bytes; }

#define GKOC_DEF_PAR_ILUT(T, TN, I, IN)                                                                        \
    extern "C" int gkoc_par_ilut_gather_##TN##_##IN(gkoc_stream_t s, int64_t n_rows, int64_t p_nnz,            \
                                                    const I* p_row_ptrs, const I* p_col_idxs, int64_t src_nnz, \
                                                    const I* src_row_ptrs, const I* src_col_idxs,              \
                                                    const T* src_vals, T* out_vals)                            \
    {                                                                                                          \
        return gather<T, I>(s, n_rows, p_nnz, p_row_ptrs, p_col_idxs, src_nnz, src_row_ptrs, src_col_idxs,     \
                            src_vals, out_vals);                                                               \
    }                                                                                                          \
    extern "C" int gkoc_par_ilut_candidate_values_##TN##_##IN(                                                 \
        gkoc_stream_t s, int64_t n_rows, int64_t p_nnz, const I* p_row_ptrs, const I* p_col_idxs,              \
        int64_t a_nnz, const I* a_row_ptrs, const I* a_col_idxs, const T* a_vals, int64_t m_nnz,               \
        const I* m_row_ptrs, const I* m_col_idxs, const T* m_vals, T* out_vals)                                \
    {                                                                                                          \
        return candidate_values<false, T, I>(s, n_rows, p_nnz, p_row_ptrs, p_col_idxs, a_nnz, a_row_ptrs,      \
                                             a_col_idxs, a_vals, m_nnz, m_row_ptrs, m_col_idxs, m_vals,        \
                                             out_vals);                                                        \
    }                                                                                                          \
    extern "C" int gkoc_par_ict_candidate_values_##TN##_##IN(                                                  \
        gkoc_stream_t s, int64_t n_rows, int64_t p_nnz, const I* p_row_ptrs, const I* p_col_idxs,              \
        int64_t a_nnz, const I* a_row_ptrs, const I* a_col_idxs, const T* a_vals, int64_t l_nnz,               \
        const I* l_row_ptrs, const I* l_col_idxs, const T* l_vals, T* out_vals)                                \
    {                                                                                                          \
        return candidate_values<true, T, I>(s, n_rows, p_nnz, p_row_ptrs, p_col_idxs, a_nnz, a_row_ptrs,       \
                                            a_col_idxs, a_vals, l_nnz, l_row_ptrs, l_col_idxs, l_vals,         \
                                            out_vals);                                                         \
    }                                                                                                          \
    extern "C" int gkoc_par_ilut_threshold_select_##TN##_##IN(gkoc_stream_t s, int64_t n_rows,                 \
                                                              const I* row_ptrs, const I* col_idxs,            \
                                                              const T* vals, int part, int64_t keep,           \
                                                              void* work, size_t work_bytes,                   \
                                                              T* threshold_dev)                                \
    {                                                                                                          \
        return threshold_select<T, I>(s, n_rows, row_ptrs, col_idxs, vals, part, keep, work, work_bytes,       \
                                      threshold_dev);                                                          \
    }                                                                                                          \
    extern "C" int gkoc_par_ilut_keep_mask_##TN##_##IN(gkoc_stream_t s, int64_t n_rows, int64_t nnz,           \
                                                       const I* row_ptrs, const I* col_idxs, const T* vals,    \
                                                       const T* thr_lower_dev, const T* thr_upper_dev,         \
                                                       T* mask)                                                \
    {                                                                                                          \
        return keep_mask<T, I>(s, n_rows, nnz, row_ptrs, col_idxs, vals, thr_lower_dev, thr_upper_dev, mask);  \
    }
GKOC_DEF_PAR_ILUT(double, f64, int32_t, i32)
GKOC_DEF_PAR_ILUT(double, f64, int64_t, i64)
GKOC_DEF_PAR_ILUT(float, f32, int32_t, i32)
GKOC_DEF_PAR_ILUT(float, f32, int64_t, i64)
