// The analysis behind the column-offset plan of csr_offsets.hpp: the kernels that build the per-segment tables and
// per-row masks of a (row_ptrs, col_idxs) pair and find the classes of equal segments.  Launched by offsets_build
// (csr_structure.hip), the only file that includes this header; the product kernel and the layout constants are
// in csr_offsets.hpp.
#pragma once
#include "csr_offsets.hpp"

namespace gkoc {

#ifdef __HIPCC__

// One wave per 64-row segment, lane = row.  Round by round the wave-minimum of the lanes' next unconsumed
// `col - row` is appended to the table; the lanes that hold it set their mask bit and advance.  A lane whose
// next offset is not above the last appended one has a row that is not strictly ascending; a 33rd offset or
// one outside int32 ends it as well (D = 0).
template <typename I>
__global__ __launch_bounds__(256) void csr_offsets_build_kernel(int64_t n_rows, const I* __restrict__ row_ptrs,
                                                                const I* __restrict__ cols,
                                                                int32_t* __restrict__ seg_tab,
                                                                uint32_t* __restrict__ row_mask)
{
    const int64_t seg = int64_t(blockIdx.x) * 4 + threadIdx.x / 64;
    const int lane = threadIdx.x % 64;
    if (seg * 64 >= n_rows) return;
    const int64_t row = seg * 64 + lane;
    const bool valid = row < n_rows;
    int64_t pos = valid ? int64_t(row_ptrs[row]) : 0;
    const int64_t end = valid ? int64_t(row_ptrs[row + 1]) : 0;
    constexpr long long NONE = 0x7fffffffffffffffll;
    uint32_t mask = 0;
    int D = 0;
    int32_t my_off = 0;
    bool ok = true;
    long long last = 0;
    for (;;) {
        const long long cur = pos < end ? (long long)(cols[pos]) - (long long)(row) : NONE;
        long long m = cur;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const long long t = __shfl_xor(m, o, 64);
            m = t < m ? t : m;
        }
        if (m == NONE) break;
        if (D == OFFS_MAX || (D > 0 && m <= last) || m < -2147483648ll || m > 2147483647ll) {
            ok = false;
            break;
        }
        if (lane == D) my_off = int32_t(m);
        if (cur == m) {
            mask |= 1u << D;
            ++pos;
        }
        last = m;
        ++D;
    }
    if (!ok) D = 0;
    if (lane == 0) seg_tab[seg * OFFS_TAB] = D;
    if (lane < OFFS_MAX) seg_tab[seg * OFFS_TAB + 1 + lane] = lane < D ? my_off : 0;
    if (valid) row_mask[row] = ok ? mask : 0u;
}

// One workgroup: skip[w] = bit per segment "eligible" (| the long-row flags of csr_long_rows.hpp: what the
// row-segment kernel leaves out when it runs beside this kernel), count[0] = eligible segments, count[1] = the
// largest D of the plan (the launcher picks the product kernel's number of diagonal slots by it).
__global__ __launch_bounds__(1024) void csr_offsets_finish_kernel(int64_t n_seg, const int32_t* __restrict__ seg_tab,
                                                                  const uint32_t* __restrict__ long_bits,
                                                                  uint32_t* __restrict__ skip,
                                                                  unsigned long long* __restrict__ count)
{
    __shared__ long long part[16];
    __shared__ int d_max;
    if (threadIdx.x == 0) d_max = 0;
    __syncthreads();
    const int64_t n_words = (n_seg + 31) / 32;
    long long mine = 0;
    int my_d = 0;
    for (int64_t w = threadIdx.x; w < n_words; w += 1024) {
        uint32_t bits = 0;
        for (int j = 0; j < 32; ++j) {
            const int64_t s = w * 32 + j;
            const int D = s < n_seg ? seg_tab[s * OFFS_TAB] : 0;
            if (D > 0) bits |= 1u << j;
            my_d = D > my_d ? D : my_d;
        }
        mine += __popc(bits);
        skip[w] = long_bits != nullptr ? (bits | long_bits[w]) : bits;
    }
    atomicMax(&d_max, my_d);
    const long long total = block_sum<1024>(mine, part);
    __syncthreads();
    if (threadIdx.x == 0) {
        count[0] = static_cast<unsigned long long>(total);
        count[1] = static_cast<unsigned long long>(d_max);
    }
}

// ---- classes of equal segments ------------------------------------------------------------------------------
// The class key of a segment: word w < 64 is the mask of row 64 seg + w (0 at or behind n_rows), word 64 + j the
// j-th table word.  Lane l holds words l and (l < OFFS_TAB) 64 + l.
struct class_words {
    uint32_t mask, tab;
};
__device__ __forceinline__ class_words class_words_of(int64_t n_rows, int64_t seg, int lane,
                                                      const int32_t* __restrict__ seg_tab,
                                                      const uint32_t* __restrict__ row_mask)
{
    const int64_t row = seg * 64 + lane;
    class_words w;
    w.mask = row < n_rows ? row_mask[row] : 0u;
    w.tab = lane < OFFS_TAB ? uint32_t(seg_tab[seg * OFFS_TAB + lane]) : 0u;
    return w;
}

__device__ __forceinline__ unsigned long long class_mix(unsigned long long z)      // (the splitmix64 finalizer)
{
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// One wave per segment: hash[seg] = the sum over the 97 key words of mix(position, word), cut to the bits of
// `keep` (all of them; fewer only to provoke collisions: GKOC_TUNE_CSR_OFFSETS_HASH_BITS), ids[seg] = seg.
__global__ __launch_bounds__(256) void csr_offsets_hash_kernel(int64_t n_rows, int64_t n_seg,
                                                               const int32_t* __restrict__ seg_tab,
                                                               const uint32_t* __restrict__ row_mask,
                                                               unsigned long long keep,
                                                               unsigned long long* __restrict__ hash,
                                                               uint32_t* __restrict__ ids)
{
    const int64_t seg = int64_t(blockIdx.x) * 4 + threadIdx.x / 64;
    const int lane = threadIdx.x % 64;
    if (seg >= n_seg) return;
    const class_words w = class_words_of(n_rows, seg, lane, seg_tab, row_mask);
    unsigned long long h = class_mix((static_cast<unsigned long long>(lane) << 32) | w.mask);
    if (lane < OFFS_TAB) h += class_mix((static_cast<unsigned long long>(64 + lane) << 32) | w.tab);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) h += __shfl_xor(h, o, 64);
    if (lane == 0) {
        hash[seg] = h & keep;
        ids[seg] = uint32_t(seg);
    }
}

// One wave per position i of the sorted (hash, segment) pairs.  The leader of i is the first position that holds
// the same hash (a binary search; the sort is stable, so the leader is the run's lowest segment).  is_new[i] = 1
// where the segment opens a class: it is the leader, or one of its 97 words differs from the leader's.
__global__ __launch_bounds__(256) void csr_offsets_leader_kernel(int64_t n_rows, int64_t n_seg,
                                                                 const int32_t* __restrict__ seg_tab,
                                                                 const uint32_t* __restrict__ row_mask,
                                                                 const unsigned long long* __restrict__ hash_sorted,
                                                                 const uint32_t* __restrict__ ids_sorted,
                                                                 uint32_t* __restrict__ leader,
                                                                 uint32_t* __restrict__ is_new)
{
    const int64_t i = int64_t(blockIdx.x) * 4 + threadIdx.x / 64;
    const int lane = threadIdx.x % 64;
    if (i >= n_seg) return;
    const unsigned long long h = hash_sorted[i];
    int64_t lo = 0, hi = i;
    while (lo < hi) {
        const int64_t mid = (lo + hi) / 2;
        if (hash_sorted[mid] < h) {
            lo = mid + 1;
        } else {
            hi = mid;
        }
    }
    bool same = true;
    if (lo != i) {
        const class_words a = class_words_of(n_rows, int64_t(ids_sorted[i]), lane, seg_tab, row_mask);
        const class_words b = class_words_of(n_rows, int64_t(ids_sorted[lo]), lane, seg_tab, row_mask);
        same = __all(a.mask == b.mask && a.tab == b.tab) != 0;
    }
    if (lane == 0) {
        leader[i] = uint32_t(lo);
        is_new[i] = (lo == i || !same) ? 1u : 0u;
    }
}

// count[2] = the number of classes, from the exclusive scan of is_new over the sorted order (class_at); count[3] =
// the number of stored entries (the launcher sizes the product by it)
__global__ void csr_offsets_class_count_kernel(int64_t n_seg, const uint32_t* __restrict__ is_new,
                                               const uint32_t* __restrict__ class_at, int64_t n_rows,
                                               const int32_t* __restrict__ row_ptrs,
                                               unsigned long long* __restrict__ count)
{
    count[2] = static_cast<unsigned long long>(class_at[n_seg - 1]) + is_new[n_seg - 1];
    const int32_t nnz = row_ptrs[n_rows];
    count[3] = nnz > 0 ? static_cast<unsigned long long>(nnz) : 0ull;
}

// One wave per sorted position: the segment's class id - its own where it opens a class, its leader's otherwise -
// and, where it opens one, the class' table and masks.
__global__ __launch_bounds__(256) void csr_offsets_compact_kernel(int64_t n_rows, int64_t n_seg,
                                                                  const int32_t* __restrict__ seg_tab,
                                                                  const uint32_t* __restrict__ row_mask,
                                                                  const uint32_t* __restrict__ ids_sorted,
                                                                  const uint32_t* __restrict__ leader,
                                                                  const uint32_t* __restrict__ is_new,
                                                                  const uint32_t* __restrict__ class_at,
                                                                  int32_t* __restrict__ seg_class,
                                                                  int32_t* __restrict__ cls_tab,
                                                                  uint32_t* __restrict__ cls_mask)
{
    const int64_t i = int64_t(blockIdx.x) * 4 + threadIdx.x / 64;
    const int lane = threadIdx.x % 64;
    if (i >= n_seg) return;
    const int64_t seg = int64_t(ids_sorted[i]);
    const bool opens = is_new[i] != 0;
    const int64_t cid = int64_t(opens ? class_at[i] : class_at[leader[i]]);
    if (lane == 0) seg_class[seg] = int32_t(cid);
    if (opens) {
        const class_words w = class_words_of(n_rows, seg, lane, seg_tab, row_mask);
        cls_mask[cid * 64 + lane] = w.mask;
        if (lane < OFFS_TAB) cls_tab[cid * OFFS_TAB + lane] = int32_t(w.tab);
    }
}

#endif  // __HIPCC__

}  // namespace gkoc
