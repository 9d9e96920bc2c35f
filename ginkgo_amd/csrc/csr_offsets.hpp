// CSR SpMV through cached per-segment column offsets (csr::spmv / advanced_spmv, one right-hand side).
//
// In a stencil or banded matrix `col - row` takes a few values only.  If the rows of a 64-row segment have
// strictly ascending columns and the union of their `col - row` has at most 32 values off_0 < off_1 < ...,
// then an entry's diagonal slot d says where it is stored (ascending d = storage order), so
//   * the segment's column indices need not be read at all (8 instead of 12 bytes per entry for double);
//   * x[row + off_d] for the 64 neighbouring rows of a segment is ONE contiguous 512-byte load instead of 64
//     gathered 8-byte accesses (the row-segment kernel of csr_spmv_pipe.hpp runs the vector L1 at its
//     access-rate ceiling with those).
// The PLAN - per segment the number of offsets D (0: not eligible) and the offsets, per row a 32-bit
// presence mask (bit d: the row stores an entry at column row + off_d) - describes (row_ptrs, col_idxs)
// alone and is built once per structure by csr_offsets_build_kernel; the launcher (csr_spmv.hip) keeps it,
// keyed by the two arrays, and drops it when either is freed or written.  The VALUES are read live by every
// product.  Segments that are not eligible (unsorted rows, duplicate columns, more than 32 offsets) stay
// with the row-segment kernel.
//
// csr_spmv_pipe3_kernel_offsets: a wave owns the segments the row-segment kernel's wave would own.  Per segment
// (a resident group of 64 rows; 32-row groups with an 8 KB stage were measured 2.8 x slower, docs/KERNELS.md 36):
//   * the group's values are streamed exactly like there - 16-byte loads per lane, contiguous per wave, all
//     of a group in flight at once - and parked in LDS AS VALUES (the whole group is resident before its row
//     phase: at most 64 x 32 entries, so no lane needs resume state);
//   * the loads of the NEXT group's values are issued as soon as the registers are free, i.e. before the
//     row phase of this one, and all x loads of this group before them (vmcnt is in-order: an x load issued
//     behind the value loads would be waited for behind them);
//   * row phase, lane = row: for d = 0 .. D-1 (compile-time index, wave-uniform exit in steps of 8) the load
//     of x[clamp(row + off_d)] is unconditional and in bounds, the value of an absent slot is never used:
//     sum += v * x only where bit d of the mask is set, separate multiply and add, ascending d = storage
//     order - the operations of the sequential reference in its order, hence its bits; an absent slot
//     contributes NOTHING (not 0 * x: an Inf / NaN in x or a signed zero would change bits).
// No atomics, no waiting between workgroups.
#pragma once
#include "common.hpp"
#include <type_traits>

namespace gkoc {

constexpr int OFFS_MAX = 32;                 // offsets per segment = bits of a row's mask
constexpr int OFFS_TAB = OFFS_MAX + 1;       // int32 per segment: D, off_0 .. off_31

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
// row-segment kernel leaves out when it runs beside this kernel), *count = eligible segments.
__global__ __launch_bounds__(1024) void csr_offsets_finish_kernel(int64_t n_seg, const int32_t* __restrict__ seg_tab,
                                                                  const uint32_t* __restrict__ long_bits,
                                                                  uint32_t* __restrict__ skip,
                                                                  unsigned long long* __restrict__ count)
{
    __shared__ long long part[16];
    const int64_t n_words = (n_seg + 31) / 32;
    long long mine = 0;
    for (int64_t w = threadIdx.x; w < n_words; w += 1024) {
        uint32_t bits = 0;
        for (int j = 0; j < 32; ++j) {
            const int64_t s = w * 32 + j;
            if (s < n_seg && seg_tab[s * OFFS_TAB] > 0) bits |= 1u << j;
        }
        mine += __popc(bits);
        skip[w] = long_bits != nullptr ? (bits | long_bits[w]) : bits;
    }
    const long long total = block_sum<1024>(mine, part);
    if (threadIdx.x == 0) *count = static_cast<unsigned long long>(total);
}

// T = double / float, 32-bit indices.  ADV: c = alpha A x + beta c.  DOT: also this wave's part of <x, c>
// (gkoc_x_csr_spmv_dot_*; the same lane-to-row assignment, per-wave butterfly and slot as the row-segment
// kernel, so the folded value has the same bits).
template <typename T, bool ADV, bool DOT>
__global__ __launch_bounds__(64, 2) void csr_spmv_pipe3_kernel_offsets(
    int32_t n_rows, int32_t n_cols, int64_t n_segments, int spw, const int32_t* __restrict__ row_ptrs,
    const T* __restrict__ vals, const T* __restrict__ x, T* __restrict__ c, const T* __restrict__ alpha_p,
    const T* __restrict__ beta_p, const int32_t* __restrict__ seg_tab, const uint32_t* __restrict__ row_mask,
    T* __restrict__ dot_partial)
{
    constexpr int GR = 64;                             // rows of a resident group = the segment
    constexpr int E = 16 / sizeof(T);                  // entries per lane and load
    constexpr int CAP = GR * OFFS_MAX;                 // entries of a group at most
    constexpr int NL = CAP / (64 * E) + 1;             // loads per lane: the stream starts up to E - 1 entries early
    constexpr int GPS = 64 / GR;                       // groups per segment
    // (a native vector type: an array of structs of this size is not kept in registers by the compiler)
    typedef T VT __attribute__((ext_vector_type(E)));
    __shared__ __attribute__((aligned(16))) T stage[CAP + E];

    const int lane = threadIdx.x;
    const int64_t wave_id = blockIdx.x;
    const int64_t sb = wave_id * spw;
    const int n_units = int((sb + spw < n_segments ? int64_t(spw) : n_segments - sb)) * GPS;
    T alpha = T(1), beta = T(0);
    if (ADV) {
        alpha = alpha_p[0];
        beta = beta_p[0];
    }
    T dot_acc = T(0);

    // what the wave knows about a group before it streams it: wave-uniform, read with scalar loads (which the
    // vector loads in flight do not wait for)
    struct unit {
        int D;          // 0: nothing to do (segment not eligible, or no rows)
        int row0;
        int k0a, len;   // aligned stream start; entries from there to the group's end (0: none)
        const int32_t* tab;
    };
    auto unit_of = [&](int u) {
        unit q;
        const int64_t s = sb + u / GPS;
        q.row0 = int(s * 64) + (u % GPS) * GR;
        q.tab = seg_tab + s * OFFS_TAB;
        q.D = (u < n_units && q.row0 < n_rows) ? q.tab[0] : 0;
        q.k0a = q.len = 0;
        if (q.D > 0) {
            const int last = q.row0 + GR < n_rows ? q.row0 + GR : n_rows;
            const int k0 = row_ptrs[q.row0];
            const int k1 = row_ptrs[last];
            q.k0a = k0 & ~(E - 1);
            q.len = k1 > k0 ? k1 - q.k0a : 0;
            // (a structure rewritten behind the plan's back must not write outside the stage)
            if (q.len > CAP + E - 1) q.len = CAP + E - 1;
        }
        return q;
    };
    // Every load is unconditional: a lane behind the group's end reads the 16 bytes that hold the group's last
    // entry again (inside the array; one access for all such lanes), and what it reads is not stored.
    VT v[NL];
    auto load_vals = [&](const unit& q) {
        const int last_chunk = (q.len - 1) & ~(E - 1);
#pragma unroll
        for (int t = 0; t < NL; ++t) {
            const int k = (t * 64 + lane) * E;
            v[t] = *reinterpret_cast<const VT*>(vals + (int64_t(q.k0a) + (k < last_chunk ? k : last_chunk)));
        }
    };
    // one group; ND = 8 or 32 diagonal slots (compile-time indices: x and the values stay in registers)
    auto group = [&](auto nd_c, const unit& cur, const unit& nxt, int u) {
        constexpr int ND = decltype(nd_c)::value;
        const int row = cur.row0 + lane;
        const bool valid = lane < GR && row < n_rows;
        const int last = cur.row0 + GR < n_rows ? cur.row0 + GR : n_rows;
        const int rs = row_ptrs[valid ? row : last] - cur.k0a;
        uint32_t mask = row_mask[valid ? row : cur.row0];
        if (!valid) mask = 0u;
        T sum = T(0), bdot = T(0);
        if (ADV && beta != T(0)) sum = c[valid ? row : cur.row0] * beta;
        if (DOT) bdot = x[valid ? row : cur.row0];
        // clamp(row + off_d): the column itself for a stored entry, anything in bounds for an absent slot
        // (the sum wraps for those at worst)
        const int ncm1 = n_cols - 1;
        T xv[ND];
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const int idx = int(uint32_t(row) + uint32_t(cur.tab[1 + d]));
            xv[d] = x[idx < 0 ? 0 : (idx > ncm1 ? ncm1 : idx)];
        }
        if (cur.len > 0) {
#pragma unroll
            for (int t = 0; t < NL; ++t) {
                const int k = (t * 64 + lane) * E;
                if (k < cur.len) *reinterpret_cast<VT*>(&stage[k]) = v[t];
            }
        }
        wave_lds_sync();
        // the registers are free: the next group's values are under way during this group's row phase
        if (nxt.D > 0 && nxt.len > 0) load_vals(nxt);
#pragma unroll
        for (int d0 = 0; d0 < ND; d0 += 8) {
            T val[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                // entries of the row in front of slot d = stored slots below d
                const int pos = rs + __popc(mask & ((1u << (d0 + i)) - 1u));
                val[i] = stage[pos];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                // (keeps the eight LDS reads together in front of the arithmetic)
                asm volatile("" : "+v"(val[i]));
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const T pr = ADV ? (alpha * val[i]) * xv[d0 + i] : val[i] * xv[d0 + i];
                sum = ((mask >> (d0 + i)) & 1u) != 0 ? sum + pr : sum;
            }
        }
        if (valid) c[row] = sum;
        if constexpr (DOT) {
            // (the row-segment kernel's lane for this row is row % 64 too)
            const T term = bdot * sum;
            if (valid) dot_acc += term;
        }
        wave_lds_sync();
    };

    unit cur = unit_of(0);
    if (cur.D > 0 && cur.len > 0) load_vals(cur);
    for (int u = 0; u < n_units; ++u) {
        const unit nxt = unit_of(u + 1);
        if (cur.D > 8) {
            group(std::integral_constant<int, OFFS_MAX>{}, cur, nxt, u);
        } else if (cur.D > 0) {
            group(std::integral_constant<int, 8>{}, cur, nxt, u);
        } else if (nxt.D > 0 && nxt.len > 0) {
            load_vals(nxt);
        }
        cur = nxt;
    }
    if constexpr (DOT) {
        dot_acc = wave_sum(dot_acc);
        if (lane == 0) dot_partial[wave_id] = dot_acc;
    }
}

#endif  // __HIPCC__

}  // namespace gkoc
