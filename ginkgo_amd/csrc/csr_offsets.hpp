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
// alone and is built once per structure by csr_offsets_build_kernel (csr_offsets_analysis.hpp); csr_structure.hip
// keeps it, keyed by the two arrays, and drops it when either is freed or written.  The VALUES are read live by
// every product.  Segments that are not eligible (unsorted rows, duplicate columns, more than 32 offsets) stay
// with the row-segment kernel.
// The plan is kept BY CLASS: two segments whose 33 table words (D, 32 zero-padded offsets) and 64 mask words (0
// for a row at or behind n_rows) are equal bit for bit share one entry of cls_tab / cls_mask, and a segment
// keeps its class id alone (seg_class, 4 bytes).  In a matrix from a structured mesh nearly every segment
// repeats another (the 27-point stencil 256^3: 27 classes among 262 144 segments), so a product streams 4 bytes a
// segment where the per-segment table and the per-row masks were 388, and the class tables stay in cache.  A
// structure without repetition has one class per segment: the same bytes plus the id.  The classes are found
// behind the build kernel (csr_offsets_hash_kernel .. csr_offsets_compact_kernel, same header): a 64-bit hash per
// segment, a stable sort of (hash, segment), the first segment of a run of equal hashes is its leader, and a
// member joins the leader's class only after comparing all 97 words with it - a hash collision costs a class of
// its own, never a wrong table.
//
// csr_spmv_pipe3_kernel_offsets: a wave owns the segments the row-segment kernel's wave would own.  Per segment
// (a resident group of 64 rows; 32-row groups with an 8 KB stage were measured 2.8 x slower, docs/KERNELS.md 36):
//   * the group's values are streamed exactly like there - 16-byte loads per lane, contiguous per wave, all
//     of a group in flight at once - and parked in LDS AS VALUES (the whole group is resident before its row
//     phase: at most 64 x ND entries, ND the kernel's number of diagonal slots, so no lane needs resume state);
//     the stream, the stage and the x loads are sized by ND: NL = ND / E + 1 loads of E = 16 / sizeof(T) entries
//     per lane (double 5 / 9 / 15 / 17 for ND = 8 / 16 / 28 / 32, float 3 / 5 / 8 / 9), NL x 64 x E entries of LDS
//     (double 5 / 9 / 15 / 17 KiB) - the 27-point stencil runs with 15 value and 28 x loads per lane, not 17 and 32;
//   * the loads of the NEXT group's values are issued as soon as the registers are free, i.e. before the
//     row phase of this one, and all x loads of this group before them (vmcnt is in-order: an x load issued
//     behind the value loads would be waited for behind them);
//   * row phase, lane = row: a row's entries start at the stream's lead plus the wave's exclusive prefix sum of
//     popc(mask) (one mask bit per stored entry: row_ptrs[row] is not read; the two ends of the group come from
//     scalar loads); for d = 0 .. ND-1 (compile-time index; ND = 8, 16, 28 or 32 slots per kernel) the load
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

// Exclusive prefix sum of v over the 64 lanes of a wave in six DPP steps: four shifts within the rows of 16
// lanes, then lane 15 of a row into the next row and lane 31 into the upper half.  A lane without a source keeps
// the 0 of `old`.  No LDS crossbar (ds_bpermute) and no index registers.
__device__ __forceinline__ int wave_exclusive_sum(int v)
{
    int s = v;
    s += __builtin_amdgcn_update_dpp(0, s, 0x111, 0xf, 0xf, false);   // row_shr:1
    s += __builtin_amdgcn_update_dpp(0, s, 0x112, 0xf, 0xf, false);   // row_shr:2
    s += __builtin_amdgcn_update_dpp(0, s, 0x114, 0xf, 0xf, false);   // row_shr:4
    s += __builtin_amdgcn_update_dpp(0, s, 0x118, 0xf, 0xf, false);   // row_shr:8
    s += __builtin_amdgcn_update_dpp(0, s, 0x142, 0xa, 0xf, false);   // row_bcast:15, rows 1 and 3
    s += __builtin_amdgcn_update_dpp(0, s, 0x143, 0xc, 0xf, false);   // row_bcast:31, rows 2 and 3
    return s - v;
}

// T = double / float, 32-bit indices.  ADV: c = alpha A x + beta c.  DOT: also this wave's part of <x, c>
// (gkoc_x_csr_spmv_dot_*; the same lane-to-row assignment, per-wave butterfly and slot as the row-segment
// kernel, so the folded value has the same bits).
//
// The schedule of a group, which the wait counts of the compiled kernel depend on (vmcnt retires in order; a
// load issued under a condition makes the compiler count at the join as if it had not been issued, and every
// later wait is then too strict by that many loads):
//   1. the group's mask and ND x loads, from offsets that are already in scalar registers - ND, the number of
//      diagonal slots, is the KERNEL's (8, 16, 28 or 32: the smallest that holds the plan's largest D, picked by
//      the launcher), not the segment's: a count that depended on the segment would be a condition again.  A
//      segment with fewer offsets has offset 0 and mask bit 0 in the slots it lacks: in-bounds loads that no sum
//      reads;
//   2. the scalar loads of the NEXT unit (row pointers; D and the offsets from its class' table, whose address
//      needs no load: the class ids of the wave's segments are in registers since the kernel's start): under way
//      while the values arrive;
//   3. the group's values, in flight since the previous group's step 4, go to the stage: all NL chunks of
//      every lane, no branch (entries at or behind `len` are never read: pos < len for every stored slot);
//   4. the NL value loads of the next group, ALWAYS issued, from ONE load site in the loop (and one in front
//      of it), so v[] has one register home and the compiler a static count of loads behind every x load;
//   5. the row phase: the prefix sum of the row lengths waits for the mask alone (vmcnt(NL + ND): the first load
//      of the group), the wait in front of the last x leaves the NL loads of step 4 in flight.
// Compiled for double, ND = 28: stage write vmcnt(43) .. (29) = the group's own 29 loads behind the values, row
// phase vmcnt(43) .. vmcnt(15), no vmcnt wait between the top of a group and its last x load; 155 VGPRs (fused
// dot 159), 15 KiB of LDS: 3 waves per SIMD by registers, 10 waves per CU by LDS (docs/KERNELS.md 36).
// "Always" because the loop runs over the groups that HAVE a successor; the wave's last group does 1 - 3 and 5
// behind it.  (Issuing step 4 there too, as re-reads of the group's last 16 bytes, was measured: with two
// segments per wave every second prefetch is then a dummy, and the kernel was 3.7 % slower than with the
// conditional prefetch it replaced, docs/KERNELS.md 36.)
// __launch_bounds__(64, 3) on the 28-slot kernels changes neither their registers nor, measurably, their time
// (docs/KERNELS.md 36): all instantiations keep (64, 2).
// NT: the value stream is loaded and c stored non-temporally (`global_load_dwordx4 ... nt`, counted by vmcnt like
// any load: the waits above are the same).  A value is used once per product, and with NT the stream does not
// pass through the L2 and Infinity Cache lines that serve the re-reads of x: -5 % on the 27-point stencil 256^3
// (3.6 GB of values).  A product whose bytes FIT the 256 MiB Infinity Cache is served from it call after call,
// and there NT costs 18 - 25 % (docs/KERNELS.md 36): the launcher sets it by the product's bytes.
template <typename T, bool ADV, bool DOT, int ND, bool NT>
__global__ __launch_bounds__(64, 2) void csr_spmv_pipe3_kernel_offsets(
    int32_t n_rows, int32_t n_cols, int64_t n_segments, int spw, const int32_t* __restrict__ row_ptrs,
    const T* __restrict__ vals, const T* __restrict__ x, T* __restrict__ c, const T* __restrict__ alpha_p,
    const T* __restrict__ beta_p, const int32_t* __restrict__ seg_class, const int32_t* __restrict__ cls_tab,
    const uint32_t* __restrict__ cls_mask, T* __restrict__ dot_partial)
{
    constexpr int GR = 64;                             // rows of a resident group = the segment
    constexpr int E = 16 / sizeof(T);                  // entries per lane and load
    constexpr int CAP = GR * ND;                       // entries of a group at most: D <= ND offsets a row
    constexpr int NL = CAP / (64 * E) + 1;             // loads per lane: the stream starts up to E - 1 entries early
    static_assert(ND >= 8 && ND <= OFFS_MAX && ND % 4 == 0, "bodies of eight slots and a last one of ND - 24");
    // (the stage takes a whole stream: `len` is clamped to CAP + E - 1 below)
    static_assert(NL * 64 * E >= CAP + E - 1, "stage too small");
    // (a native vector type: an array of structs of this size is not kept in registers by the compiler)
    typedef T VT __attribute__((ext_vector_type(E)));
    __shared__ __attribute__((aligned(16))) T stage[NL * 64 * E];

    const int lane = threadIdx.x;
    const int64_t wave_id = blockIdx.x;
    const int64_t sb = wave_id * spw;
    const int n_units = int(sb + spw < n_segments ? int64_t(spw) : n_segments - sb);
    T alpha = T(1), beta = T(0);
    if (ADV) {
        alpha = alpha_p[0];
        beta = beta_p[0];
    }
    T dot_acc = T(0);
    // The class ids of ALL the wave's segments (spw is 1 or 2: plan_segments), read up front: the address of a
    // class' table depends on its id, and with the ids in registers before the first unit is read no table
    // address is waited for inside the loop - read_unit stays straight-line scalar loads.  (A wave's only or
    // last segment is read twice.)
    const int32_t cid0 = seg_class[n_units > 0 ? sb : 0];
    const int32_t cid1 = seg_class[n_units > 1 ? sb + 1 : (n_units > 0 ? sb : 0)];

    // what the wave knows about a group before it streams it: wave-uniform, read with scalar loads (which the
    // vector loads in flight do not wait for) one group ahead, the segment's offsets included
    struct unit {
        int u;          // index among the wave's units; n_units and above: there is none
        int D;
        int cid;        // the segment's class: row cid of cls_tab, rows 64 cid .. of cls_mask
        int row0;
        int lead;       // entries of the previous group in front of this one's first: k0 - k0a < E
        int k0a, len;   // aligned stream start; entries from there to the group's end.  0: nothing to do
                        // (behind the wave's last unit, segment not eligible; or a structure rewritten behind
                        // the plan's back, which alone gives an eligible segment no entries)
        int32_t off[ND];
    };
    // what unit_of reads: straight-line scalar loads, every address one of a unit the wave owns (the last
    // one again behind the end); nothing here waits for them
    struct unit_raw {
        int u, row0, k0, k1, D, cid;
        int32_t off[ND];
    };
    auto read_unit = [&](int u) {
        unit_raw r;
        r.u = u;
        const int uc = u < n_units ? u : n_units - 1;
        const int64_t s = sb + uc;
        r.cid = uc == 0 ? cid0 : cid1;
        const int32_t* tab = cls_tab + int64_t(r.cid) * OFFS_TAB;
        r.row0 = int(s * 64);
        const int last = r.row0 + GR < n_rows ? r.row0 + GR : n_rows;
        r.k0 = row_ptrs[r.row0];
        r.k1 = row_ptrs[last];
        r.D = tab[0];
#pragma unroll
        for (int d = 0; d < ND; ++d) r.off[d] = tab[1 + d];
        return r;
    };
    auto unit_from = [&](const unit_raw& r) {
        unit q;
        q.u = r.u;
        q.D = r.D;
        q.cid = r.cid;
        q.row0 = r.row0;
#pragma unroll
        for (int d = 0; d < ND; ++d) q.off[d] = r.off[d];
        q.k0a = r.k0 & ~(E - 1);
        q.lead = r.k0 - q.k0a;
        int len = r.k1 - q.k0a;
        // (a structure rewritten behind the plan's back must not write outside the stage)
        if (len > CAP + E - 1) len = CAP + E - 1;
        q.len = (r.u < n_units && r.D > 0 && r.D <= ND && r.k1 > r.k0) ? len : 0;
        return q;
    };
    auto unit_of = [&](int u) { return unit_from(read_unit(u)); };
    // The value loads of a group with len > 0: unconditional, a lane behind the group's end reads the 16 bytes
    // that hold the group's last entry again (one access for all such lanes), and what it reads is not read by
    // any row.  INVARIANT: every address lies within [k0a, k0a + len) of a group that this wave owns.  There are
    // two load sites, this one in front of the loop and one in it, and v[] has one register home.
    VT v[NL];
    auto load_vals = [&](const unit& q) {
        const int last_chunk = (q.len - 1) & ~(E - 1);
#pragma unroll
        for (int t = 0; t < NL; ++t) {
            const int k = (t * 64 + lane) * E;
            const VT* from =
                reinterpret_cast<const VT*>(vals + (int64_t(q.k0a) + (k < last_chunk ? k : last_chunk)));
            if constexpr (NT) {
                v[t] = __builtin_nontemporal_load(from);
            } else {
                v[t] = *from;
            }
        }
    };
    // A group in two halves, so that the loop below can put the next group's value loads between them.
    // What a lane keeps from one half to the other; diagonal slots are compile-time indices (x and the values
    // stay in registers).
    struct lane_state {
        int row;
        bool valid;
        uint32_t mask_raw;
        T sum, bdot;
        T xv[ND];
    };
    // first half (cur.len > 0, its values in v[]): the group's own loads, the scalar loads of the next unit,
    // the values to the stage.  Returns with v[] free.
    auto head = [&](const unit& cur, lane_state& ls, unit_raw& nxt_raw) {
        ls.row = cur.row0 + lane;
        ls.valid = ls.row < n_rows;
        // (first what the row phase needs first; a class' mask of a row at or behind n_rows is 0)
        // (a scalar base and the lane as a 32-bit offset: no address pair kept in vector registers)
        ls.mask_raw = (cls_mask + int64_t(cur.cid) * 64)[threadIdx.x];
        ls.sum = T(0);
        ls.bdot = T(0);
        if (ADV && beta != T(0)) ls.sum = c[ls.valid ? ls.row : cur.row0] * beta;
        if (DOT) ls.bdot = x[ls.valid ? ls.row : cur.row0];
        // clamp(row + off_d): the column itself for a stored entry, anything in bounds for an absent slot
        // (the sum wraps for those at worst)
        const int ncm1 = n_cols - 1;
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const int idx = int(uint32_t(ls.row) + uint32_t(cur.off[d]));
            ls.xv[d] = x[idx < 0 ? 0 : (idx > ncm1 ? ncm1 : idx)];
        }
        nxt_raw = read_unit(cur.u + 1);
#pragma unroll
        for (int t = 0; t < NL; ++t) *reinterpret_cast<VT*>(&stage[(t * 64 + lane) * E]) = v[t];
        wave_lds_sync();
        // (nothing that waits - for the scalar loads above, for x, the mask or the row pointer - moves up in
        // front of the stage write or, in the loop, in front of the value loads that follow)
        __builtin_amdgcn_sched_barrier(0);
    };
    // the wave's next group with values behind the unit read ahead, u >= n_units if there is none
    auto next_group = [&](const unit_raw& nxt_raw) {
        unit nxt = unit_from(nxt_raw);
        while (nxt.u < n_units && nxt.len == 0) nxt = unit_of(nxt.u + 1);
        return nxt;
    };
    // second half: the row phase and the store
    auto rows = [&](const unit& cur, lane_state& ls) {
        __builtin_amdgcn_sched_barrier(0);
        const uint32_t mask = ls.valid ? ls.mask_raw : 0u;
        // The row's start in the stage.  The build kernel sets one mask bit per stored entry, so the rows in
        // front of this one hold the wave's exclusive prefix sum of popc(mask) entries, behind the `lead` entries
        // of the previous group: row_ptrs[row] is not loaded.  With popc(mask) <= D <= ND (unit_from) every
        // index below is at most lead + 64 ND - 1 < CAP + E - 1: inside the stage whatever row_ptrs holds, also
        // for a structure rewritten behind the plan's back.  Waits for the mask load only.
        const int rs = cur.lead + wave_exclusive_sum(__popc(mask));
        T sum = ls.sum;
        auto slots = [&](auto d0_c) {
            constexpr int d0 = decltype(d0_c)::value;
            constexpr int NB = ND - d0 < 8 ? ND - d0 : 8;      // (the last body of 28 slots has four)
            T val[NB];
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                // entries of the row in front of slot d = stored slots below d
                const int pos = rs + __popc(mask & ((1u << (d0 + i)) - 1u));
                val[i] = stage[pos];
            }
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                // (keeps the eight LDS reads together in front of the arithmetic)
                asm volatile("" : "+v"(val[i]));
            }
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const T pr = ADV ? (alpha * val[i]) * ls.xv[d0 + i] : val[i] * ls.xv[d0 + i];
                sum = ((mask >> (d0 + i)) & 1u) != 0 ? sum + pr : sum;
            }
        };
        slots(std::integral_constant<int, 0>{});
        if constexpr (ND > 8) slots(std::integral_constant<int, 8>{});
        if constexpr (ND > 16) slots(std::integral_constant<int, 16>{});
        if constexpr (ND > 24) slots(std::integral_constant<int, 24>{});
        // (the sum of EVERY lane is complete here: without this the compiler moves the row phase under the
        // `valid` branch below, whose other side reaches the next group with this group's x loads unwaited-for
        // and puts write-after-load waits between the next group's x loads)
        asm volatile("" : "+v"(sum));
        if constexpr (NT) {
            if (ls.valid) __builtin_nontemporal_store(sum, &c[ls.row]);
        } else {
            if (ls.valid) c[ls.row] = sum;
        }
        if constexpr (DOT) {
            // (the row-segment kernel's lane for this row is row % 64 too)
            const T term = ls.bdot * sum;
            if (ls.valid) dot_acc += term;
        }
        wave_lds_sync();
    };

    if (n_units > 0) {
        unit cur = unit_of(0);
        while (cur.u < n_units && cur.len == 0) cur = unit_of(cur.u + 1);
        if (cur.u < n_units) {
            lane_state ls;
            unit_raw nxt_raw;
            load_vals(cur);
            // Every group that has a successor: the successor's NL value loads are issued between the halves,
            // ALWAYS (the loop is left in front of them otherwise), so they are under way during the row phase
            // and no wait of the row phase asks for them.  The wave's last group runs behind the loop with
            // nothing but its own loads in flight.
            head(cur, ls, nxt_raw);
            unit nxt = next_group(nxt_raw);
            while (nxt.u < n_units) {
                load_vals(nxt);
                rows(cur, ls);
                cur = nxt;
                head(cur, ls, nxt_raw);
                nxt = next_group(nxt_raw);
            }
            rows(cur, ls);
        }
    }
    if constexpr (DOT) {
        dot_acc = wave_sum(dot_acc);
        if (lane == 0) dot_partial[wave_id] = dot_acc;
    }
}

#endif  // __HIPCC__

}  // namespace gkoc
