// CSR SpMV for gfx950: software-pipelined row-segment-per-wavefront kernel.
//
// Replaces gko::kernels::hip::csr::{spmv, advanced_spmv}
// (decl core/matrix/csr_kernels.hpp:29-43; semantics
// reference/matrix/csr_kernels.cpp:49-118; stock GPU version
// common/cuda_hip/matrix/csr_kernels.template.cpp:206-586,2351-2468).
//
// The kernel lives in csr_spmv_pipe.hpp (variant 3).  Summary:
//  * one 64-lane wavefront owns 64 consecutive rows = one contiguous range of
//    the val / col_idx streams, read with 16-byte-per-lane vector loads (no
//    per-row alignment loss, no idle lanes on 27-nnz rows), double-buffered in
//    registers so the HBM round trip overlaps the b-vector gather;
//  * products val[k]*b[col[k]] go to an LDS ring (8 KB per wave, 20 waves/CU);
//  * lane = row then adds its products from LDS in k order => same summation
//    order and roundings as the sequential reference (this file is compiled
//    with -ffp-contract=off): BIT-IDENTICAL results, no atomics, no zeroing
//    pass over c, no host-built srow table, any strategy name accepted;
//  * rows longer than GKOC_CSR_LONG_ROW are summed cooperatively by the whole
//    wave (tolerance instead of bit-exactness for those rows only).
//
// Algorithmic HBM bytes: nnz*(sizeof(T)+sizeof(I)) + (n+1)*sizeof(I)
//                        + n_cols*sizeof(T) (b once) + n*sizeof(T) (c).
//
// What the launchers know about a matrix from earlier products - its long rows, its column-offset plan - is kept
// by csr_structure.hip; a product holds a csr_structure_lease while it enqueues kernels that read it.
#include <algorithm>
#include <type_traits>

#include "common.hpp"
#include "csr_long_rows.hpp"
#include "csr_offsets.hpp"
#include "csr_spmv_multi.hpp"
#include "csr_spmv_pipe.hpp"
#include "csr_structure.hpp"
#include "fused.hpp"

namespace gkoc {
namespace {

// ---- the launch plan of the row-segment kernels (csr_spmv_pipe3_kernel, csr_spmv_multi_kernel) -------------
template <int N>
using int_c = std::integral_constant<int, N>;

// 64-row segments (lane = row in the row phase).  Large matrices: 2 segments
// = 128 rows per wavefront, whose 1 KB of results is written in one burst at
// the end of the wave (mode 0x2000).  Below 65536 segments (4 M rows) the
// grid is only a few rounds of the 5120 resident waves deep and the tail
// dominates: one segment per wave then (+1 % at 2 M rows, +7 % at 0.9 M,
// +15 % at 0.26 M rows).  In-order dispatch keeps the set of resident waves
// on a compact window of rows, which is what lets the b-vector lines shared
// by neighbouring rows hit in L2.
// (round 3, measured again on 1 / 2 / 4 / 16.7 M rows, profiles/r03_experiments.txt: forcing one or
// two segments per wave or 32-row segments changes nothing or loses: 2.1 M rows 139.8 us with
// this rule, 142-147 us with the alternatives)
struct segment_plan {
    int64_t n_seg;      // 64-row segments of the matrix
    int spw;            // segments per wave
    int64_t n_waves;    // = workgroups
};

// forced_spw = 1 or 2: that many segments per wave whatever the size (any other value: the rule)
int plan_segments(int64_t n_rows, segment_plan* plan, int64_t forced_spw = 0)
{
    const int64_t n_seg = ceildiv(n_rows, 64);
    const int spw = (forced_spw == 1 || forced_spw == 2) ? int(forced_spw) : (n_seg < 65536 ? 1 : 2);
    const int64_t n_waves = ceildiv(n_seg, spw);
    GKOC_REQUIRE(n_waves < (int64_t(1) << 31), GKOC_E_NOT_SUPPORTED, "more than 2^31 row segments");
    *plan = segment_plan{n_seg, spw, n_waves};
    return GKOC_OK;
}

// the kernel's mode bits for spw segments per wave (spw << 12: csr_spmv_pipe.hpp DEFER) as a compile-time
// constant: launch(int_c<0x1000>) or launch(int_c<0x2000>)
template <typename F>
void with_store_mode(int spw, F&& launch)
{
    if (spw == 2) {
        launch(int_c<0x2000>{});
    } else {
        launch(int_c<0x1000>{});
    }
}

// E-element vector loads need the array bases aligned like the vector types (vecT<V, E> / vecT<I, E>: true
// for whole allocations; sub-views that are not take the scalar-load instantiation E = 1)
template <typename V, typename I>
bool streams_aligned(const V* vals, const I* cols, int E)
{
    return reinterpret_cast<uintptr_t>(vals) % (E * sizeof(V)) == 0 &&
           reinterpret_cast<uintptr_t>(cols) % (E * sizeof(I)) == 0;
}

// Load layouts of the row-segment kernel, <E, U> = entries per lane and load x load groups in flight.
template <typename T>
struct pipe_layout {
    // 32 B of values per lane and load: 4 doubles or 8 floats (ring = 8 KB); the layout of rounds 1-2 is <EV, 1>
    static constexpr int EV = 32 / sizeof(T);
    static constexpr int RINGV = 8192 / sizeof(T);
    // Entries per lane and load x load groups in flight (ring 8 KB): 2 x 3 for double, 4 x 2 for
    // float - 16 B of values per lane and load, 48 / 32 B in flight.  Measured in one process on L256
    // (tools/f32_variants.py, profiles/r03_experiments.txt): double 4 x 1 (rounds 1-2) 985 us, 2 x 3
    // 954, 2 x 4 960, 1 x 6 968, 4 x 2 980, 1 x 8 978, 1 x 4 986; float 8 x 1 (rounds 1-2) 847 us,
    // 4 x 2 793, 4 x 3 823, 8 x 2 / 4 x 4 / 2 x 8 slower.  By size (tools/csr_layout_ab.py, double): 4.1 M rows
    // 251 -> 246 us, 8.4 M 510 -> 495, 16.8 M 985 -> 953; the Flan-like matrix (81 per row) 272 both;
    // 5-pt 4096^2 397 -> 405.
    static constexpr int PE = sizeof(T) == 8 ? 2 : 4, PU = sizeof(T) == 8 ? 3 : 2;
};

// Three and more right-hand sides, fragment layout (csr_spmv_multi.hpp): the lanes of a gather cover whole
// rows of b.  Small waves - 16 rows, 6 KB of LDS - so that 20+ of them are resident per CU.  L256
// (profiles/r03_multi_rhs_256.txt): 3 / 4 / 8 columns 2.17 / 2.23 / 5.08 ms with the ring and row-ordered
// kernels of round 2 -> 1.77 / 1.77 / 1.97 ms.  Measured variants: 32 / 64 rows per wave (12 / 24 KB: 2.2 -
// 4.6 ms), 2 - 8 entries per step (+- 3 %; 3 for eight columns, 4 for four); two columns stay with the ring
// kernel (launch_csr_pair: 1.46 ms, this layout 2.36 ms with 32-row waves).
// Since round 5 the pipelined form, four segments per wave: L256 3 / 4 / 8 columns 1.87 / 1.90 / 2.10 ->
// 1.76 / 1.79 / 2.00 ms (profiles/r05_multi_rhs_pmc.txt).  The variants GKOC_TUNE_CSR_MULTI_VARIANT used to
// select - the kernel of rounds 3-4 with pairs of columns or two row groups per wave, other entries-per-step
// and segments-per-wave choices, strided rounds, values handed over by the row below - were all measured slower
// (that file and profiles/r06/r06_multi_rhs_baseline.txt) and are not launched any more.
template <typename T, typename I, bool ADV>
int launch_csr_columns(gkoc_stream_t s, int64_t n_rows, int64_t n_cols, const T* alpha, const I* row_ptrs,
                       const I* col_idxs, const T* vals, const T* b, int64_t ldb, const T* beta, T* c,
                       int64_t ldc, int64_t nrhs)
{
    const bool idx32 = n_cols * ldb < (int64_t(1) << 32);
    const bool pairs_ok = reinterpret_cast<uintptr_t>(b) % (2 * sizeof(T)) == 0 && ldb % 2 == 0 &&
                          reinterpret_cast<uintptr_t>(c) % (2 * sizeof(T)) == 0 && ldc % 2 == 0;
    const int64_t chunk_rows = tune_value(GKOC_TUNE_MULTI_XCD_CHUNK_ROWS);
    // chunks of NR columns, CPL columns per lane (64 * CPL / NR rows per segment), KU entries per step;
    // pipelined: csr_spmv_frag_pipe_kernel with four segments per wave, else csr_spmv_frag_kernel
    auto launch = [&](auto nr, auto cpl, auto ku, auto pipelined) -> int {
        constexpr int NR = decltype(nr)::value, CPL = decltype(cpl)::value, KU = decltype(ku)::value;
        constexpr bool PIPE = decltype(pipelined)::value;
        constexpr int rows = 64 * CPL / NR, segs = PIPE ? 4 : 1;
        const int64_t nwg = ceildiv(ceildiv(n_rows, rows), segs);
        GKOC_REQUIRE(nwg < (int64_t(1) << 31), GKOC_E_NOT_SUPPORTED, "more than 2^31 waves");
        const dim3 grid(static_cast<unsigned>(nwg)), block(64);
        auto go = [&](auto idx) {
            constexpr bool IDX32 = decltype(idx)::value;
            if constexpr (PIPE) {
                csr_spmv_frag_pipe_kernel<T, I, ADV, NR, CPL, KU, IDX32><<<grid, block, 0, as_stream(s)>>>(
                    n_rows, row_ptrs, col_idxs, vals, b, ldb, c, ldc, static_cast<int>(nrhs), alpha, beta, segs,
                    chunk_rows / (rows * segs));
            } else {
                csr_spmv_frag_kernel<T, I, ADV, NR, CPL, KU, IDX32><<<grid, block, 0, as_stream(s)>>>(
                    n_rows, row_ptrs, col_idxs, vals, b, ldb, c, ldc, static_cast<int>(nrhs), alpha, beta,
                    chunk_rows / rows);
            }
        };
        if (idx32) {
            go(std::true_type{});
        } else {
            go(std::false_type{});
        }
        GKOC_LAUNCH_OK();
        return GKOC_OK;
    };
    // four lanes per row: one column each up to four columns, a pair of columns each beyond
    if (nrhs <= 4) return launch(int_c<4>{}, int_c<1>{}, int_c<4>{}, std::true_type{});
    if (pairs_ok) return launch(int_c<8>{}, int_c<2>{}, int_c<3>{}, std::true_type{});
    // odd strides or unaligned b / c: eight lanes per row, one column each, the kernel of rounds 3-4
    return launch(int_c<8>{}, int_c<1>{}, int_c<4>{}, std::false_type{});
}

// Two right-hand sides, vector loads possible: the row-segment walk of the single-column kernel with the two
// products of an entry side by side in the LDS ring (csr_spmv_multi_kernel; 8 KB ring of 512
// entries).  L256: 1.46 ms against 2.18 ms for one pass per column.
template <typename T, typename I, bool ADV>
int launch_csr_pair(gkoc_stream_t s, int64_t n_rows, const T* alpha, const I* row_ptrs, const I* col_idxs,
                    const T* vals, const T* b, int64_t ldb, const T* beta, T* c, int64_t ldc)
{
    using lay = pipe_layout<T>;
    segment_plan p;
    GKOC_TRY(plan_segments(n_rows, &p));
    const dim3 grid(static_cast<unsigned>(p.n_waves)), block(64);
    const int b_vec_ok = reinterpret_cast<uintptr_t>(b) % (2 * sizeof(T)) == 0 && ldb % 2 == 0;
    const int64_t xcd_chunk = tune_value(GKOC_TUNE_MULTI_XCD_CHUNK_ROWS) / (64 * p.spw);
    auto launch = [&](auto e, auto u) {
        csr_spmv_multi_kernel<T, I, ADV, decltype(e)::value, decltype(u)::value, lay::RINGV / 2, 2>
            <<<grid, block, 0, as_stream(s)>>>(n_rows, p.n_seg, p.spw, row_ptrs, col_idxs, vals, b, ldb, c, ldc, 2,
                                               alpha, beta, b_vec_ok, xcd_chunk);
    };
    // two entries per lane and load, two load groups in flight (more, smaller loads under way: the
    // single-column kernel's lesson of round 3): L256 1.457 -> 1.38-1.40 ms = 55 % of 8 TB/s
    // (profiles/r04_experiments.txt); GKOC_TUNE_CSR_LOAD_GROUPS = 1: four entries, one group
    if (tune_value(GKOC_TUNE_CSR_LOAD_GROUPS) == 1) {
        launch(int_c<lay::EV>{}, int_c<1>{});
    } else {
        launch(int_c<lay::EV / 2>{}, int_c<2>{});
    }
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

// ---- the product through a column-offset plan (csr_offsets.hpp; the plan is csr_structure.hip's) -------------
// The plan a one-column, unit-stride product of these arrays may use, or nullptr: double / float values aligned
// for 16-byte loads and 32-bit indices.  Valid while the lease is held - to the last kernel that reads it.
template <typename T, typename I>
offsets_plan* offsets_plan_of(csr_structure_lease& lease, hipStream_t st, int64_t n_rows, int64_t n_cols,
                              const I* row_ptrs, const I* col_idxs, const T* vals, const T* b,
                              const csr_long_info& lng)
{
    if constexpr (std::is_same<I, int32_t>::value && (sizeof(T) == 8 || sizeof(T) == 4)) {
        if (vals != nullptr && b != nullptr && reinterpret_cast<uintptr_t>(vals) % 16 == 0) {
            return csr_offsets_plan_for(lease, st, n_rows, n_cols, row_ptrs, col_idxs, lng);
        }
    }
    return nullptr;
}

// the MI355X's Infinity Cache, 256 MiB: a product that streams more than this per call cannot live in it, and its
// value stream and result bypass it (measured on both sides of it: docs/KERNELS.md 36)
constexpr int64_t offsets_nt_min_bytes = int64_t(256) << 20;

// the product of the plan's segments: the kernel with the fewest diagonal slots (8, 16, 28 or 32) that holds the
// plan's largest D - its value stream, its stage and its x loads are sized by the slot count (one straight-line
// body per kernel, csr_offsets.hpp; a segment with fewer offsets is right in any wider kernel).  28 is the 27-point
// stencil's.
// The price: in a plan that has wide segments the narrow ones issue dead x loads - 5 % on a matrix with one
// segment of 9 offsets in eight of 3 under the 32-slot kernel, nothing with one in two (docs/KERNELS.md 36).
template <typename T, bool ADV, bool DOT>
void launch_offsets_kernel(hipStream_t st, const offsets_plan& pl, const segment_plan& p, int64_t n_rows,
                           int64_t n_cols, const T* alpha, const int32_t* row_ptrs, const T* vals, const T* b,
                           const T* beta, T* c, T* dot_partial)
{
    const dim3 grid(static_cast<unsigned>(p.n_waves)), block(64);
    // values, x, c and the row pointers: what a product streams.  Above the Infinity Cache's size the values and
    // c go non-temporally (csr_offsets.hpp NT), below it repeated products are served from that cache
    const int64_t product_bytes = pl.nnz * int64_t(sizeof(T)) + (n_rows + n_cols) * int64_t(sizeof(T)) + n_rows * 4;
    auto launch = [&](auto nd, auto nt) {
        constexpr int ND = decltype(nd)::value;
        csr_spmv_pipe3_kernel_offsets<T, ADV, DOT, ND, decltype(nt)::value><<<grid, block, 0, st>>>(
            int32_t(n_rows), int32_t(n_cols), p.n_seg, p.spw, row_ptrs, vals, b, c, alpha, beta, pl.seg_class,
            pl.cls_tab, pl.cls_mask, dot_partial);
    };
    auto go = [&](auto nd) {
        if (product_bytes > offsets_nt_min_bytes) {
            launch(nd, std::true_type{});
        } else {
            launch(nd, std::false_type{});
        }
    };
    if (pl.max_d <= 8) {
        go(std::integral_constant<int, 8>{});
    } else if (pl.max_d <= 16) {
        go(std::integral_constant<int, 16>{});
    } else if (pl.max_d <= 28) {
        go(std::integral_constant<int, 28>{});
    } else {
        go(std::integral_constant<int, OFFS_MAX>{});
    }
}

// The hub rows' kernels run BEHIND the row-segment kernel on the caller's stream.  (Round 6 also ran them
// BESIDE it - a side stream per calling stream, forked in front of the product and joined behind it by two
// events; the two kernels write disjoint rows of c.  The heavy-tailed stand-in took 245.7 us that way
// against 231.5 us in sequence, profiles/r06/r06_hub_rows_beside.txt: gone again.)
template <typename T, typename I, bool ADV>
int launch_hub_rows(hipStream_t st, const csr_long_info& lng, int64_t n_rows, const T* alpha, const I* row_ptrs,
                    const I* col_idxs, const T* vals, const T* b, int64_t ldb, const T* beta, T* c, int64_t ldc)
{
    // (the chunk sums go to the CALLING stream's buffer: long_partial_for)
    csr_flagged_segments_kernel<T, I, ADV><<<dim3(unsigned(lng.count * LONG_PARTS)), dim3(LONG_WG), 0, st>>>(
        n_rows, row_ptrs, col_idxs, vals, b, ldb, c, ldc, alpha, beta, lng.list, static_cast<T*>(lng.partial));
    GKOC_LAUNCH_OK();
    csr_long_rows_fold_kernel<T, I, ADV><<<dim3(unsigned(lng.count)), dim3(64), 0, st>>>(
        n_rows, row_ptrs, c, ldc, beta, lng.list, static_cast<const T*>(lng.partial));
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

// One right-hand side - and whatever the launchers above do not take: the kernel walks nrhs columns one
// after the other.
template <typename T, typename I, bool ADV>
int launch_csr_single(gkoc_stream_t s, int64_t n_rows, int64_t n_cols, const T* alpha, const I* row_ptrs, const I* col_idxs,
                      const T* vals, const T* b, int64_t ldb, const T* beta, T* c, int64_t ldc, int64_t nrhs)
{
    using lay = pipe_layout<T>;
    // What is cached about the matrix is leased to the end of this function: neither the flags nor a plan can be
    // released while their product is being enqueued.
    csr_structure_lease lease;
    // rows far longer than the rest: their segments are left out here and done by many workgroups
    // (csr_long_rows.hpp); one right-hand side
    csr_long_info lng;
    if (nrhs == 1 && tune_value(GKOC_TUNE_CSR_LONG_ROWS) != 0) {
        GKOC_TRY(csr_long_info_for(lease, as_stream(s), n_rows, row_ptrs, &lng));
    }
    const uint32_t* seg_skip = lng.count > 0 ? lng.bits : nullptr;
    // stencil-like structure seen before: the column-offset plan (csr_offsets.hpp) takes its eligible
    // segments, the row-segment kernel below the others
    constexpr bool offsets_type = std::is_same<I, int32_t>::value && (sizeof(T) == 8 || sizeof(T) == 4);
    offsets_plan* plan = nullptr;
    if (nrhs == 1 && ldb == 1 && ldc == 1) {
        plan = offsets_plan_of(lease, as_stream(s), n_rows, n_cols, row_ptrs, col_idxs, vals, b, lng);
    }
    if (lng.count <= 0 && plan == nullptr) lease.give_back();      // (nothing cached is read below)
    // GKOC_TUNE_CSR_SEGS_PER_WAVE forces 1 or 2 segments per wave (round 6 tried "up to eight for matrices
    // with short rows" - the heavy-tailed stand-in 256 us with one, 261 with two, 276 with four, 320 with eight
    // segments; 5-pt 4096^2 325 / 289 / 325 / 315; profiles/r06/r06_segments_per_wave.txt: the size rule
    // stays, and the four / eight-segment variants - whose loop over runs of unflagged segments cost every
    // variant of the kernel 12-16 VGPRs - are gone again)
    segment_plan p;
    GKOC_TRY(plan_segments(n_rows, &p, tune_value(GKOC_TUNE_CSR_SEGS_PER_WAVE)));
    const dim3 grid(static_cast<unsigned>(p.n_waves)), block(64);
    if constexpr (offsets_type) {
        if (plan != nullptr) {
            launch_offsets_kernel<T, ADV, false>(as_stream(s), *plan, p, n_rows, n_cols, alpha, row_ptrs, vals, b,
                                                 beta, c, static_cast<T*>(nullptr));
            GKOC_LAUNCH_OK();
            ++plan->products;
            if (plan->skip == nullptr) return GKOC_OK;      // every segment was eligible
            seg_skip = plan->skip;
        }
    }
    // XCD-contiguous wave order needs enough waves per XCD to keep the in-order
    // window argument valid; below that the plain order is used
    // ... and is the default for a matrix WITH HUB ROWS (flagged segments): its gathers go all over b, and with
    // one contiguous eighth of the rows per XCD an L2 holds the lines of its own eighth instead of a share of
    // everybody's.  Heavy-tailed stand-in 246.6 -> 226.0 us; the stencils lose 0.5-3 % with it (27-pt 256^3
    // 982 -> 1003, 5-pt 4096^2 274 -> 282) and keep the plain order (profiles/r06/r06_waves_per_workgroup.txt).
    // GKOC_TUNE_CSR_XCD_MAP: 1 = always, 2 = never.
    const int64_t xcd_choice = tune_value(GKOC_TUNE_CSR_XCD_MAP);
    const int xcd_map =
        ((xcd_choice == 1 || (xcd_choice == 0 && lng.count > 0)) && p.n_waves >= 8 * 1024) ? 1 : 0;
    // Measured and rejected on the Flan-like matrix and on L256 (profiles/r02_experiments,
    // profiles/r02_flan_pmc): 16 / 32 KB rings with 2-4 load groups (fewer resident waves: 299-475 us
    // against 288), 32-row segments (294), one or two entries per lane and load so that neighbouring
    // lanes gather neighbouring columns (301-305).  What helped was the row-phase loop
    // (csr_spmv_pipe.hpp): 295 -> 277 us.
    // (round 6 also tried two / four / eight WAVES per workgroup, every wave with its own segments and ring - a
    // grid of one-wave workgroups of short-row segments is paced by the dispatcher: 3.5 ns per wave chip-wide,
    // profiles/r06_irregular_pmc.txt.  The pace is per wave, not per workgroup: heavy-tailed stand-in 247 / 241 /
    // 246 / 299 us, every stencil 10-40 % slower; profiles/r06/r06_waves_per_workgroup.txt.)
    const bool vec_ok = streams_aligned(vals, col_idxs, lay::EV);
    const int64_t groups = tune_value(GKOC_TUNE_CSR_LOAD_GROUPS);
    const bool long_float_rows = sizeof(T) == 4 && lng.nnz > 0 && lng.nnz >= 40 * n_rows;
    with_store_mode(p.spw, [&](auto mode) {
        auto launch = [&](auto e, auto u) {
            csr_spmv_pipe3_kernel<T, I, ADV, 64, decltype(e)::value, decltype(u)::value, lay::RINGV, 1,
                                  decltype(mode)::value><<<grid, block, 0, as_stream(s)>>>(
                n_rows, p.n_seg, p.spw, row_ptrs, col_idxs, vals, b, ldb, c, ldc, static_cast<int>(nrhs), alpha,
                beta, nullptr, xcd_map, static_cast<const I*>(nullptr), static_cast<int*>(nullptr), int64_t(0),
                int64_t(0), static_cast<const uint32_t*>(nullptr), uint32_t(0), static_cast<const I*>(nullptr),
                static_cast<const I*>(nullptr), static_cast<const T*>(nullptr), static_cast<uint32_t*>(nullptr),
                uint32_t(0), 0, int64_t(-1), seg_skip);
        };
        if (!vec_ok) {
            launch(int_c<1>{}, int_c<4>{});
        } else if (groups == 3 || (groups == 0 && long_float_rows)) {
            // float values and LONG rows (40 and more entries on average; the count comes with the first product's
            // look at the row pointers): ONE entry per lane and load, eight load groups - neighbouring lanes then
            // gather neighbouring entries of a row, whose columns come in runs (a 27-pt stencil with 2 / 3 / 5
            // unknowns per node, 53 / 79 / 130 per row: 172 -> 165, 200 -> 182, 231 -> 207 us against four entries
            // per lane; 7 and 27 per row lose 5-6 % with it, and for double all layouts are within 1.5 %:
            // profiles/r06/r06_load_layouts.txt).  GKOC_TUNE_CSR_LOAD_GROUPS: 3 forces it, 4 = two entries x four
            // groups, 1 = the wide loads.
            launch(int_c<1>{}, int_c<8>{});
        } else if (groups == 4) {
            launch(int_c<2>{}, int_c<4>{});
        } else if (groups == 1 || p.n_seg < 32768) {
            // below 2 M rows the grid is a few rounds deep and the wider layout of rounds 1-2 is as fast or
            // faster (64^3: 18.4 against 20.7 us; 1 - 2 M rows: equal); key 2 = 1 forces it for A/B runs
            launch(int_c<lay::EV>{}, int_c<1>{});
        } else {
            launch(int_c<lay::PE>{}, int_c<lay::PU>{});
        }
    });
    GKOC_LAUNCH_OK();
    if (lng.count > 0) {
        GKOC_TRY((launch_hub_rows<T, I, ADV>(as_stream(s), lng, n_rows, alpha, row_ptrs, col_idxs, vals, b, ldb,
                                             beta, c, ldc)));
    }
    return GKOC_OK;
}

template <typename T, typename I, bool ADV>
int launch_csr(gkoc_stream_t s, int64_t n_rows, int64_t n_cols, const T* alpha, const I* row_ptrs, const I* col_idxs,
               const T* vals, const T* b, int64_t ldb, const T* beta, T* c, int64_t ldc, int64_t nrhs)
{
    GKOC_REQUIRE(n_rows >= 0 && n_cols >= 0 && nrhs >= 0, GKOC_E_INVALID, "negative dimension");
    if (n_rows == 0 || nrhs == 0) return GKOC_OK;
    GKOC_REQUIRE(row_ptrs && c, GKOC_E_INVALID, "null pointer");
    GKOC_REQUIRE(ldc >= nrhs && (n_cols == 0 || ldb >= nrhs), GKOC_E_INVALID, "stride smaller than nrhs");
    if (ADV) GKOC_REQUIRE(alpha && beta, GKOC_E_INVALID, "null alpha/beta");
    if (nrhs >= 3) {
        return launch_csr_columns<T, I, ADV>(s, n_rows, n_cols, alpha, row_ptrs, col_idxs, vals, b, ldb, beta, c,
                                             ldc, nrhs);
    }
    if (nrhs == 2 && streams_aligned(vals, col_idxs, pipe_layout<T>::EV)) {
        return launch_csr_pair<T, I, ADV>(s, n_rows, alpha, row_ptrs, col_idxs, vals, b, ldb, beta, c, ldc);
    }
    // (two columns whose matrix streams are not aligned for vector loads: one pass per column)
    return launch_csr_single<T, I, ADV>(s, n_rows, n_cols, alpha, row_ptrs, col_idxs, vals, b, ldb, beta, c, ldc, nrhs);
}

// The distributed product in ONE kernel (csr_spmv_pipe.hpp, GATE): the interior rows of the rank's
// local block and, on the last waves of the grid, the boundary rows as complete rows over [local
// columns | halo]; b = [local vector | halo] (unit stride); gate = two counters in device memory
// (zero at the start).
__global__ void gate_open_kernel(uint32_t* gate, uint32_t epoch)
{
    __hip_atomic_store(gate, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Boundary waves may SPIN (their halo travels on another stream), and a spinning wave keeps its
// slot and its 8 KB of LDS until the gate opens.  The kernels that open it - the exchange's
// (RCCL's send / recv workgroups) and gkoc_gate_open - need room on the device to run at all, and
// stream priority does not preempt resident waves.  So at most 8 boundary waves per CU are ever
// launched (2048 on an MI355X, of about 5120 that are resident at a time with 8 KB of LDS each):
// more than half of every resource stays with waves that finish by themselves.  Above that bound
// the caller takes the join-based product (local rows || exchange, stream-ordered boundary rows),
// whose waiting is the stream's, as in the reference (core/distributed/matrix.cpp:450-509 req.wait()).
int64_t gated_wave_cap() { return int64_t(current_device_props().num_cu) * 8; }

bool gated_fits(int64_t n_rows, int64_t head_rows, int64_t tail_rows)
{
    if (n_rows <= 0 || head_rows < 0 || tail_rows < 0 || head_rows + tail_rows > n_rows ||
        head_rows + tail_rows == 0) {
        return false;
    }
    return ceildiv(head_rows + tail_rows, 64) <= gated_wave_cap();
}

template <typename T, typename I>
int launch_csr_gated(gkoc_stream_t s, int64_t n_rows, const I* row_ptrs, const I* col_idxs, const T* vals,
                     const I* bnd_ptrs, const I* bnd_cols, const T* bnd_vals, const T* b, T* c,
                     int64_t head_rows, int64_t tail_rows, const uint32_t* gate, uint32_t epoch,
                     uint32_t* fork_word, uint32_t fork_number, T* dot_out = nullptr, void* work = nullptr,
                     size_t work_bytes = 0)
{
    GKOC_REQUIRE(n_rows > 0 && head_rows >= 0 && tail_rows >= 0 && head_rows + tail_rows <= n_rows,
                 GKOC_E_INVALID, "bad dimensions");
    GKOC_REQUIRE(head_rows + tail_rows > 0, GKOC_E_INVALID, "no boundary rows: use gkoc_csr_spmv_*");
    GKOC_REQUIRE(row_ptrs && col_idxs && vals && bnd_ptrs && bnd_cols && bnd_vals && b && c && gate,
                 GKOC_E_INVALID, "null pointer");
    GKOC_REQUIRE(gated_fits(n_rows, head_rows, tail_rows), GKOC_E_NOT_SUPPORTED,
                 "more boundary rows than may wait on the device at once (gkoc_csr_spmv_gated_fits): "
                 "use the join-based product");
    using lay = pipe_layout<T>;
    GKOC_REQUIRE(streams_aligned(vals, col_idxs, lay::EV) && streams_aligned(bnd_vals, bnd_cols, lay::EV),
                 GKOC_E_NOT_SUPPORTED, "values / column indices not aligned for vector loads");
    const int64_t n_int = ceildiv(n_rows - head_rows - tail_rows, 64);
    const int64_t n_bnd = ceildiv(head_rows + tail_rows, 64);
    GKOC_REQUIRE(n_int + n_bnd < (int64_t(1) << 31), GKOC_E_NOT_SUPPORTED, "more than 2^31 row segments");
    T* partial = nullptr;
    if (dot_out) {
        // one partial sum per wave (interior waves first, then the boundary waves)
        GKOC_REQUIRE(work && work_bytes >= fused_workspace_bytes(n_rows + 128, sizeof(T)), GKOC_E_WORKSPACE,
                     "workspace too small (gkoc_x_workspace_bytes(n_rows + 128))");
        partial = static_cast<T*>(work);
    }
    const dim3 grid(static_cast<unsigned>(n_int + n_bnd)), block(64);      // one segment per wave
    // the cheap gate (no agent-scope acquire for a wave that did not wait) rests on the halo lying on
    // 128-byte lines of its own: b on a line boundary and the halo at a multiple of 128 bytes behind it
    // (the documented layout: n_rows rounded up to 32 entries).  A b that is not aligned cannot have that.
    // ... and on the halo's writer being THIS device: with a peer on another device the policy is 2 until the
    // caller's self-check on that communicator has passed (common.hpp gate_fence_policy)
    const int gate_fence = std::max(
        gate_fence_policy(),
        (tune_value(GKOC_TUNE_GATE_FENCE) != 0 || reinterpret_cast<uintptr_t>(b) % 128 != 0) ? 1 : 0);
    // where in the grid the boundary waves sit: GKOC_TUNE_GATE_POS per cent of the interior waves
    // in front of them (100 = they are the last waves)
    int64_t pos = tune_value(GKOC_TUNE_GATE_POS);
    if (pos < 0 || pos > 100) pos = 100;
    const int64_t bnd_first = pos >= 100 ? -1 : n_int * pos / 100;
    // load layout: the two-entry loads with three groups in flight of the full-size kernel also for a
    // rank's share of a strong-scaling run (30 000 waves, 130 us: 2 us per product faster than one
    // 32-byte load per lane and stream, profiles/r04_dist_sim_variants.txt); GKOC_TUNE_CSR_LOAD_GROUPS = 1
    // selects the other
    const bool wide = tune_value(GKOC_TUNE_CSR_LOAD_GROUPS) == 1;
    // mode: GATE | one segment per wave (0x11000), | 0x40 with the dot product
    auto launch = [&](auto mode) {
        auto go = [&](auto e, auto u) {
            csr_spmv_pipe3_kernel<T, I, false, 64, decltype(e)::value, decltype(u)::value, lay::RINGV, 1,
                                  decltype(mode)::value><<<grid, block, 0, as_stream(s)>>>(
                n_rows, n_int + n_bnd, 1, row_ptrs, col_idxs, vals, b, 1, c, 1, 1, nullptr, nullptr, partial, 0,
                nullptr, nullptr, head_rows, tail_rows, gate, epoch, bnd_ptrs, bnd_cols, bnd_vals, fork_word,
                fork_number, gate_fence, bnd_first);
        };
        if (wide) {
            go(int_c<lay::EV>{}, int_c<1>{});
        } else {
            go(int_c<lay::PE>{}, int_c<lay::PU>{});
        }
    };
    if (dot_out) {
        launch(int_c<0x11040>{});
    } else {
        launch(int_c<0x11000>{});
    }
    GKOC_LAUNCH_OK();
    if (dot_out) {
        // ONE fold launch whatever the count (<= 2^31 / 64 partial sums would still be one block's
        // loop; a rank's share has some 30 000): fixed tree, the value does not depend on timing
        fold_partials_wide_kernel<T><<<dim3(1), dim3(fold_block), 0, as_stream(s)>>>(n_int + n_bnd, partial,
                                                                                      dot_out);
        GKOC_LAUNCH_OK();
    }
    return GKOC_OK;
}

// Diagnostic: `blocks` workgroups of `threads` threads and `lds_bytes` of LDS each that stay on
// the device for `usec` microseconds (tests: a late exchange, an RCCL-sized kernel that must find
// room next to waiting waves)
__global__ void delay_kernel(long long ticks)
{
    extern __shared__ char delay_lds[];
    if (threadIdx.x == 0) delay_lds[0] = 0;
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
}

// Mixed precision: values stored as V (float), vectors and arithmetic T (double).  8 instead of
// 12 bytes per stored entry; the result has the bits of the T kernel on the widened values.
// Columns one after the other (the matrix is streamed once per column).
template <typename T, typename V, typename I, bool ADV>
int launch_csr_mixed(gkoc_stream_t s, int64_t n_rows, int64_t n_cols, const T* alpha, const I* row_ptrs,
                     const I* col_idxs, const V* vals, const T* b, int64_t ldb, const T* beta, T* c, int64_t ldc,
                     int64_t nrhs)
{
    GKOC_REQUIRE(n_rows >= 0 && n_cols >= 0 && nrhs >= 0, GKOC_E_INVALID, "negative dimension");
    if (n_rows == 0 || nrhs == 0) return GKOC_OK;
    GKOC_REQUIRE(row_ptrs && c, GKOC_E_INVALID, "null pointer");
    GKOC_REQUIRE(ldc >= nrhs && (n_cols == 0 || ldb >= nrhs), GKOC_E_INVALID, "stride smaller than nrhs");
    if (ADV) GKOC_REQUIRE(alpha && beta, GKOC_E_INVALID, "null alpha/beta");
    using lay = pipe_layout<T>;
    segment_plan p;
    GKOC_TRY(plan_segments(n_rows, &p));
    const dim3 grid(static_cast<unsigned>(p.n_waves)), block(64);
    // four entries per lane and load (16 B of values, 16 B of columns); eight need 129 VGPRs
    // (three waves per SIMD)
    const bool vec_ok = streams_aligned(vals, col_idxs, lay::EV);
    with_store_mode(p.spw, [&](auto mode) {
        auto launch = [&](auto e, auto u) {
            csr_spmv_pipe3_kernel<T, I, ADV, 64, decltype(e)::value, decltype(u)::value, lay::RINGV, 1,
                                  decltype(mode)::value, V><<<grid, block, 0, as_stream(s)>>>(
                n_rows, p.n_seg, p.spw, row_ptrs, col_idxs, vals, b, ldb, c, ldc, static_cast<int>(nrhs), alpha,
                beta, nullptr, 0);
        };
        if (vec_ok) {
            // (round 3: 2 x 1, 2 x 2, 1 x 2, 1 x 4, 4 x 2 entries x groups all lose, 1000 - 1440 us
            // against 879)
            launch(int_c<lay::EV>{}, int_c<1>{});
        } else {
            launch(int_c<1>{}, int_c<4>{});
        }
    });
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

// c = A b and dot_out = <b, c> in one pass over the matrix (square A, one
// right-hand side, unit strides): every wave also emits its part of the dot
// product, a fixed two-level fold adds them up
template <typename T, typename I>
int launch_csr_dot(gkoc_stream_t s, int64_t n, const I* row_ptrs, const I* col_idxs, const T* vals, const T* b, T* c,
                   T* dot_out, void* work, size_t work_bytes)
{
    GKOC_REQUIRE(n >= 0, GKOC_E_INVALID, "negative dimension");
    GKOC_REQUIRE(dot_out, GKOC_E_INVALID, "null result");
    if (n == 0) {
        GKOC_HIP(hipMemsetAsync(dot_out, 0, sizeof(T), as_stream(s)));
        return GKOC_OK;
    }
    GKOC_REQUIRE(row_ptrs && b && c && work, GKOC_E_INVALID, "null pointer");
    GKOC_REQUIRE(work_bytes >= fused_workspace_bytes(n, sizeof(T)), GKOC_E_WORKSPACE,
                 "workspace too small (gkoc_x_workspace_bytes)");
    // a matrix with rows far beyond the rest: the product with its long rows spread over many workgroups
    // (csr_long_rows.hpp), then the dot product as a pass of its own - the fusion saves one pass over two
    // vectors, a hub row summed by one wave costs milliseconds
    csr_structure_lease lease;
    csr_long_info lng;
    if (tune_value(GKOC_TUNE_CSR_LONG_ROWS) != 0) {
        GKOC_TRY(csr_long_info_for(lease, as_stream(s), n, row_ptrs, &lng));
        if (lng.count > 0) {
            lease.give_back();      // (launch_csr takes its own, and the mutex is not recursive)
            GKOC_TRY((launch_csr<T, I, false>(s, n, n, nullptr, row_ptrs, col_idxs, vals, b, 1, nullptr, c, 1, 1)));
            if constexpr (std::is_same<T, double>::value) {
                return gkoc_dense_compute_dot_f64(s, n, 1, b, 1, c, 1, dot_out, work, work_bytes);
            } else {
                return gkoc_dense_compute_dot_f32(s, n, 1, b, 1, c, 1, dot_out, work, work_bytes);
            }
        }
    }
    // one segment per wave below 4 M rows, as in the plain kernel (a rank's share of a
    // strong-scaling run is that small: 2.1 M rows at 8 ranks, 255 -> 24x us per CG iteration)
    using lay = pipe_layout<T>;
    // (GKOC_TUNE_CSR_SEGS_PER_WAVE forces one or two here as in the plain product; the workspace has a slot per
    // segment, so either fits, and both kernels below take their waves and dot_partial slots from the same p)
    segment_plan p;
    GKOC_TRY(plan_segments(n, &p, tune_value(GKOC_TUNE_CSR_SEGS_PER_WAVE)));
    T* partial = static_cast<T*>(work);
    T* scratch = partial + (fused_workspace_bytes(n, sizeof(T)) / sizeof(T) - fold_chunks);
    const dim3 grid(static_cast<unsigned>(p.n_waves)), block(64);
    const bool vec_ok = streams_aligned(vals, col_idxs, 4);      // (for four entries whatever the type)
    const int xcd_map = (tune_value(GKOC_TUNE_CSR_XCD_MAP) == 1 && p.n_waves >= 8 * 1024) ? 1 : 0;
    // the column-offset plan, where EVERY segment is eligible (a wave's part of <b, c> comes from one kernel)
    // (no hub rows here: lng.count is 0)
    offsets_plan* plan = offsets_plan_of(lease, as_stream(s), n, n, row_ptrs, col_idxs, vals, b, lng);
    if constexpr (std::is_same<I, int32_t>::value) {
        if (plan != nullptr && plan->skip == nullptr) {
            launch_offsets_kernel<T, false, true>(as_stream(s), *plan, p, n, n, static_cast<const T*>(nullptr),
                                                  row_ptrs, vals, b, static_cast<const T*>(nullptr), c, partial);
            GKOC_LAUNCH_OK();
            ++plan->products;
            return fold_partials<T>(s, p.n_waves, partial, scratch, dot_out, false);
        }
    }
    lease.give_back();      // (nothing cached is read below)
    // four waves per SIMD, like the plain product: the dot's registers (and, since round 6, the loop over runs
    // of unflagged segments) had taken the double / int32 kernel to 133 VGPRs = three waves - 985 -> 1107 us on
    // L256 (profiles/r06/r06_bench_kernel_stats_regression.csv); with the bound the compiler stays at 128
    constexpr int DOT_WPS = sizeof(I) == 4 ? 4 : 1;      // (64-bit indices: 161 VGPRs, the bound would spill)
    with_store_mode(p.spw, [&](auto mode) {
        auto launch = [&](auto e, auto u) {
            // (mode | 0x40: every wave also emits its part of <b, c>)
            csr_spmv_pipe3_kernel<T, I, false, 64, decltype(e)::value, decltype(u)::value, 1024, DOT_WPS,
                                  (decltype(mode)::value | 0x40)><<<grid, block, 0, as_stream(s)>>>(
                n, p.n_seg, p.spw, row_ptrs, col_idxs, vals, b, 1, c, 1, 1, nullptr, nullptr, partial, xcd_map);
        };
        if (vec_ok) {
            launch(int_c<lay::PE>{}, int_c<lay::PU>{});
        } else {
            launch(int_c<1>{}, int_c<4>{});
        }
    });
    GKOC_LAUNCH_OK();
    return fold_partials<T>(s, p.n_waves, partial, scratch, dot_out, false);
}

}  // namespace

// Complex values (round 6).  The product of round 5 was one thread per row walking global memory: 15.0 ms on
// the 27-pt 256^3 matrix with complex<double> values = 0.63 TB/s, 78 % of a CbGmres<complex<double>> iteration
// (profiles/r06/r06_cb_gmres_complex_kernel_stats.csv).  The row-segment kernel is a template on the value
// type and needs nothing a complex value does not have: products (textbook expression) go to the LDS ring as
// 16 / 8-byte entries, lane = row adds them in k order - y(row) = sum_k a(row, k) b(col_k) in the reference's
// order, (alpha a) b on top of beta y for the advanced form (reference/matrix/csr_kernels.cpp:53-112).
// One entry per lane and load for complex<double> (16-byte value loads, four load groups in flight), two for
// complex<float>; 8 KB ring.  Several right-hand sides: one pass per column (the kernel's nrhs loop).
template <typename T, typename I>
int csr_spmv_complex(gkoc_stream_t s, int64_t n_rows, int64_t nrhs, const I* row_ptrs, const I* col_idxs,
                     const T* vals, const T* alpha, const T* b, int64_t ldb, const T* beta, T* c, int64_t ldc)
{
    if (n_rows <= 0 || nrhs <= 0) return GKOC_OK;
    GKOC_REQUIRE(row_ptrs && c, GKOC_E_INVALID, "null pointer");
    GKOC_REQUIRE(nrhs <= 0x7fffffff, GKOC_E_NOT_SUPPORTED, "more than 2^31 right-hand sides");
    // a matrix without entries or without columns (the non-local part of a rank that has no neighbours) comes
    // with null arrays / a null b: the thread-per-row kernel never touches them, this one's idle lanes read b[0]
    if (col_idxs == nullptr || vals == nullptr || b == nullptr) return GKOC_E_NOT_SUPPORTED;
    constexpr int E = sizeof(T) == 16 ? 1 : 2, U = sizeof(T) == 16 ? 4 : 2;
    if (!streams_aligned(vals, col_idxs, E) || reinterpret_cast<uintptr_t>(b) % sizeof(T) != 0 ||
        reinterpret_cast<uintptr_t>(c) % sizeof(T) != 0) {
        return GKOC_E_NOT_SUPPORTED;
    }
    segment_plan p;
    GKOC_TRY(plan_segments(n_rows, &p));
    const dim3 grid(static_cast<unsigned>(p.n_waves)), block(64);
    // four waves per SIMD where the kernel is within a few registers of it (complex<double>, 32-bit indices: 132)
    constexpr int CX_WPS = sizeof(I) == 4 ? 4 : 1;
    if (alpha != nullptr) GKOC_REQUIRE(beta != nullptr, GKOC_E_INVALID, "alpha and beta go together");
    with_store_mode(p.spw, [&](auto mode) {
        auto launch = [&](auto advanced) {
            constexpr bool ADV = decltype(advanced)::value;
            csr_spmv_pipe3_kernel<T, I, ADV, 64, E, U, pipe_layout<T>::RINGV, (ADV ? 1 : CX_WPS),
                                  decltype(mode)::value><<<grid, block, 0, as_stream(s)>>>(
                n_rows, p.n_seg, p.spw, row_ptrs, col_idxs, vals, b, ldb, c, ldc, static_cast<int>(nrhs), alpha,
                beta);
        };
        if (alpha != nullptr) {
            launch(std::true_type{});
        } else {
            launch(std::false_type{});
        }
    });
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}
#define GKOC_INST_CX(T, I)                                                                                       \
    template int csr_spmv_complex<T, I>(gkoc_stream_t, int64_t, int64_t, const I*, const I*, const T*, const T*, \
                                        const T*, int64_t, const T*, T*, int64_t);
GKOC_INST_CX(gkoc_c128, int32_t)
GKOC_INST_CX(gkoc_c128, int64_t)
GKOC_INST_CX(gkoc_c64, int32_t)
GKOC_INST_CX(gkoc_c64, int64_t)
#undef GKOC_INST_CX

}  // namespace gkoc

using namespace gkoc;

#define GKOC_DEF_CSR(T, TN, I, IN)                                                                                  \
    extern "C" int gkoc_csr_spmv_##TN##_##IN(gkoc_stream_t s, int64_t n_rows, int64_t n_cols, const I* row_ptrs,       \
                                             const I* col_idxs, const T* vals, const T* b, int64_t ldb, T* c,          \
                                             int64_t ldc, int64_t nrhs)                                                \
    {                                                                                                                  \
        return launch_csr<T, I, false>(s, n_rows, n_cols, nullptr, row_ptrs, col_idxs, vals, b, ldb, nullptr, c, ldc,  \
                                       nrhs);                                                                          \
    }                                                                                                                  \
    extern "C" int gkoc_csr_advanced_spmv_##TN##_##IN(                                                                 \
        gkoc_stream_t s, int64_t n_rows, int64_t n_cols, const T* alpha, const I* row_ptrs, const I* col_idxs,         \
        const T* vals, const T* b, int64_t ldb, const T* beta, T* c, int64_t ldc, int64_t nrhs)                        \
    {                                                                                                                  \
        return launch_csr<T, I, true>(s, n_rows, n_cols, alpha, row_ptrs, col_idxs, vals, b, ldb, beta, c, ldc, nrhs); \
    }                                                                                                                  \
    extern "C" int gkoc_x_csr_spmv_dot_##TN##_##IN(gkoc_stream_t s, int64_t n, const I* row_ptrs, const I* col_idxs,   \
                                                   const T* vals, const T* b, T* c, T* dot_out, void* work,            \
                                                   size_t work_bytes)                                                  \
    {                                                                                                                  \
        return launch_csr_dot<T, I>(s, n, row_ptrs, col_idxs, vals, b, c, dot_out, work, work_bytes);                  \
    }

GKOC_DEF_CSR(double, f64, int32_t, i32)
GKOC_DEF_CSR(double, f64, int64_t, i64)
GKOC_DEF_CSR(float, f32, int32_t, i32)
GKOC_DEF_CSR(float, f32, int64_t, i64)

#define GKOC_DEF_CSR_GATED(T, TN, I, IN)                                                             \
    extern "C" int gkoc_csr_spmv_gated_##TN##_##IN(                                                   \
        gkoc_stream_t s, int64_t n_rows, const I* row_ptrs, const I* col_idxs, const T* vals,         \
        const I* bnd_ptrs, const I* bnd_cols, const T* bnd_vals, const T* b, T* c, int64_t head_rows, \
        int64_t tail_rows, const uint32_t* gate, uint32_t epoch, uint32_t* fork_word,                 \
        uint32_t fork_number)                                                                         \
    {                                                                                                 \
        return launch_csr_gated<T, I>(s, n_rows, row_ptrs, col_idxs, vals, bnd_ptrs, bnd_cols,        \
                                      bnd_vals, b, c, head_rows, tail_rows, gate, epoch, fork_word,   \
                                      fork_number);                                                   \
    }
GKOC_DEF_CSR_GATED(double, f64, int32_t, i32)
GKOC_DEF_CSR_GATED(double, f64, int64_t, i64)
GKOC_DEF_CSR_GATED(float, f32, int32_t, i32)
GKOC_DEF_CSR_GATED(float, f32, int64_t, i64)

#define GKOC_DEF_CSR_GATED_DOT(T, TN, I, IN)                                                         \
    extern "C" int gkoc_x_csr_spmv_gated_dot_##TN##_##IN(                                             \
        gkoc_stream_t s, int64_t n_rows, const I* row_ptrs, const I* col_idxs, const T* vals,         \
        const I* bnd_ptrs, const I* bnd_cols, const T* bnd_vals, const T* b, T* c, int64_t head_rows, \
        int64_t tail_rows, const uint32_t* gate, uint32_t epoch, uint32_t* fork_word,                 \
        uint32_t fork_number, T* dot_out, void* work, size_t work_bytes)                              \
    {                                                                                                 \
        GKOC_REQUIRE(dot_out, GKOC_E_INVALID, "null result");                                         \
        return launch_csr_gated<T, I>(s, n_rows, row_ptrs, col_idxs, vals, bnd_ptrs, bnd_cols,        \
                                      bnd_vals, b, c, head_rows, tail_rows, gate, epoch, fork_word,   \
                                      fork_number, dot_out, work, work_bytes);                        \
    }
GKOC_DEF_CSR_GATED_DOT(double, f64, int32_t, i32)
GKOC_DEF_CSR_GATED_DOT(double, f64, int64_t, i64)
GKOC_DEF_CSR_GATED_DOT(float, f32, int32_t, i32)
GKOC_DEF_CSR_GATED_DOT(float, f32, int64_t, i64)

extern "C" int gkoc_csr_spmv_gated_fits(int64_t n_rows, int64_t head_rows, int64_t tail_rows)
{
    return gkoc::gated_fits(n_rows, head_rows, tail_rows) ? 1 : 0;
}

extern "C" int gkoc_gate_open(gkoc_stream_t s, uint32_t* gate, uint32_t epoch)
{
    GKOC_REQUIRE(gate, GKOC_E_INVALID, "gate == NULL");
    gkoc::gate_open_kernel<<<dim3(1), dim3(1), 0, as_stream(s)>>>(gate, epoch);
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

extern "C" int gkoc_debug_delay(gkoc_stream_t s, int64_t usec, int blocks, int threads, int lds_bytes)
{
    GKOC_REQUIRE(usec >= 0 && blocks > 0 && threads > 0 && threads <= 1024 && lds_bytes >= 0 &&
                     lds_bytes <= 64 * 1024,
                 GKOC_E_INVALID, "bad delay arguments");
    /* wall_clock64 counts at 100 MHz on gfx950 */                                                    
    gkoc::delay_kernel<<<dim3(unsigned(blocks)), dim3(unsigned(threads)), size_t(lds_bytes), as_stream(s)>>>(
        (long long)usec * 100);
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

#define GKOC_DEF_CSR_MIXED(I, IN)                                                                                  \
    extern "C" int gkoc_csr_spmv_f32_f64_##IN(gkoc_stream_t s, int64_t n_rows, int64_t n_cols, const I* row_ptrs,      \
                                              const I* col_idxs, const float* vals, const double* b, int64_t ldb,      \
                                              double* c, int64_t ldc, int64_t nrhs)                                    \
    {                                                                                                                  \
        return launch_csr_mixed<double, float, I, false>(s, n_rows, n_cols, nullptr, row_ptrs, col_idxs, vals, b, ldb, \
                                                         nullptr, c, ldc, nrhs);                                       \
    }                                                                                                                  \
    extern "C" int gkoc_csr_advanced_spmv_f32_f64_##IN(                                                                \
        gkoc_stream_t s, int64_t n_rows, int64_t n_cols, const double* alpha, const I* row_ptrs, const I* col_idxs,    \
        const float* vals, const double* b, int64_t ldb, const double* beta, double* c, int64_t ldc, int64_t nrhs)     \
    {                                                                                                                  \
        return launch_csr_mixed<double, float, I, true>(s, n_rows, n_cols, alpha, row_ptrs, col_idxs, vals, b, ldb,    \
                                                        beta, c, ldc, nrhs);                                           \
    }
GKOC_DEF_CSR_MIXED(int32_t, i32)
GKOC_DEF_CSR_MIXED(int64_t, i64)

extern "C" size_t gkoc_x_workspace_bytes(int64_t n, size_t value_size)
{
    return gkoc::fused_workspace_bytes(n < 0 ? 0 : n, value_size);
}
