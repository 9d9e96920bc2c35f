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
#include <algorithm>
#include <atomic>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>
#include <type_traits>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "common.hpp"
#include "csr_long_rows.hpp"
#include "csr_offsets.hpp"
#include "csr_spmv_multi.hpp"
#include "csr_spmv_pipe.hpp"
#include "fused.hpp"

namespace gkoc {
namespace {

// ---- which 64-row segments of a matrix hold a row beyond GKOC_CSR_LONG_ROW (csr_long_rows.hpp) --------
// Found by one scan of the row pointers the first time a (device, row_ptrs, n_rows) is multiplied, kept
// here (flags and list read-only from then on; the chunk sums of a product go to a buffer per (matrix, stream),
// so products of one matrix on several streams share nothing that is written); gkoc_free forgets the entries of
// a pointer that goes away (csr_long_rows_forget).  A few dozen matrices at most: the OLDEST entry makes room,
// after a device synchronisation (a product on any stream may still read its flags).  The first product of a
// matrix therefore synchronises its stream once (the scan's answer is needed on the host) - documented in
// gko_cdna4.h; inside a stream capture the matrix is multiplied by the row-segment kernel alone.
std::mutex g_long_mtx;
struct long_entry {
    csr_long_info info;
    // one buffer of chunk sums per stream that has multiplied this matrix (count x 8 x 64 values of 8 bytes)
    std::vector<std::pair<hipStream_t, void*>> partials;
};
std::map<std::tuple<int, const void*, int64_t>, long_entry> g_long_cache;
std::atomic<int> g_long_cached{0};
constexpr size_t long_cache_cap = 128;
constexpr int64_t long_list_cap = 4096;      // more flagged segments than this: the matrix has no "few long rows"

thread_local bool t_long_releasing = false;      // gkoc_free below comes back through csr_long_rows_forget

void long_info_release(long_entry& en)
{
    csr_long_info& f = en.info;
    t_long_releasing = true;
    if (f.bits) (void)gkoc_free(f.bits);
    if (f.list) (void)gkoc_free(f.list);
    for (auto& sp : en.partials) (void)gkoc_free(sp.second);
    en.partials.clear();
    f = csr_long_info{};
    t_long_releasing = false;
}

bool stream_is_capturing(hipStream_t st)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        return true;
    }
    return false;
}

// the calling stream's buffer of chunk sums (allocated the first time the stream multiplies the matrix; not
// inside a stream capture: the product is then left to the row-segment kernel alone, which handles any row)
void long_partial_for(long_entry& en, hipStream_t st, csr_long_info* out)
{
    *out = en.info;
    if (en.info.count <= 0) return;
    for (auto& sp : en.partials) {
        if (sp.first == st) {
            out->partial = sp.second;
            return;
        }
    }
    void* p = nullptr;
    if (stream_is_capturing(st) ||
        gkoc_malloc(&p, size_t(en.info.count) * LONG_MAX_PER_SEG * LONG_PARTS * 8) != GKOC_OK) {
        (void)hipGetLastError();
        *out = csr_long_info{};
        out->nnz = en.info.nnz;
        return;
    }
    en.partials.emplace_back(st, p);
    out->partial = p;
}

template <typename T, typename I>
int long_info_of(gkoc_stream_t s, int64_t n_rows, const I* row_ptrs, csr_long_info* out)
{
    int dev = 0;
    GKOC_HIP(hipGetDevice(&dev));
    const auto key = std::make_tuple(dev, static_cast<const void*>(row_ptrs), n_rows);
    std::lock_guard<std::mutex> g(g_long_mtx);
    auto it = g_long_cache.find(key);
    if (it != g_long_cache.end()) {
        long_partial_for(it->second, as_stream(s), out);
        return GKOC_OK;
    }
    // a stream that is being captured into a hipGraph cannot be synchronised: a matrix first seen there is
    // multiplied by the row-segment kernel alone (correct for any row), and looked at on its next product
    if (stream_is_capturing(as_stream(s))) {
        *out = csr_long_info{};
        return GKOC_OK;
    }
    if (g_long_cache.size() >= long_cache_cap) {
        auto oldest = g_long_cache.begin();
        for (auto jt = g_long_cache.begin(); jt != g_long_cache.end(); ++jt) {
            if (jt->second.info.seq < oldest->second.info.seq) oldest = jt;
        }
        if (oldest->second.info.count > 0) GKOC_HIP(hipDeviceSynchronize());   // (a product in flight may use it)
        long_info_release(oldest->second);
        g_long_cache.erase(oldest);
    }
    csr_long_info f;
    static uint64_t arrivals = 0;
    f.seq = ++arrivals;
    const int64_t n_seg = ceildiv(n_rows, int64_t(64));
    const size_t bit_bytes = size_t(ceildiv(n_seg, int64_t(32))) * 4;
    const size_t list_bytes = size_t(1 + long_list_cap) * 8;
    void *bits = nullptr, *list = nullptr;
    GKOC_TRY(gkoc_malloc(&bits, bit_bytes));
    if (gkoc_malloc(&list, list_bytes) != GKOC_OK) {
        t_long_releasing = true;
        (void)gkoc_free(bits);
        t_long_releasing = false;
        return GKOC_E_INVALID;
    }
    hipStream_t st = as_stream(s);
    unsigned long long count = 0;
    I nnz_dev = I(0);
    bool ok = hipMemsetAsync(bits, 0, bit_bytes, st) == hipSuccess && hipMemsetAsync(list, 0, 8, st) == hipSuccess;
    if (ok) {
        csr_long_row_scan_kernel<I><<<dim3(unsigned(ceildiv(n_seg, int64_t(4)))), dim3(256), 0, st>>>(
            n_rows, row_ptrs, static_cast<uint32_t*>(bits), static_cast<unsigned long long*>(list), long_list_cap);
        // (the number of stored entries comes with the same wait: the launcher sizes a wave's share by it)
        ok = hipGetLastError() == hipSuccess &&
             hipMemcpyAsync(&count, list, 8, hipMemcpyDeviceToHost, st) == hipSuccess &&
             hipMemcpyAsync(&nnz_dev, row_ptrs + n_rows, sizeof(I), hipMemcpyDeviceToHost, st) == hipSuccess &&
             hipStreamSynchronize(st) == hipSuccess;
    }
    if (ok) f.nnz = int64_t(nnz_dev);
    if (!ok || count == 0 || int64_t(count) > long_list_cap) {
        // none (the common case), or so many that "a few long rows" is not what this matrix has: the
        // row-segment kernel does everything, as before
        (void)hipGetLastError();
        t_long_releasing = true;
        (void)gkoc_free(bits);
        (void)gkoc_free(list);
        t_long_releasing = false;
    } else {
        f.count = int64_t(count);
        f.bits = static_cast<uint32_t*>(bits);
        f.list = static_cast<unsigned long long*>(list);
    }
    long_entry& en = g_long_cache[key];
    en.info = f;
    g_long_cached.store(int(g_long_cache.size()));
    long_partial_for(en, st, out);
    return GKOC_OK;
}

}  // namespace

void csr_long_rows_forget(const void* ptr)
{
    if (ptr == nullptr || t_long_releasing || g_long_cached.load(std::memory_order_relaxed) == 0) return;
    std::vector<long_entry> gone;
    {
        std::lock_guard<std::mutex> g(g_long_mtx);
        for (auto it = g_long_cache.begin(); it != g_long_cache.end();) {
            if (std::get<1>(it->first) == ptr) {
                gone.push_back(it->second);
                it = g_long_cache.erase(it);
            } else {
                ++it;
            }
        }
        g_long_cached.store(int(g_long_cache.size()));
    }
    for (auto& en : gone) {
        if (en.info.count > 0) (void)hipDeviceSynchronize();      // a product in flight may still use its buffers
        long_info_release(en);
    }
}

std::atomic<int> g_csr_offsets_cached{0};

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

// ---- cached per-segment column offsets (csr_offsets.hpp) ---------------------------------------------------
// A derived, read-only description of (row_ptrs, col_idxs), keyed by (device, row_ptrs, col_idxs, n_rows), in
// the style of the long-row cache above.  Only for index arrays that are live allocations of the library's own
// allocator: their addresses cannot be reused without gkoc_free seeing them.  Built by the SECOND product on the
// same arrays (a one-shot product never pays; GKOC_TUNE_CSR_OFFSETS = 1: by the first, 2: never), never inside a
// stream capture (the product takes the row-segment kernel and the next one tries again).  Dropped by
// csr_offsets_forget: gkoc_free, every C-ABI entry that writes an index array of a CSR matrix, gkoc_memcpy_h2d /
// _d2d into one, gkoc_csr_structure_changed.  Lookup and launch happen under the mutex, so a plan cannot be
// released between the two; its buffers are released after a device synchronisation.
std::mutex g_off_mtx;
struct offsets_plan {
    int state = 0;                  // 0: seen once, 1: in use, 2: rejected (fewer than half of the segments eligible)
    int64_t n_seg = 0, eligible = 0;
    int max_d = 0;                  // the largest D of a segment: picks the product kernel's diagonal slots
    int64_t n_classes = 0;          // distinct (table, masks) among the segments (csr_offsets.hpp)
    int64_t nnz = 0;                // stored entries when the plan was built: sizes the product (offsets_nt_min_bytes)
    int32_t* seg_class = nullptr;   // device: the class id of every segment
    int32_t* cls_tab = nullptr;     // device: OFFS_TAB int32 per class
    uint32_t* cls_mask = nullptr;   // device: 64 words per class, one per row of a segment
    uint32_t* skip = nullptr;       // device: bit per segment the row-segment kernel leaves out (eligible | long-flagged)
    bool with_long = false;         // skip holds the long-row flags too
    int64_t bytes = 0, products = 0;
    uint64_t seq = 0;
    size_t rp_bytes = 0, ci_bytes = 0;      // the two allocations the plan describes (csr_offsets_forget)
};
using offsets_key = std::tuple<int, const void*, const void*, int64_t>;
std::map<offsets_key, offsets_plan> g_off_cache;
constexpr size_t offsets_cache_cap = 128;
// at least this share of the segments must be eligible, in per cent (docs/KERNELS.md: measured on a stencil
// whose every other segment is not)
constexpr int64_t offsets_min_share = 50;
// the MI355X's Infinity Cache, 256 MiB: a product that streams more than this per call cannot live in it, and its
// value stream and result bypass it (measured on both sides of it: docs/KERNELS.md 36)
constexpr int64_t offsets_nt_min_bytes = int64_t(256) << 20;

// buffers of dropped plans that could not be released at once (inside a stream capture the device cannot be
// synchronised): released with the next plan that goes.  Guarded by g_off_mtx.
std::vector<void*> g_off_graveyard;

// Only plans that HAVE buffers pay the synchronisation (a product in flight on any stream may still read them):
// matrices that were multiplied through a plan, as with the long-row cache above.
void offsets_release(std::vector<offsets_plan>& gone)
{
    std::vector<void*> bufs;
    for (auto& pl : gone) {
        for (void* b : {static_cast<void*>(pl.seg_class), static_cast<void*>(pl.cls_tab),
                        static_cast<void*>(pl.cls_mask), static_cast<void*>(pl.skip)}) {
            if (b) bufs.push_back(b);
        }
    }
    if (bufs.empty()) return;
    std::lock_guard<std::mutex> g(g_off_mtx);
    g_off_graveyard.insert(g_off_graveyard.end(), bufs.begin(), bufs.end());
    if (hipDeviceSynchronize() != hipSuccess) {
        (void)hipGetLastError();      // (a capture is under way: they wait in the graveyard)
        return;
    }
    for (void* b : g_off_graveyard) (void)arena_free(b);
    g_off_graveyard.clear();
}

// scratch of the class search for n segments, in bytes, and where its parts lie
struct class_scratch {
    size_t hash, hash_sorted, ids, ids_sorted, leader, is_new, class_at, prim, prim_bytes, total;
};
class_scratch class_scratch_of(int64_t n)
{
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    size_t sort_bytes = 0, scan_bytes = 0;
    unsigned long long* k = nullptr;
    uint32_t* v = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, sort_bytes, k, k, v, v, size_t(n), 0, 64, hipStream_t(nullptr));
    (void)rocprim::exclusive_scan(nullptr, scan_bytes, v, v, uint32_t(0), size_t(n), rocprim::plus<uint32_t>(),
                                  hipStream_t(nullptr));
    class_scratch c;
    size_t at = 0;
    auto part = [&](size_t bytes) {
        const size_t here = at;
        at += up(bytes);
        return here;
    };
    c.hash = part(size_t(n) * 8);
    c.hash_sorted = part(size_t(n) * 8);
    c.ids = part(size_t(n) * 4);
    c.ids_sorted = part(size_t(n) * 4);
    c.leader = part(size_t(n) * 4);
    c.is_new = part(size_t(n) * 4);
    c.class_at = part(size_t(n) * 4);
    c.prim_bytes = sort_bytes > scan_bytes ? sort_bytes : scan_bytes;
    c.prim = part(c.prim_bytes);
    c.total = at;
    return c;
}

// The analysis.  One pass over the column indices gives the per-segment tables and the per-row masks; behind it,
// on the same stream, the class search of csr_offsets.hpp (hash, stable sort of (hash, segment), compare with the
// run's leader, scan).  The eligible count, the largest D and the number of classes come back with ONE stream
// synchronisation.  An accepted plan is then compacted - a class id per segment, a table and 64 masks per class,
// sized by the count - and the per-segment tables, the per-row masks and the scratch are freed behind a second,
// short synchronisation (the compaction reads them): what a plan keeps is 4 n_seg + 388 n_classes bytes
// (+ the skip bits), 1 MiB for the 27-point stencil 256^3 where tables and masks were 97 MiB.
int offsets_build(hipStream_t st, int64_t n_rows, const int32_t* row_ptrs, const int32_t* col_idxs,
                  const csr_long_info& lng, offsets_plan& pl)
{
    const int64_t n_seg = ceildiv(n_rows, int64_t(64));
    const size_t tab_bytes = size_t(n_seg) * OFFS_TAB * 4, mask_bytes = size_t(n_rows) * 4;
    const size_t skip_bytes = size_t(ceildiv(n_seg, int64_t(32))) * 4;
    const size_t ids_bytes = size_t(n_seg) * 4;
    const class_scratch cs = class_scratch_of(n_seg);
    // (cut to its low bits only to provoke collisions: the tests of the compare-with-the-leader path)
    const int64_t hash_bits = tune_value(GKOC_TUNE_CSR_OFFSETS_HASH_BITS);
    const unsigned long long keep = (hash_bits < 0 || hash_bits >= 64) ? ~0ull : ((1ull << hash_bits) - 1ull);
    void *tab = nullptr, *mask = nullptr, *skip = nullptr, *count_dev = nullptr, *ids = nullptr, *work = nullptr;
    void *ctab = nullptr, *cmask = nullptr;
    bool ok = n_seg > 0 && arena_malloc(&tab, tab_bytes, GKOC_MEM_INDICES) == GKOC_OK &&
              arena_malloc(&mask, mask_bytes, GKOC_MEM_INDICES) == GKOC_OK &&
              arena_malloc(&skip, skip_bytes, GKOC_MEM_INDICES) == GKOC_OK &&
              arena_malloc(&ids, ids_bytes, GKOC_MEM_INDICES) == GKOC_OK &&
              arena_malloc(&work, cs.total, GKOC_MEM_INDICES) == GKOC_OK &&
              arena_malloc(&count_dev, 32, GKOC_MEM_VECTOR) == GKOC_OK;
    char* w = static_cast<char*>(work);
    auto at = [&](size_t off) { return static_cast<void*>(w + off); };
    const dim3 seg_grid(unsigned(ceildiv(n_seg, int64_t(4)))), seg_block(256);
    unsigned long long count[4] = {0, 0, 0, 0};
    if (ok) {
        const int32_t* tab_c = static_cast<const int32_t*>(tab);
        const uint32_t* mask_c = static_cast<const uint32_t*>(mask);
        csr_offsets_build_kernel<int32_t><<<seg_grid, seg_block, 0, st>>>(
            n_rows, row_ptrs, col_idxs, static_cast<int32_t*>(tab), static_cast<uint32_t*>(mask));
        csr_offsets_finish_kernel<<<dim3(1), dim3(1024), 0, st>>>(
            n_seg, tab_c, lng.count > 0 ? lng.bits : nullptr, static_cast<uint32_t*>(skip),
            static_cast<unsigned long long*>(count_dev));
        csr_offsets_hash_kernel<<<seg_grid, seg_block, 0, st>>>(
            n_rows, n_seg, tab_c, mask_c, keep, static_cast<unsigned long long*>(at(cs.hash)),
            static_cast<uint32_t*>(at(cs.ids)));
        size_t prim_bytes = cs.prim_bytes;
        ok = hipGetLastError() == hipSuccess &&
             rocprim::radix_sort_pairs(at(cs.prim), prim_bytes, static_cast<unsigned long long*>(at(cs.hash)),
                                       static_cast<unsigned long long*>(at(cs.hash_sorted)),
                                       static_cast<uint32_t*>(at(cs.ids)), static_cast<uint32_t*>(at(cs.ids_sorted)),
                                       size_t(n_seg), 0, 64, st) == hipSuccess;
        if (ok) {
            csr_offsets_leader_kernel<<<seg_grid, seg_block, 0, st>>>(
                n_rows, n_seg, tab_c, mask_c, static_cast<const unsigned long long*>(at(cs.hash_sorted)),
                static_cast<const uint32_t*>(at(cs.ids_sorted)), static_cast<uint32_t*>(at(cs.leader)),
                static_cast<uint32_t*>(at(cs.is_new)));
            prim_bytes = cs.prim_bytes;
            ok = hipGetLastError() == hipSuccess &&
                 rocprim::exclusive_scan(at(cs.prim), prim_bytes, static_cast<uint32_t*>(at(cs.is_new)),
                                         static_cast<uint32_t*>(at(cs.class_at)), uint32_t(0), size_t(n_seg),
                                         rocprim::plus<uint32_t>(), st) == hipSuccess;
        }
        if (ok) {
            csr_offsets_class_count_kernel<<<dim3(1), dim3(1), 0, st>>>(
                n_seg, static_cast<const uint32_t*>(at(cs.is_new)), static_cast<const uint32_t*>(at(cs.class_at)),
                n_rows, row_ptrs, static_cast<unsigned long long*>(count_dev));
            ok = hipGetLastError() == hipSuccess;
        }
        // (whatever was enqueued has run when the buffers are freed below, also after an error)
        const bool copied = ok && hipMemcpyAsync(count, count_dev, 32, hipMemcpyDeviceToHost, st) == hipSuccess;
        ok = hipStreamSynchronize(st) == hipSuccess && copied;
    }
    (void)hipGetLastError();
    if (count_dev) (void)arena_free(count_dev);
    pl.n_seg = n_seg;
    pl.eligible = ok ? int64_t(count[0]) : 0;
    pl.max_d = ok ? int(count[1]) : 0;
    const int64_t n_classes = ok ? int64_t(count[2]) : 0;
    const bool accepted = ok && pl.eligible > 0 && pl.eligible * 100 >= n_seg * offsets_min_share;
    bool compacted = false;
    if (accepted && n_classes >= 1 && n_classes <= n_seg &&
        arena_malloc(&ctab, size_t(n_classes) * OFFS_TAB * 4, GKOC_MEM_INDICES) == GKOC_OK &&
        arena_malloc(&cmask, size_t(n_classes) * 64 * 4, GKOC_MEM_INDICES) == GKOC_OK) {
        csr_offsets_compact_kernel<<<seg_grid, seg_block, 0, st>>>(
            n_rows, n_seg, static_cast<const int32_t*>(tab), static_cast<const uint32_t*>(mask),
            static_cast<const uint32_t*>(at(cs.ids_sorted)), static_cast<const uint32_t*>(at(cs.leader)),
            static_cast<const uint32_t*>(at(cs.is_new)), static_cast<const uint32_t*>(at(cs.class_at)),
            static_cast<int32_t*>(ids), static_cast<int32_t*>(ctab), static_cast<uint32_t*>(cmask));
        const bool launched = hipGetLastError() == hipSuccess;
        compacted = hipStreamSynchronize(st) == hipSuccess && launched;
        (void)hipGetLastError();
    }
    if (tab) (void)arena_free(tab);
    if (mask) (void)arena_free(mask);
    if (work) (void)arena_free(work);
    if (!compacted) {
        for (void* b : {skip, ids, ctab, cmask}) {
            if (b) (void)arena_free(b);
        }
        // too few eligible segments: rejected for good; an analysis that FAILED (no memory, a stream error) is
        // tried again by the next product
        if (ok && !accepted) pl.state = 2;
        return GKOC_OK;
    }
    pl.state = 1;
    pl.n_classes = n_classes;
    pl.nnz = int64_t(count[3]);
    pl.seg_class = static_cast<int32_t*>(ids);
    pl.cls_tab = static_cast<int32_t*>(ctab);
    pl.cls_mask = static_cast<uint32_t*>(cmask);
    pl.bytes = int64_t(ids_bytes) + n_classes * int64_t((OFFS_TAB + 64) * 4);
    if (pl.eligible == n_seg) {
        (void)arena_free(skip);        // every segment is this kernel's: the row-segment kernel is not launched
    } else {
        pl.skip = static_cast<uint32_t*>(skip);
        pl.with_long = lng.count > 0;
        pl.bytes += int64_t(skip_bytes);
    }
    return GKOC_OK;
}

// plans that made room in the cache while the mutex was held: released when the holder is destroyed, which the
// callers arrange to happen AFTER their lock is gone (declared in front of it)
struct evicted_plans {
    std::vector<offsets_plan> v;
    ~evicted_plans() { offsets_release(v); }
};

// The plan this product may use, or nullptr.  The caller holds g_off_mtx.
offsets_plan* offsets_plan_for(hipStream_t st, int64_t n_rows, int64_t n_cols, const int32_t* row_ptrs,
                               const int32_t* col_idxs, const csr_long_info& lng, std::vector<offsets_plan>* evicted)
{
    const int64_t mode = tune_value(GKOC_TUNE_CSR_OFFSETS);
    if (mode == 2 || row_ptrs == nullptr || col_idxs == nullptr || n_cols < 1 ||
        n_rows >= (int64_t(1) << 31) - 64 || n_cols >= (int64_t(1) << 31)) {
        return nullptr;
    }
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    const offsets_key key{dev, row_ptrs, col_idxs, n_rows};
    auto it = g_off_cache.find(key);
    if (it == g_off_cache.end()) {
        const size_t rp_bytes = arena_allocation_bytes(row_ptrs), ci_bytes = arena_allocation_bytes(col_idxs);
        if (rp_bytes == 0 || ci_bytes == 0) return nullptr;
        if (g_off_cache.size() >= offsets_cache_cap) {
            auto oldest = g_off_cache.begin();
            for (auto jt = g_off_cache.begin(); jt != g_off_cache.end(); ++jt) {
                if (jt->second.seq < oldest->second.seq) oldest = jt;
            }
            evicted->push_back(oldest->second);      // (released by the caller once the mutex is free)
            g_off_cache.erase(oldest);
        }
        static uint64_t arrivals = 0;
        offsets_plan fresh;
        fresh.seq = ++arrivals;
        fresh.rp_bytes = rp_bytes;
        fresh.ci_bytes = ci_bytes;
        it = g_off_cache.emplace(key, fresh).first;
        g_csr_offsets_cached.store(int(g_off_cache.size()));
        if (mode != 1) return nullptr;      // the first product of these arrays
    }
    offsets_plan& pl = it->second;
    if (pl.state == 0) {
        if (stream_is_capturing(st)) return nullptr;
        (void)offsets_build(st, n_rows, row_ptrs, col_idxs, lng, pl);
    }
    if (pl.state != 1) return nullptr;
    // the row-segment kernel beside this one must leave out what the plan's skip bits say, and somebody must
    // do the long-flagged segments: only with the flags the plan was built with
    if (pl.skip != nullptr && pl.with_long != (lng.count > 0)) return nullptr;
    return &pl;
}

// the product of the plan's segments: the kernel with the fewest diagonal slots (8, 16, 28 or 32) that holds the
// plan's largest D - its value stream, its stage and its x loads are sized by the slot count (one straight-line
// body per kernel, csr_offsets.hpp; a segment with fewer offsets is right in any wider kernel).  28 is the 27-point
// stencil's.
// The price: in a plan that has wide segments the narrow ones issue dead x loads - 5 % on a matrix with one
// segment of 9 offsets in eight of 3 under the 32-slot kernel, nothing with one in two (docs/KERNELS.md 36).
template <typename T, bool ADV, bool DOT, int ND>
void launch_offsets_kernel_nd(hipStream_t st, const offsets_plan& pl, const segment_plan& p, int64_t n_rows,
                              int64_t n_cols, const T* alpha, const int32_t* row_ptrs, const T* vals, const T* b,
                              const T* beta, T* c, T* dot_partial)
{
    const dim3 grid(static_cast<unsigned>(p.n_waves)), block(64);
    // values, x, c and the row pointers: what a product streams.  Above the Infinity Cache's size the values and
    // c go non-temporally (csr_offsets.hpp NT), below it repeated products are served from that cache
    const int64_t product_bytes = pl.nnz * int64_t(sizeof(T)) + (n_rows + n_cols) * int64_t(sizeof(T)) + n_rows * 4;
    if (product_bytes > offsets_nt_min_bytes) {
        csr_spmv_pipe3_kernel_offsets<T, ADV, DOT, ND, true><<<grid, block, 0, st>>>(
            int32_t(n_rows), int32_t(n_cols), p.n_seg, p.spw, row_ptrs, vals, b, c, alpha, beta, pl.seg_class,
            pl.cls_tab, pl.cls_mask, dot_partial);
    } else {
        csr_spmv_pipe3_kernel_offsets<T, ADV, DOT, ND, false><<<grid, block, 0, st>>>(
            int32_t(n_rows), int32_t(n_cols), p.n_seg, p.spw, row_ptrs, vals, b, c, alpha, beta, pl.seg_class,
            pl.cls_tab, pl.cls_mask, dot_partial);
    }
}

template <typename T, bool ADV, bool DOT>
void launch_offsets_kernel(hipStream_t st, const offsets_plan& pl, const segment_plan& p, int64_t n_rows,
                           int64_t n_cols, const T* alpha, const int32_t* row_ptrs, const T* vals, const T* b,
                           const T* beta, T* c, T* dot_partial)
{
    auto go = [&](auto nd) {
        launch_offsets_kernel_nd<T, ADV, DOT, decltype(nd)::value>(st, pl, p, n_rows, n_cols, alpha, row_ptrs, vals,
                                                                   b, beta, c, dot_partial);
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
    // rows far longer than the rest: their segments are left out here and done by many workgroups
    // (csr_long_rows.hpp); one right-hand side
    csr_long_info lng;
    if (nrhs == 1 && tune_value(GKOC_TUNE_CSR_LONG_ROWS) != 0) {
        GKOC_TRY((long_info_of<T, I>(s, n_rows, row_ptrs, &lng)));
    }
    const uint32_t* seg_skip = lng.count > 0 ? lng.bits : nullptr;
    // stencil-like structure seen before: the column-offset plan (csr_offsets.hpp) takes its eligible
    // segments, the row-segment kernel below the others.  Held to the end: a plan is not released while its
    // product is being enqueued.
    constexpr bool offsets_type = std::is_same<I, int32_t>::value && (sizeof(T) == 8 || sizeof(T) == 4);
    evicted_plans evicted;
    std::unique_lock<std::mutex> plan_lock(g_off_mtx, std::defer_lock);
    offsets_plan* plan = nullptr;
    if constexpr (offsets_type) {
        if (nrhs == 1 && ldb == 1 && ldc == 1 && vals != nullptr && b != nullptr &&
            reinterpret_cast<uintptr_t>(vals) % 16 == 0 && tune_value(GKOC_TUNE_CSR_OFFSETS) != 2) {
            plan_lock.lock();
            plan = offsets_plan_for(as_stream(s), n_rows, n_cols, row_ptrs, col_idxs, lng, &evicted.v);
            if (plan == nullptr) plan_lock.unlock();
        }
    }
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
int launch_csr(gkoc_stream_t s, int64_t n_rows, int64_t n_cols, const T* alpha,
               const I* row_ptrs, const I* col_idxs, const T* vals, const T* b,
               int64_t ldb, const T* beta, T* c, int64_t ldc, int64_t nrhs)
{
    GKOC_REQUIRE(n_rows >= 0 && n_cols >= 0 && nrhs >= 0, GKOC_E_INVALID,
                 "negative dimension");
    if (n_rows == 0 || nrhs == 0) return GKOC_OK;
    GKOC_REQUIRE(row_ptrs && c, GKOC_E_INVALID, "null pointer");
    GKOC_REQUIRE(ldc >= nrhs && (n_cols == 0 || ldb >= nrhs), GKOC_E_INVALID,
                 "stride smaller than nrhs");
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
int launch_csr_mixed(gkoc_stream_t s, int64_t n_rows, int64_t n_cols, const T* alpha,
                     const I* row_ptrs, const I* col_idxs, const V* vals, const T* b, int64_t ldb,
                     const T* beta, T* c, int64_t ldc, int64_t nrhs)
{
    GKOC_REQUIRE(n_rows >= 0 && n_cols >= 0 && nrhs >= 0, GKOC_E_INVALID, "negative dimension");
    if (n_rows == 0 || nrhs == 0) return GKOC_OK;
    GKOC_REQUIRE(row_ptrs && c, GKOC_E_INVALID, "null pointer");
    GKOC_REQUIRE(ldc >= nrhs && (n_cols == 0 || ldb >= nrhs), GKOC_E_INVALID,
                 "stride smaller than nrhs");
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
int launch_csr_dot(gkoc_stream_t s, int64_t n, const I* row_ptrs,
                   const I* col_idxs, const T* vals, const T* b, T* c,
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
    if (tune_value(GKOC_TUNE_CSR_LONG_ROWS) != 0) {
        csr_long_info lng;
        GKOC_TRY((long_info_of<T, I>(s, n, row_ptrs, &lng)));
        if (lng.count > 0) {
            GKOC_TRY((launch_csr<T, I, false>(s, n, n, nullptr, row_ptrs, col_idxs, vals, b, 1, nullptr, c, 1, 1)));
            if constexpr (sizeof(T) == 8) {
                return gkoc_dense_compute_dot_f64(s, n, 1, reinterpret_cast<const double*>(b), 1,
                                                  reinterpret_cast<const double*>(c), 1,
                                                  reinterpret_cast<double*>(dot_out), work, work_bytes);
            } else {
                return gkoc_dense_compute_dot_f32(s, n, 1, reinterpret_cast<const float*>(b), 1,
                                                  reinterpret_cast<const float*>(c), 1,
                                                  reinterpret_cast<float*>(dot_out), work, work_bytes);
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
    if constexpr (std::is_same<I, int32_t>::value) {
        if (vals != nullptr && reinterpret_cast<uintptr_t>(vals) % 16 == 0 && tune_value(GKOC_TUNE_CSR_OFFSETS) != 2) {
            evicted_plans evicted;
            std::lock_guard<std::mutex> plan_lock(g_off_mtx);
            offsets_plan* plan = offsets_plan_for(as_stream(s), n, n, row_ptrs, col_idxs, csr_long_info{}, &evicted.v);
            if (plan != nullptr && plan->skip == nullptr) {
                launch_offsets_kernel<T, false, true>(as_stream(s), *plan, p, n, n, static_cast<const T*>(nullptr),
                                                      row_ptrs, vals, b, static_cast<const T*>(nullptr), c, partial);
                GKOC_LAUNCH_OK();
                ++plan->products;
                return fold_partials<T>(s, p.n_waves, partial, scratch, dot_out, false);
            }
        }
    }
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

// ---- diagonal extraction / sortedness / per-row sort ---------------------

// One wave per 64 rows: the rows' contiguous column-index (and value) range is
// staged in LDS with coalesced loads, lane = row then works on its row there.
// Segments longer than the stage fall back to walking global memory per lane.
constexpr int row_stage_cap = 2048;

template <typename I>
struct row_segment {
    int64_t row, rs, re, K0, K1;
    bool valid;
};

template <typename I>
__device__ __forceinline__ row_segment<I> load_row_segment(int64_t n_rows,
                                                           const I* row_ptrs)
{
    row_segment<I> g;
    const int64_t first = int64_t(blockIdx.x) * 64;
    g.row = first + threadIdx.x;
    g.valid = g.row < n_rows;
    const int64_t last = first + 64 < n_rows ? first + 64 : n_rows;
    g.rs = row_ptrs[g.valid ? g.row : last];
    g.re = row_ptrs[g.valid ? g.row + 1 : last];
    g.K0 = row_ptrs[first];
    g.K1 = row_ptrs[last];
    return g;
}

template <typename T, typename I>
__global__ __launch_bounds__(64) void extract_diag_kernel(
    int64_t n_diag, const I* __restrict__ row_ptrs, const I* __restrict__ cols,
    const T* __restrict__ vals, T* __restrict__ diag)
{
    __shared__ I lc[row_stage_cap];
    const row_segment<I> g = load_row_segment<I>(n_diag, row_ptrs);
    const bool staged = g.K1 - g.K0 <= row_stage_cap;
    if (staged) {
        for (int i = threadIdx.x; i < int(g.K1 - g.K0); i += 64) lc[i] = cols[g.K0 + i];
        wave_lds_sync();
    }
    if (!g.valid) return;
    T d = T(0);
    for (int64_t k = g.rs; k < g.re; ++k) {
        const I c = staged ? lc[k - g.K0] : cols[k];
        if (int64_t(c) == g.row) {
            d = vals[k];
            break;
        }
    }
    diag[g.row] = d;
}

template <typename I>
__global__ __launch_bounds__(64) void is_sorted_kernel(
    int64_t n_rows, const I* __restrict__ row_ptrs, const I* __restrict__ cols,
    int* __restrict__ flag)
{
    __shared__ I lc[row_stage_cap];
    const row_segment<I> g = load_row_segment<I>(n_rows, row_ptrs);
    const bool staged = g.K1 - g.K0 <= row_stage_cap;
    if (staged) {
        for (int i = threadIdx.x; i < int(g.K1 - g.K0); i += 64) lc[i] = cols[g.K0 + i];
        wave_lds_sync();
    }
    bool ok = true;
    if (g.valid) {
        for (int64_t k = g.rs + 1; k < g.re; ++k) {
            const I a = staged ? lc[k - 1 - g.K0] : cols[k - 1];
            const I b = staged ? lc[k - g.K0] : cols[k];
            if (a > b) {
                ok = false;
                break;
            }
        }
    }
    if (__any(!ok) && threadIdx.x == 0) atomicAnd(flag, 0);
}

// stable insertion sort per row (rows are short on this path; Ginkgo only
// calls it when is_sorted_by_column_index returned false)
template <typename T, typename I>
__global__ __launch_bounds__(64) void sort_rows_kernel(
    int64_t n_rows, const I* __restrict__ row_ptrs, I* __restrict__ cols,
    T* __restrict__ vals)
{
    __shared__ I lc[row_stage_cap];
    __shared__ T lv[row_stage_cap];
    const row_segment<I> g = load_row_segment<I>(n_rows, row_ptrs);
    const bool staged = g.K1 - g.K0 <= row_stage_cap;
    if (staged) {
        const int seg = int(g.K1 - g.K0);
        for (int i = threadIdx.x; i < seg; i += 64) {
            lc[i] = cols[g.K0 + i];
            lv[i] = vals[g.K0 + i];
        }
        wave_lds_sync();
        if (g.valid) {
            const int a = int(g.rs - g.K0), e = int(g.re - g.K0);
            for (int i = a + 1; i < e; ++i) {
                const I ci = lc[i];
                const T vi = lv[i];
                int k = i - 1;
                while (k >= a && lc[k] > ci) {
                    lc[k + 1] = lc[k];
                    lv[k + 1] = lv[k];
                    --k;
                }
                lc[k + 1] = ci;
                lv[k + 1] = vi;
            }
        }
        wave_lds_sync();
        for (int i = threadIdx.x; i < seg; i += 64) {
            cols[g.K0 + i] = lc[i];
            vals[g.K0 + i] = lv[i];
        }
        return;
    }
    if (!g.valid) return;
    for (int64_t i = g.rs + 1; i < g.re; ++i) {
        const I ci = cols[i];
        const T vi = vals[i];
        int64_t k = i - 1;
        while (k >= g.rs && cols[k] > ci) {
            cols[k + 1] = cols[k];
            vals[k + 1] = vals[k];
            --k;
        }
        cols[k + 1] = ci;
        vals[k + 1] = vi;
    }
}

}  // namespace

// (common.hpp) the index array(s) in [first, first + bytes) are freed or written: what was derived from them goes
void csr_offsets_forget(const void* first, size_t bytes)
{
    const char* lo = static_cast<const char*>(first);
    const char* hi = lo + (bytes ? bytes : 1);
    std::vector<offsets_plan> gone;
    {
        std::lock_guard<std::mutex> g(g_off_mtx);
        for (auto it = g_off_cache.begin(); it != g_off_cache.end();) {
            const char* rp = static_cast<const char*>(std::get<1>(it->first));
            const char* ci = static_cast<const char*>(std::get<2>(it->first));
            // [lo, hi) overlaps either allocation (a copy into the middle of an array counts)
            if ((lo < rp + it->second.rp_bytes && rp < hi) || (lo < ci + it->second.ci_bytes && ci < hi)) {
                gone.push_back(it->second);
                it = g_off_cache.erase(it);
            } else {
                ++it;
            }
        }
        g_csr_offsets_cached.store(int(g_off_cache.size()));
    }
    offsets_release(gone);
}

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

#define GKOC_DEF_CSR(T, TN, I, IN)                                             \
    extern "C" int gkoc_csr_spmv_##TN##_##IN(                                  \
        gkoc_stream_t s, int64_t n_rows, int64_t n_cols, const I* row_ptrs,    \
        const I* col_idxs, const T* vals, const T* b, int64_t ldb, T* c,       \
        int64_t ldc, int64_t nrhs)                                             \
    {                                                                          \
        return launch_csr<T, I, false>(s, n_rows, n_cols, nullptr, row_ptrs,   \
                                       col_idxs, vals, b, ldb, nullptr, c,     \
                                       ldc, nrhs);                             \
    }                                                                          \
    extern "C" int gkoc_csr_advanced_spmv_##TN##_##IN(                         \
        gkoc_stream_t s, int64_t n_rows, int64_t n_cols, const T* alpha,       \
        const I* row_ptrs, const I* col_idxs, const T* vals, const T* b,       \
        int64_t ldb, const T* beta, T* c, int64_t ldc, int64_t nrhs)           \
    {                                                                          \
        return launch_csr<T, I, true>(s, n_rows, n_cols, alpha, row_ptrs,      \
                                      col_idxs, vals, b, ldb, beta, c, ldc,    \
                                      nrhs);                                   \
    }                                                                          \
    extern "C" int gkoc_x_csr_spmv_dot_##TN##_##IN(                            \
        gkoc_stream_t s, int64_t n, const I* row_ptrs, const I* col_idxs,      \
        const T* vals, const T* b, T* c, T* dot_out, void* work,               \
        size_t work_bytes)                                                     \
    {                                                                          \
        return launch_csr_dot<T, I>(s, n, row_ptrs, col_idxs, vals, b, c,      \
                                    dot_out, work, work_bytes);                \
    }                                                                          \
    extern "C" int gkoc_csr_extract_diagonal_##TN##_##IN(                      \
        gkoc_stream_t s, int64_t n_rows, int64_t n_cols, const I* row_ptrs,    \
        const I* col_idxs, const T* vals, T* diag)                             \
    {                                                                          \
        const int64_t nd = n_rows < n_cols ? n_rows : n_cols;                  \
        if (nd <= 0) return GKOC_OK;                                           \
        extract_diag_kernel<T, I>                                              \
            <<<dim3(unsigned(ceildiv(nd, 64))), dim3(64), 0, as_stream(s)>>>(  \
                nd, row_ptrs, col_idxs, vals, diag);                           \
        GKOC_LAUNCH_OK();                                                      \
        return GKOC_OK;                                                        \
    }                                                                          \
    extern "C" int gkoc_csr_is_sorted_by_column_index_##TN##_##IN(             \
        gkoc_stream_t s, int64_t n_rows, const I* row_ptrs,                    \
        const I* col_idxs, int* is_sorted_host)                                \
    {                                                                          \
        GKOC_REQUIRE(is_sorted_host, GKOC_E_INVALID, "null result");           \
        *is_sorted_host = 1;                                                   \
        if (n_rows <= 0) return GKOC_OK;                                       \
        int* flag = nullptr;                                                   \
        GKOC_TRY(scratch_malloc(as_stream(s), reinterpret_cast<void**>(&flag), \
                                sizeof(int)));                                 \
        /* any non-zero pattern = sorted; set on the device (an asynchronous */ \
        /* copy from pageable host memory is not ordered with the kernel)    */ \
        GKOC_HIP(hipMemsetAsync(flag, 1, sizeof(int), as_stream(s)));          \
        is_sorted_kernel<I>                                                    \
            <<<dim3(unsigned(ceildiv(n_rows, 64))), dim3(64), 0,               \
               as_stream(s)>>>(n_rows, row_ptrs, col_idxs, flag);              \
        GKOC_LAUNCH_OK();                                                      \
        GKOC_HIP(hipMemcpyAsync(is_sorted_host, flag, sizeof(int),             \
                                hipMemcpyDeviceToHost, as_stream(s)));         \
        GKOC_HIP(hipStreamSynchronize(as_stream(s)));                          \
        GKOC_TRY(scratch_free(as_stream(s), flag));                            \
        *is_sorted_host = *is_sorted_host != 0;                                \
        return GKOC_OK;                                                        \
    }                                                                          \
    extern "C" int gkoc_csr_sort_by_column_index_##TN##_##IN(                  \
        gkoc_stream_t s, int64_t n_rows, const I* row_ptrs, I* col_idxs,       \
        T* vals)                                                               \
    {                                                                          \
        if (n_rows <= 0) return GKOC_OK;                                       \
        gkoc::csr_structure_written(col_idxs);                                 \
        sort_rows_kernel<T, I>                                                 \
            <<<dim3(unsigned(ceildiv(n_rows, 64))), dim3(64), 0,               \
               as_stream(s)>>>(n_rows, row_ptrs, col_idxs, vals);              \
        GKOC_LAUNCH_OK();                                                      \
        return GKOC_OK;                                                        \
    }

GKOC_DEF_CSR(double, f64, int32_t, i32)
GKOC_DEF_CSR(double, f64, int64_t, i64)
GKOC_DEF_CSR(float, f32, int32_t, i32)
GKOC_DEF_CSR(float, f32, int64_t, i64)

// csr::sort_by_column_index for complex values (pairs; the kernel only moves them)
#define GKOC_DEF_CSR_SORT(T, TN, I, IN)                                        \
    extern "C" int gkoc_csr_sort_by_column_index_##TN##_##IN(                  \
        gkoc_stream_t s, int64_t n_rows, const I* row_ptrs, I* col_idxs,       \
        T* vals)                                                               \
    {                                                                          \
        if (n_rows <= 0) return GKOC_OK;                                       \
        gkoc::csr_structure_written(col_idxs);                                 \
        sort_rows_kernel<T, I>                                                 \
            <<<dim3(unsigned(ceildiv(n_rows, 64))), dim3(64), 0,               \
               as_stream(s)>>>(n_rows, row_ptrs, col_idxs, vals);              \
        GKOC_LAUNCH_OK();                                                      \
        return GKOC_OK;                                                        \
    }
GKOC_DEF_CSR_SORT(gkoc_c128, c128, int32_t, i32)
GKOC_DEF_CSR_SORT(gkoc_c128, c128, int64_t, i64)
GKOC_DEF_CSR_SORT(gkoc_c64, c64, int32_t, i32)
GKOC_DEF_CSR_SORT(gkoc_c64, c64, int64_t, i64)

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

extern "C" int gkoc_csr_structure_changed(const void* index_array)
{
    gkoc::csr_structure_written(index_array);
    return GKOC_OK;
}

extern "C" int gkoc_csr_plan_info(const void* row_ptrs, const void* col_idxs, int* state, int64_t* eligible_segments,
                                  int64_t* segments, int64_t* bytes, int64_t* products_by_plan)
{
    int st = -1;
    int64_t el = 0, ns = 0, by = 0, pr = 0;
    int dev = 0;
    GKOC_HIP(hipGetDevice(&dev));
    {
        std::lock_guard<std::mutex> g(gkoc::g_off_mtx);
        for (const auto& kv : gkoc::g_off_cache) {
            if (std::get<0>(kv.first) == dev && std::get<1>(kv.first) == row_ptrs &&
                std::get<2>(kv.first) == col_idxs) {
                st = kv.second.state;
                el = kv.second.eligible;
                ns = kv.second.n_seg;
                by = kv.second.bytes;
                pr = kv.second.products;
            }
        }
    }
    if (state) *state = st;
    if (eligible_segments) *eligible_segments = el;
    if (segments) *segments = ns;
    if (bytes) *bytes = by;
    if (products_by_plan) *products_by_plan = pr;
    return GKOC_OK;
}

extern "C" int gkoc_csr_plan_classes(const void* row_ptrs, const void* col_idxs, uint64_t* classes)
{
    uint64_t nc = 0;
    int dev = 0;
    GKOC_HIP(hipGetDevice(&dev));
    {
        std::lock_guard<std::mutex> g(gkoc::g_off_mtx);
        for (const auto& kv : gkoc::g_off_cache) {
            if (std::get<0>(kv.first) == dev && std::get<1>(kv.first) == row_ptrs &&
                std::get<2>(kv.first) == col_idxs) {
                nc = uint64_t(kv.second.n_classes);
            }
        }
    }
    if (classes) *classes = nc;
    return GKOC_OK;
}

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

#define GKOC_DEF_CSR_MIXED(I, IN)                                                                  \
    extern "C" int gkoc_csr_spmv_f32_f64_##IN(gkoc_stream_t s, int64_t n_rows, int64_t n_cols,     \
                                              const I* row_ptrs, const I* col_idxs,                \
                                              const float* vals, const double* b, int64_t ldb,     \
                                              double* c, int64_t ldc, int64_t nrhs)                \
    {                                                                                              \
        return launch_csr_mixed<double, float, I, false>(s, n_rows, n_cols, nullptr, row_ptrs,     \
                                                         col_idxs, vals, b, ldb, nullptr, c, ldc,  \
                                                         nrhs);                                    \
    }                                                                                              \
    extern "C" int gkoc_csr_advanced_spmv_f32_f64_##IN(                                            \
        gkoc_stream_t s, int64_t n_rows, int64_t n_cols, const double* alpha, const I* row_ptrs,   \
        const I* col_idxs, const float* vals, const double* b, int64_t ldb, const double* beta,    \
        double* c, int64_t ldc, int64_t nrhs)                                                      \
    {                                                                                              \
        return launch_csr_mixed<double, float, I, true>(s, n_rows, n_cols, alpha, row_ptrs,        \
                                                        col_idxs, vals, b, ldb, beta, c, ldc,      \
                                                        nrhs);                                     \
    }
GKOC_DEF_CSR_MIXED(int32_t, i32)
GKOC_DEF_CSR_MIXED(int64_t, i64)

extern "C" size_t gkoc_x_workspace_bytes(int64_t n, size_t value_size)
{
    return gkoc::fused_workspace_bytes(n < 0 ? 0 : n, value_size);
}
