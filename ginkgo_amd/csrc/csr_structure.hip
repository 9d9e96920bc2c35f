// What the library remembers about the structure of a CSR matrix: the long-row flags and the column-offset plans
// of the SpMV launchers (csr_spmv.hip).  The rules - two keys, one mutex, the lease, the release path - are in
// csr_structure.hpp; the mechanism of both caches is structure_cache.hpp.
#include <cstring>      // (rocprim's texture_cache_iterator.hpp calls memset without including it)
#include <tuple>

#include <rocprim/rocprim.hpp>

#include "csr_long_rows.hpp"
#include "csr_offsets_analysis.hpp"
#include "csr_structure.hpp"
#include "structure_cache.hpp"

namespace gkoc {

std::atomic<int> g_csr_offsets_cached{0};      // (common.hpp csr_structure_written: the plan cache's count)

namespace {

std::mutex g_mtx;      // both caches and the graveyard

// ---- which 64-row segments of a matrix hold a row beyond GKOC_CSR_LONG_ROW (csr_long_rows.hpp) --------
// Found by one scan of the row pointers the first time a (device, row_ptrs, n_rows) is multiplied, kept
// here (flags and list read-only from then on; the chunk sums of a product go to a buffer per (matrix, stream),
// so products of one matrix on several streams share nothing that is written); gkoc_free forgets the entries of
// a pointer that goes away (csr_long_rows_forget).  The first product of a matrix therefore synchronises its
// stream once (the scan's answer is needed on the host) - documented in gko_cdna4.h; inside a stream capture the
// matrix is multiplied by the row-segment kernel alone.
struct long_entry {
    csr_long_info info;
    // one buffer of chunk sums per stream that has multiplied this matrix (count x 8 x 64 values of 8 bytes)
    std::vector<std::pair<hipStream_t, void*>> partials;
};
using long_key = std::tuple<int, const void*, int64_t>;
constexpr size_t long_cache_cap = 128;
constexpr int64_t long_list_cap = 4096;      // more flagged segments than this: the matrix has no "few long rows"
structure_cache<long_key, long_entry> g_long_cache(long_cache_cap);

// ---- cached per-segment column offsets (csr_offsets.hpp) ---------------------------------------------------
// A derived, read-only description of (row_ptrs, col_idxs), keyed by (device, row_ptrs, col_idxs, n_rows).  Only
// for index arrays that are live allocations of the library's own allocator: their addresses cannot be reused
// without gkoc_free seeing them.  Built by the SECOND product on the same arrays (a one-shot product never pays;
// GKOC_TUNE_CSR_OFFSETS = 1: by the first, 2: never), never inside a stream capture (the product takes the
// row-segment kernel and the next one tries again).  Dropped by csr_offsets_forget: gkoc_free, every C-ABI entry
// that writes an index array of a CSR matrix, gkoc_memcpy_h2d / _d2d into one, gkoc_csr_structure_changed.
using offsets_key = std::tuple<int, const void*, const void*, int64_t>;
constexpr size_t offsets_cache_cap = 128;
structure_cache<offsets_key, offsets_plan> g_off_cache(offsets_cache_cap);
// at least this share of the segments must be eligible, in per cent (docs/KERNELS.md: measured on a stencil
// whose every other segment is not)
constexpr int64_t offsets_min_share = 50;

// ---- the release path ---------------------------------------------------------------------------------------
// the device buffers of entries that left a cache (an entry that never had hub rows / a plan that was never
// built has none)
void buffers_of(const long_entry& en, std::vector<void*>* bufs)
{
    if (en.info.bits) bufs->push_back(en.info.bits);
    if (en.info.list) bufs->push_back(en.info.list);
    for (const auto& sp : en.partials) bufs->push_back(sp.second);
}
void buffers_of(const offsets_plan& pl, std::vector<void*>* bufs)
{
    for (void* b : {static_cast<void*>(pl.seg_class), static_cast<void*>(pl.cls_tab),
                    static_cast<void*>(pl.cls_mask), static_cast<void*>(pl.skip)}) {
        if (b) bufs->push_back(b);
    }
}

// buffers that could not be released at once (inside a stream capture the device cannot be synchronised):
// released with the next ones that go.  Guarded by g_mtx.
std::vector<void*> g_graveyard;

// Called WITHOUT the mutex.  Only entries that HAVE buffers pay the synchronisation (a product in flight on any
// stream may still read them).
void release_buffers(std::vector<void*>& bufs)
{
    if (bufs.empty()) return;
    std::lock_guard<std::mutex> g(g_mtx);
    g_graveyard.insert(g_graveyard.end(), bufs.begin(), bufs.end());
    bufs.clear();
    if (hipDeviceSynchronize() != hipSuccess) {
        (void)hipGetLastError();      // (a capture is under way: they wait in the graveyard)
        return;
    }
    for (void* b : g_graveyard) (void)arena_free(b);
    g_graveyard.clear();
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
        arena_malloc(&p, size_t(en.info.count) * LONG_MAX_PER_SEG * LONG_PARTS * 8, GKOC_MEM_AUTO) != GKOC_OK) {
        (void)hipGetLastError();
        *out = csr_long_info{};
        out->nnz = en.info.nnz;
        return;
    }
    en.partials.emplace_back(st, p);
    out->partial = p;
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
    auto u64 = [&](size_t off) { return static_cast<unsigned long long*>(at(off)); };
    auto u32 = [&](size_t off) { return static_cast<uint32_t*>(at(off)); };
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
        csr_offsets_hash_kernel<<<seg_grid, seg_block, 0, st>>>(n_rows, n_seg, tab_c, mask_c, keep, u64(cs.hash),
                                                                u32(cs.ids));
        size_t prim_bytes = cs.prim_bytes;
        ok = hipGetLastError() == hipSuccess &&
             rocprim::radix_sort_pairs(at(cs.prim), prim_bytes, u64(cs.hash), u64(cs.hash_sorted), u32(cs.ids),
                                       u32(cs.ids_sorted), size_t(n_seg), 0, 64, st) == hipSuccess;
        if (ok) {
            csr_offsets_leader_kernel<<<seg_grid, seg_block, 0, st>>>(
                n_rows, n_seg, tab_c, mask_c, u64(cs.hash_sorted), u32(cs.ids_sorted), u32(cs.leader), u32(cs.is_new));
            prim_bytes = cs.prim_bytes;
            ok = hipGetLastError() == hipSuccess &&
                 rocprim::exclusive_scan(at(cs.prim), prim_bytes, u32(cs.is_new), u32(cs.class_at), uint32_t(0),
                                         size_t(n_seg), rocprim::plus<uint32_t>(), st) == hipSuccess;
        }
        if (ok) {
            csr_offsets_class_count_kernel<<<dim3(1), dim3(1), 0, st>>>(
                n_seg, u32(cs.is_new), u32(cs.class_at), n_rows, row_ptrs, static_cast<unsigned long long*>(count_dev));
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
            n_rows, n_seg, static_cast<const int32_t*>(tab), static_cast<const uint32_t*>(mask), u32(cs.ids_sorted),
            u32(cs.leader), u32(cs.is_new), u32(cs.class_at), static_cast<int32_t*>(ids), static_cast<int32_t*>(ctab),
            static_cast<uint32_t*>(cmask));
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

// the cached plan of the two arrays on the current device, whatever its n_rows (gkoc_csr_plan_info / _classes)
int plan_at(const void* row_ptrs, const void* col_idxs, offsets_plan* out)
{
    int dev = 0;
    GKOC_HIP(hipGetDevice(&dev));
    *out = offsets_plan{};
    out->state = -1;
    csr_structure_lease lease;
    g_off_cache.for_each([&](const offsets_key& k, const offsets_plan& pl) {
        if (std::get<0>(k) == dev && std::get<1>(k) == row_ptrs && std::get<2>(k) == col_idxs) *out = pl;
    });
    return GKOC_OK;
}

}  // namespace

bool stream_is_capturing(hipStream_t st)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone) return false;
    (void)hipGetLastError();
    return true;
}

csr_structure_lease::csr_structure_lease() : lock(g_mtx) {}

void csr_structure_lease::give_back()
{
    if (lock.owns_lock()) lock.unlock();
    release_buffers(dropped);
}

template <typename I>
int csr_long_info_for(csr_structure_lease& lease, hipStream_t st, int64_t n_rows, const I* row_ptrs,
                      csr_long_info* out)
{
    int dev = 0;
    GKOC_HIP(hipGetDevice(&dev));
    const long_key key{dev, row_ptrs, n_rows};
    if (long_entry* en = g_long_cache.find(key)) {
        long_partial_for(*en, st, out);
        return GKOC_OK;
    }
    // a stream that is being captured into a hipGraph cannot be synchronised: a matrix first seen there is
    // multiplied by the row-segment kernel alone (correct for any row), and looked at on its next product
    if (stream_is_capturing(st)) {
        *out = csr_long_info{};
        return GKOC_OK;
    }
    // the first look at a matrix: its flags, or count = 0 - none (the common case), or so many that "a few long
    // rows" is not what this matrix has: the row-segment kernel does everything
    long_entry fresh;
    const int64_t n_seg = ceildiv(n_rows, int64_t(64));
    const size_t bit_bytes = size_t(ceildiv(n_seg, int64_t(32))) * 4;
    const size_t list_bytes = size_t(1 + long_list_cap) * 8;
    void *bits = nullptr, *list = nullptr;
    GKOC_TRY(arena_malloc(&bits, bit_bytes, GKOC_MEM_AUTO));
    if (arena_malloc(&list, list_bytes, GKOC_MEM_AUTO) != GKOC_OK) {
        (void)arena_free(bits);
        return GKOC_E_INVALID;
    }
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
    if (ok) fresh.info.nnz = int64_t(nnz_dev);
    if (!ok || count == 0 || int64_t(count) > long_list_cap) {
        (void)hipGetLastError();
        (void)arena_free(bits);
        (void)arena_free(list);
    } else {
        fresh.info.count = int64_t(count);
        fresh.info.bits = static_cast<uint32_t*>(bits);
        fresh.info.list = static_cast<unsigned long long*>(list);
    }
    std::vector<long_entry> gone;
    long_entry* en = g_long_cache.insert(key, fresh, &gone);
    for (const auto& old : gone) buffers_of(old, &lease.dropped);
    long_partial_for(*en, st, out);
    return GKOC_OK;
}
template int csr_long_info_for<int32_t>(csr_structure_lease&, hipStream_t, int64_t, const int32_t*, csr_long_info*);
template int csr_long_info_for<int64_t>(csr_structure_lease&, hipStream_t, int64_t, const int64_t*, csr_long_info*);

offsets_plan* csr_offsets_plan_for(csr_structure_lease& lease, hipStream_t st, int64_t n_rows, int64_t n_cols,
                                   const int32_t* row_ptrs, const int32_t* col_idxs, const csr_long_info& lng)
{
    const int64_t mode = tune_value(GKOC_TUNE_CSR_OFFSETS);
    if (mode == 2 || row_ptrs == nullptr || col_idxs == nullptr || n_cols < 1 ||
        n_rows >= (int64_t(1) << 31) - 64 || n_cols >= (int64_t(1) << 31)) {
        return nullptr;
    }
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    const offsets_key key{dev, row_ptrs, col_idxs, n_rows};
    offsets_plan* pl = g_off_cache.find(key);
    if (pl == nullptr) {
        offsets_plan fresh;
        fresh.rp_bytes = arena_allocation_bytes(row_ptrs);
        fresh.ci_bytes = arena_allocation_bytes(col_idxs);
        if (fresh.rp_bytes == 0 || fresh.ci_bytes == 0) return nullptr;
        std::vector<offsets_plan> gone;
        pl = g_off_cache.insert(key, fresh, &gone);
        for (const auto& en : gone) buffers_of(en, &lease.dropped);
        g_csr_offsets_cached.store(g_off_cache.count());
        if (mode != 1) return nullptr;      // the first product of these arrays
    }
    if (pl->state == 0) {
        if (stream_is_capturing(st)) return nullptr;
        (void)offsets_build(st, n_rows, row_ptrs, col_idxs, lng, *pl);
    }
    if (pl->state != 1) return nullptr;
    // the row-segment kernel beside this one must leave out what the plan's skip bits say, and somebody must
    // do the long-flagged segments: only with the flags the plan was built with
    if (pl->skip != nullptr && pl->with_long != (lng.count > 0)) return nullptr;
    return pl;
}

// (common.hpp) gkoc_free: what is remembered about the row pointers at this address goes
void csr_long_rows_forget(const void* ptr)
{
    if (ptr == nullptr || g_long_cache.count() == 0) return;
    csr_structure_lease lease;
    std::vector<long_entry> gone;
    g_long_cache.erase_if([ptr](const long_key& k, const long_entry&) { return std::get<1>(k) == ptr; }, &gone);
    for (const auto& en : gone) buffers_of(en, &lease.dropped);
}

// (common.hpp) the index array(s) in [first, first + bytes) are freed or written: what was derived from them goes
void csr_offsets_forget(const void* first, size_t bytes)
{
    const char* lo = static_cast<const char*>(first);
    const char* hi = lo + (bytes ? bytes : 1);
    csr_structure_lease lease;
    std::vector<offsets_plan> gone;
    g_off_cache.erase_if(
        [lo, hi](const offsets_key& k, const offsets_plan& pl) {
            const char* rp = static_cast<const char*>(std::get<1>(k));
            const char* ci = static_cast<const char*>(std::get<2>(k));
            // [lo, hi) overlaps either allocation (a copy into the middle of an array counts)
            return (lo < rp + pl.rp_bytes && rp < hi) || (lo < ci + pl.ci_bytes && ci < hi);
        },
        &gone);
    g_csr_offsets_cached.store(g_off_cache.count());
    for (const auto& en : gone) buffers_of(en, &lease.dropped);
}

}  // namespace gkoc

extern "C" int gkoc_csr_structure_changed(const void* index_array)
{
    gkoc::csr_structure_written(index_array);
    return GKOC_OK;
}

extern "C" int gkoc_csr_plan_info(const void* row_ptrs, const void* col_idxs, int* state, int64_t* eligible_segments,
                                  int64_t* segments, int64_t* bytes, int64_t* products_by_plan)
{
    gkoc::offsets_plan pl;
    GKOC_TRY(gkoc::plan_at(row_ptrs, col_idxs, &pl));
    if (state) *state = pl.state;
    if (eligible_segments) *eligible_segments = pl.eligible;
    if (segments) *segments = pl.n_seg;
    if (bytes) *bytes = pl.bytes;
    if (products_by_plan) *products_by_plan = pl.products;
    return GKOC_OK;
}

extern "C" int gkoc_csr_plan_classes(const void* row_ptrs, const void* col_idxs, uint64_t* classes)
{
    gkoc::offsets_plan pl;
    GKOC_TRY(gkoc::plan_at(row_ptrs, col_idxs, &pl));
    if (classes) *classes = uint64_t(pl.n_classes);
    return GKOC_OK;
}
