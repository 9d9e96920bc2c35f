// What the library remembers about the structure of a CSR matrix (csr_structure.hip), for the SpMV launchers
// (csr_spmv.hip).  Two caches, both instances of structure_cache.hpp (128 entries, the oldest arrival makes room)
// behind ONE mutex:
//   * long rows, key (device, row_ptrs, n_rows), any pointer: which 64-row segments hold a row beyond
//     GKOC_CSR_LONG_ROW (csr_long_rows.hpp), found by one scan in the first product of the key;
//   * column-offset plans, key (device, row_ptrs, col_idxs, n_rows), live allocations of the arena only: the
//     analysis of csr_offsets.hpp, made by the second product of the key.
// A product takes a LEASE - the mutex - in front of its lookups and keeps it until the last kernel that reads a
// cached buffer is enqueued, so nothing it was handed can be released under it.  Entries that leave a cache
// (eviction, gkoc_free, a written index array) give their device buffers to ONE release path, which runs after
// the mutex is free: a device synchronisation (a product in flight on any stream may still read them), then
// arena_free; while a stream capture forbids the synchronisation they wait in a graveyard for the next release.
#pragma once
#include <mutex>
#include <vector>

#include "common.hpp"

namespace gkoc {

// the long rows of a matrix: the cache entry's flags, and the CALLING stream's buffer of chunk sums
struct csr_long_info {
    int64_t count = 0;                   // flagged segments (0: none - the common case)
    uint32_t* bits = nullptr;            // device: one bit per segment
    unsigned long long* list = nullptr;  // device: [count, segment indices ...]
    int64_t nnz = -1;                    // row_ptrs[n_rows] when the matrix was looked at (-1: unknown)
    void* partial = nullptr;             // device: chunk sums, THE CALLING STREAM's buffer (filled in per call)
};

struct offsets_plan {
    int state = 0;                  // 0: seen once, 1: in use, 2: rejected (fewer than half of the segments eligible)
    int64_t n_seg = 0, eligible = 0;
    int max_d = 0;                  // the largest D of a segment: picks the product kernel's diagonal slots
    int64_t n_classes = 0;          // distinct (table, masks) among the segments (csr_offsets.hpp)
    int64_t nnz = 0;                // stored entries when the plan was built: sizes the product (offsets_nt_min_bytes)
    int32_t* seg_class = nullptr;   // device: the class id of every segment
    int32_t* cls_tab = nullptr;     // device: OFFS_TAB int32 per class
    uint32_t* cls_mask = nullptr;   // device: 64 words per class, one per row of a segment
    uint32_t* skip = nullptr;       // device: bit per segment the row-segment kernel leaves out (eligible | flagged)
    bool with_long = false;         // skip holds the long-row flags too
    int64_t bytes = 0, products = 0;
    size_t rp_bytes = 0, ci_bytes = 0;      // the two allocations the plan describes (csr_offsets_forget)
};

bool stream_is_capturing(hipStream_t st);

// Holds the caches' mutex from its construction to give_back() or its end, whichever comes first, and collects
// the buffers of the entries that made room meanwhile; they are released once the mutex is free.
struct csr_structure_lease {
    csr_structure_lease();
    ~csr_structure_lease() { give_back(); }      // (not copyable: the lock is not)
    void give_back();
    std::vector<void*> dropped;      // (filled by the lookups below)
    std::unique_lock<std::mutex> lock;
};

// The long rows of (row_ptrs, n_rows), I = int32_t / int64_t.  The first product of a key scans the row pointers
// and synchronises `st` once; inside a stream capture the answer is "none" and the next product looks.
template <typename I>
int csr_long_info_for(csr_structure_lease& lease, hipStream_t st, int64_t n_rows, const I* row_ptrs,
                      csr_long_info* out);

// The plan a one-column product of these arrays on `st` may use, or nullptr; valid while the lease is held.
offsets_plan* csr_offsets_plan_for(csr_structure_lease& lease, hipStream_t st, int64_t n_rows, int64_t n_cols,
                                   const int32_t* row_ptrs, const int32_t* col_idxs, const csr_long_info& lng);

}  // namespace gkoc
