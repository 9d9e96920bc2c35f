"""Plain restatements of the distributed set-up kernels (ginkgo_amd/csrc/dist_setup.hip), as
reference/distributed/*_kernels.cpp and partition_helpers.hpp are described in include/gko_cdna4.h and in the
comments of dist_setup.hip.  Every operation comes twice: as a loop over the input, the way the reference walks
it, and - with the suffix _v - in a vectorised numpy formulation that shares no code with the loop
(np.searchsorted, np.unique, np.lexsort, stable argsort, np.bincount, np.cumsum).  The two are compared with
each other in tests/test_dist_setup_refs_cpu.py; the GPU tests use the loops on the small cases and the
vectorised forms on the million-entry ones.

All indices are handled as int64 and narrowed at the end (`astype`, which wraps like the kernels' casts);
values are only ever moved, so they stay numpy arrays of whatever dtype the caller chose."""
import bisect

import numpy as np

INVALID = -1


class Part:
    """a partition on the host: bounds[num_ranges + 1], pids[num_ranges], starts[num_ranges], sizes[num_parts]"""

    def __init__(self, bounds, pids, num_parts):
        self.bounds = np.asarray(bounds, np.int64)
        self.pids = np.asarray(pids, np.int32)
        self.num_parts = int(num_parts)
        assert len(self.bounds) == len(self.pids) + 1 and np.all(np.diff(self.bounds) >= 0)
        assert len(self.pids) == 0 or (self.pids.min() >= 0 and self.pids.max() < num_parts)
        self.starts, self.sizes, self.num_empty = build_starting_indices_v(self.bounds, self.pids, num_parts)

    @property
    def num_ranges(self):
        return len(self.pids)


# ------------------------------------------------------------------------------------------ find_range
def find_range(idx, bounds):
    """number of upper bounds bounds[1..num_ranges] that are <= idx (partition_helpers.hpp), as a binary search"""
    lo, hi = 0, len(bounds) - 1
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if bounds[1 + mid] <= idx:
            lo = mid + 1
        else:
            hi = mid
    return lo


def find_range_v(idx, bounds):
    return np.searchsorted(np.asarray(bounds)[1:], np.asarray(idx), side="right").astype(np.int64)


# ------------------------------------------------------------------------------------------ partition
def count_ranges(mapping):
    count, prev = 0, -1
    for m in mapping:
        if m != prev:
            count += 1
        prev = m
    return count


def count_ranges_v(mapping):
    mapping = np.asarray(mapping)
    return 0 if len(mapping) == 0 else 1 + int(np.count_nonzero(np.diff(mapping)))


def build_from_contiguous(ranges, mapping=None):
    """ranges[num_ranges + 1] -> bounds (bounds[0] = 0 whatever ranges[0] is), part ids"""
    num_ranges = max(len(ranges) - 1, 0)
    bounds, pids = np.zeros(num_ranges + 1, np.int64), np.zeros(num_ranges, np.int32)
    for i in range(num_ranges):
        bounds[i + 1] = ranges[i + 1]
        pids[i] = i if mapping is None else mapping[i]
    return bounds, pids


def build_from_contiguous_v(ranges, mapping=None):
    ranges = np.asarray(ranges, np.int64)
    num_ranges = max(len(ranges) - 1, 0)
    bounds = np.concatenate([[0], ranges[1:]]).astype(np.int64)
    pids = np.arange(num_ranges, dtype=np.int32) if mapping is None else np.asarray(mapping, np.int32).copy()
    return bounds, pids


def build_from_mapping(mapping):
    bounds, pids, prev = [0], [], -1
    for i, m in enumerate(mapping):
        if m != prev:
            if i > 0:
                bounds.append(i)
            pids.append(m)
        prev = m
    if len(mapping) > 0:
        bounds.append(len(mapping))
    return np.array(bounds, np.int64), np.array(pids, np.int32)


def build_from_mapping_v(mapping):
    mapping = np.asarray(mapping, np.int32)
    if len(mapping) == 0:
        return np.zeros(1, np.int64), np.zeros(0, np.int32)
    heads = np.flatnonzero(np.concatenate([[True], mapping[1:] != mapping[:-1]]))
    return np.concatenate([heads, [len(mapping)]]).astype(np.int64), mapping[heads].copy()


def build_ranges_from_global_size(num_parts, global_size):
    per, rest = global_size // num_parts, global_size % num_parts
    out = np.zeros(num_parts + 1, np.int64)
    for i in range(num_parts):
        out[i + 1] = out[i] + per + (1 if i < rest else 0)
    return out


def build_ranges_from_global_size_v(num_parts, global_size):
    i = np.arange(num_parts + 1, dtype=np.int64)
    return i * (global_size // num_parts) + np.minimum(i, global_size % num_parts)


def build_starting_indices(offsets, parts, num_parts):
    """ranks[r] = what part parts[r] owns in the ranges before r; sizes per part; number of parts of size 0"""
    sizes = np.zeros(num_parts, np.int64)
    ranks = np.zeros(len(parts), np.int64)
    for r, p in enumerate(parts):
        ranks[r] = sizes[p]
        sizes[p] += offsets[r + 1] - offsets[r]
    return ranks, sizes, int(sum(1 for s in sizes if s == 0))


def build_starting_indices_v(offsets, parts, num_parts):
    offsets, parts = np.asarray(offsets, np.int64), np.asarray(parts, np.int64)
    length = np.diff(offsets) if len(parts) else np.zeros(0, np.int64)
    order = np.argsort(parts, kind="stable")
    sl = length[order]
    excl = np.cumsum(sl) - sl
    sizes = np.zeros(num_parts, np.int64)
    np.add.at(sizes, parts, length)
    part_first = np.concatenate([[0], np.cumsum(sizes)])[:-1] if num_parts else np.zeros(0, np.int64)
    ranks = np.zeros(len(parts), np.int64)
    ranks[order] = excl - part_first[parts[order]]
    return ranks, sizes, int(np.count_nonzero(sizes == 0))


def build_ranges_by_part(parts, num_parts):
    ids, sizes = [], np.zeros(num_parts, np.int64)
    for p in range(num_parts):
        for r, q in enumerate(parts):
            if q == p:
                ids.append(r)
                sizes[p] += 1
    return np.array(ids, np.int64), sizes


def build_ranges_by_part_v(parts, num_parts):
    parts = np.asarray(parts, np.int64)
    return np.lexsort((np.arange(len(parts)), parts)).astype(np.int64), \
        np.bincount(parts, minlength=num_parts).astype(np.int64)


def has_ordered_parts(pids):
    return all(pids[i] >= pids[i - 1] for i in range(1, len(pids)))


def has_ordered_parts_v(pids):
    return bool(np.all(np.diff(np.asarray(pids, np.int64)) >= 0))


# ------------------------------------------------------------------------------------------ partition_helpers
def sort_by_range_start(se, pids):
    """(start, end) pairs and their part ids, stably sorted by start (insertion sort)"""
    se = [int(v) for v in se]
    items, keys = [], []
    for i in range(len(pids)):
        k = bisect.bisect_right(keys, se[2 * i])      # behind every earlier pair with the same start
        keys.insert(k, se[2 * i])
        items.insert(k, (se[2 * i], se[2 * i + 1], pids[i]))
    out = np.array([v for it in items for v in it[:2]], np.int64).reshape(-1)
    return out, np.array([it[2] for it in items], np.int32)


def sort_by_range_start_v(se, pids):
    se = np.asarray(se, np.int64).reshape(-1, 2)
    order = np.argsort(se[:, 0], kind="stable")
    return se[order].reshape(-1), np.asarray(pids, np.int32)[order]


def check_consecutive_ranges(se):
    return all(se[2 * i + 2] == se[2 * i + 1] for i in range(len(se) // 2 - 1))


def check_consecutive_ranges_v(se):
    se = np.asarray(se, np.int64)
    return bool(np.all(se[2::2] == se[1:-1:2]))


def compress_ranges(se):
    """num_parts pairs -> num_parts + 1 offsets (num_parts >= 1)"""
    out = [se[0]]
    for i in range(len(se) // 2):
        out.append(se[2 * i + 1])
    return np.array(out, np.int64)


def compress_ranges_v(se):
    se = np.asarray(se, np.int64)
    return np.concatenate([se[:1], se[1::2]])


# ------------------------------------------------------------------------------------------ matrix / vector
def _local(g, part, r):
    return part.starts[r] + (g - part.bounds[r])


def separate_local_nonlocal(rows, cols, vals, rp, cp, local_part):
    """-> (local rows, local cols, local vals, non-local rows, non-local GLOBAL cols, non-local vals)"""
    lr, lc, lk, nr, nc, nk = [], [], [], [], [], []
    for i in range(len(rows)):
        rr = find_range(rows[i], rp.bounds)
        if rp.pids[rr] != local_part:
            continue
        cr = find_range(cols[i], cp.bounds)
        if cp.pids[cr] == local_part:
            lr.append(_local(rows[i], rp, rr)), lc.append(_local(cols[i], cp, cr)), lk.append(i)
        else:
            nr.append(_local(rows[i], rp, rr)), nc.append(cols[i]), nk.append(i)
    a = lambda v: np.array(v, np.int64)
    return a(lr), a(lc), vals[a(lk)], a(nr), a(nc), vals[a(nk)]


def separate_local_nonlocal_v(rows, cols, vals, rp, cp, local_part):
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    rr, cr = find_range_v(rows, rp.bounds), find_range_v(cols, cp.bounds)
    if len(rows) == 0:
        e = np.zeros(0, np.int64)
        return e, e, vals[:0], e, e, vals[:0]
    ours = rp.pids[rr] == local_part
    loc = ours & (cp.pids[cr] == local_part)
    non = ours & ~loc
    lrow = rp.starts[rr] + rows - rp.bounds[rr]
    lcol = cp.starts[cr] + cols - cp.bounds[cr]
    return lrow[loc], lcol[loc], vals[loc], lrow[non], cols[non], vals[non]


def vector_build_local(rows, cols, vals, part, local_part, out):
    """out[local row, col] = value for the rows local_part owns (distinct (row, col) pairs); in place"""
    for i in range(len(rows)):
        rr = find_range(rows[i], part.bounds)
        if part.pids[rr] == local_part:
            out[_local(rows[i], part, rr), cols[i]] = vals[i]
    return out


def vector_build_local_v(rows, cols, vals, part, local_part, out):
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    if len(rows):
        rr = find_range_v(rows, part.bounds)
        ours = part.pids[rr] == local_part
        out[(part.starts[rr] + rows - part.bounds[rr])[ours], cols[ours]] = vals[ours]
    return out


# ------------------------------------------------------------------------------------------ index_map
def build_mapping(recv, part):
    """-> (part ids that occur, remote local idxs, remote global idxs, ids per occurring part): the unique
    received ids ordered by (owning part, id)"""
    seen = set()
    for g in recv:
        seen.add((int(part.pids[find_range(g, part.bounds)]), int(g)))
    pids, loc, glob, sizes = [], [], [], []
    for p, g in sorted(seen):
        if not pids or pids[-1] != p:
            pids.append(p), sizes.append(0)
        sizes[-1] += 1
        glob.append(g)
        loc.append(_local(g, part, find_range(g, part.bounds)))
    return np.array(pids, np.int32), np.array(loc, np.int64), np.array(glob, np.int64), np.array(sizes, np.int64)


def build_mapping_v(recv, part):
    g = np.unique(np.asarray(recv, np.int64))
    if len(g) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    rr = find_range_v(g, part.bounds)
    order = np.lexsort((g, part.pids[rr]))
    g, rr = g[order], rr[order]
    pids, sizes = np.unique(part.pids[rr], return_counts=True)
    return pids.astype(np.int32), part.starts[rr] + g - part.bounds[rr], g, sizes.astype(np.int64)


def map_to_local(gids, part, target_ids, remote_flat, remote_offsets, rank, index_space):
    """index_space 0 local, 1 non-local, 2 combined; -1 for an id that is not in the space or not in the
    partition's [bounds[0], bounds[num_ranges])"""
    out = np.full(len(gids), INVALID, np.int64)
    for i, g in enumerate(gids):
        if part.num_ranges == 0 or g < part.bounds[0] or g >= part.bounds[-1]:
            continue
        rr = find_range(g, part.bounds)
        pid = part.pids[rr]
        if index_space == 0 or (index_space == 2 and pid == rank):
            if pid == rank:
                out[i] = _local(g, part, rr)
            continue
        for k, t in enumerate(target_ids):
            if t == pid:
                for j in range(remote_offsets[k], remote_offsets[k + 1]):
                    if remote_flat[j] == g:
                        out[i] = j + (part.sizes[rank] if index_space == 2 else 0)
    return out


def map_to_local_v(gids, part, target_ids, remote_flat, remote_offsets, rank, index_space):
    gids = np.asarray(gids, np.int64)
    out = np.full(len(gids), INVALID, np.int64)
    if part.num_ranges == 0 or len(gids) == 0:
        return out
    inside = (gids >= part.bounds[0]) & (gids < part.bounds[-1])
    g = np.where(inside, gids, part.bounds[0])
    rr = find_range_v(g, part.bounds)
    pid = part.pids[rr].astype(np.int64)
    local = inside & (pid == rank)
    if index_space in (0, 2):
        out[local] = (part.starts[rr] + g - part.bounds[rr])[local]
    if index_space in (1, 2) and len(remote_flat):
        # one key per (part, id): the flat remote ids are ascending in it
        span = int(part.bounds[-1] - part.bounds[0]) + 1
        remote_flat = np.asarray(remote_flat, np.int64)
        rpart = np.repeat(np.asarray(target_ids, np.int64), np.diff(remote_offsets))
        rkey = rpart * span + (remote_flat - part.bounds[0])
        key = pid * span + (g - part.bounds[0])
        k = np.searchsorted(rkey, key)
        hit = inside & (k < len(rkey)) & (rkey[np.minimum(k, len(rkey) - 1)] == key)
        if index_space == 2:
            hit &= ~local
        out[hit] = k[hit] + (part.sizes[rank] if index_space == 2 else 0)
    return out


def map_to_global(lids, bounds, starts, local_size, local_ranges, remote_flat, index_space):
    """local_ranges: the range ids of the rank in range order; -1 for a local id outside the space"""
    out = np.full(len(lids), INVALID, np.int64)
    for i, lid in enumerate(lids):
        lid = int(lid)
        local = index_space == 0
        if index_space == 2:
            if lid < local_size:
                local = True
            else:
                lid -= local_size
        if local:
            if 0 <= lid < local_size:
                rid = None
                for r in local_ranges:      # the last local range whose starting index is <= lid
                    if starts[r] <= lid:
                        rid = r
                out[i] = lid - starts[rid] + bounds[rid]
        elif 0 <= lid < len(remote_flat):
            out[i] = remote_flat[lid]
    return out


def map_to_global_v(lids, bounds, starts, local_size, local_ranges, remote_flat, index_space):
    lids = np.asarray(lids, np.int64)
    out = np.full(len(lids), INVALID, np.int64)
    bounds, starts = np.asarray(bounds, np.int64), np.asarray(starts, np.int64)
    local_ranges, remote_flat = np.asarray(local_ranges, np.int64), np.asarray(remote_flat, np.int64)
    if index_space in (0, 2) and len(local_ranges):
        ok = (lids >= 0) & (lids < local_size)
        k = np.searchsorted(starts[local_ranges], lids[ok], side="right") - 1
        rid = local_ranges[k]
        out[ok] = lids[ok] - starts[rid] + bounds[rid]
    if index_space in (1, 2):
        shift = local_size if index_space == 2 else 0
        ok = (lids >= shift) & (lids - shift < len(remote_flat))
        out[ok] = remote_flat[lids[ok] - shift]
    return out


# ------------------------------------------------------------------------------------------ assembly
def count_non_owning_entries(rows, part, local_part, send_count):
    """send_count (per part) is ADDED TO, in place; -> (send_positions, original_positions)"""
    n = len(rows)
    orig, key = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for i in range(n):
        pid = part.pids[find_range(rows[i], part.bounds)]
        if pid != local_part:
            send_count[pid] += 1
            orig[i], key[i] = i, pid
        else:
            orig[i], key[i] = -1, local_part
    items, keys = [], []             # stable insertion sort by key
    for i in range(n):
        k = bisect.bisect_right(keys, key[i])
        keys.insert(k, key[i])
        items.insert(k, orig[i])
    orig_sorted = np.array(items, np.int64)
    pos, run = np.zeros(n, np.int64), 0
    for i in range(n):
        pos[i] = run
        run += 0 if orig_sorted[i] == -1 else 1
    return pos, orig_sorted


def count_non_owning_entries_v(rows, part, local_part, send_count):
    rows = np.asarray(rows, np.int64)
    n = len(rows)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    pid = part.pids[find_range_v(rows, part.bounds)].astype(np.int64)
    send = pid != local_part
    send_count += np.bincount(pid[send], minlength=len(send_count)).astype(send_count.dtype)
    orig = np.where(send, np.arange(n), -1)
    orig_sorted = orig[np.argsort(pid, kind="stable")]     # (an owned entry's key is local_part = its pid)
    flag = (orig_sorted != -1).astype(np.int64)
    return np.cumsum(flag) - flag, orig_sorted


def fill_send_buffers(rows, cols, vals, send_positions, original_positions):
    total = int(sum(1 for o in original_positions if o >= 0))
    srow, scol, sidx = np.zeros(total, np.int64), np.zeros(total, np.int64), np.zeros(total, np.int64)
    for i, o in enumerate(original_positions):
        if o >= 0:
            srow[send_positions[i]], scol[send_positions[i]], sidx[send_positions[i]] = rows[o], cols[o], o
    return srow, scol, vals[sidx]


def fill_send_buffers_v(rows, cols, vals, send_positions, original_positions):
    orig = np.asarray(original_positions, np.int64)
    take = orig[orig >= 0]
    at = np.asarray(send_positions, np.int64)[orig >= 0]
    assert np.array_equal(at, np.arange(len(take)))
    return np.asarray(rows, np.int64)[take], np.asarray(cols, np.int64)[take], vals[take]


# ------------------------------------------------------------------------------------------ case families
def random_values(rng, n, dtype):
    """random BIT patterns (NaN payloads, infinities, denormals) plus -0.0 and two NaNs with payloads in front:
    a value that went through arithmetic instead of being copied shows"""
    dtype = np.dtype(dtype)
    v = rng.integers(0, 256, n * dtype.itemsize, dtype=np.uint8).view(dtype).copy()
    word = {4: np.uint32, 8: np.uint64, 16: np.uint64}[dtype.itemsize]
    w = v.view(word)
    special = {np.uint32: [0x80000000, 0x7FA00001, 0xFFC12345],
               np.uint64: [0x8000000000000000, 0x7FF4000000000001, 0xFFF8000000012345]}[word]
    for k, s in enumerate(special[:len(w)]):
        w[k] = s
    return v


def mapping_runs(rng, n, parts, max_run):
    """a mapping of n ids to the part ids `parts` in runs of 1..max_run, neighbouring runs differing"""
    out, prev = np.zeros(n, np.int32), -1
    i = 0
    while i < n:
        p = int(parts[rng.integers(len(parts))])
        if p == prev and len(parts) > 1:
            continue
        k = int(rng.integers(1, max_run + 1))
        out[i:i + k] = p
        i, prev = i + k, p
    return out


D_NUM_PARTS = 9
D_MAPPING_PARTS = [0, 1, 3, 4, 5, 6, 8]        # parts 2 and 7 get no id


def mapping_d(seed=5, n=600):
    return mapping_runs(np.random.default_rng(seed), n, D_MAPPING_PARTS, 5)


def partition(name, offset=0):
    """the partitions (a) .. (f) of the tests, see docs/binding_kernel_tests.md"""
    if name == "a":                             # one range, one part
        return Part([0, 1000], [0], 1)
    if name == "b":                             # contiguous, 7 uneven parts
        return Part(np.cumsum([0, 13, 1, 200, 57, 300, 2, 427]), np.arange(7), 7)
    if name == "c":                             # the same ranges, part ids permuted
        return Part(np.cumsum([0, 13, 1, 200, 57, 300, 2, 427]), [3, 0, 6, 1, 5, 2, 4], 7)
    if name in ("d", "e"):
        # from a mapping with many short ranges: parts own several non-adjacent ranges; part 2 owns nothing,
        # part 7 only a zero-length range, and zero-length ranges of parts 0, 4 and 8 sit at the front, in the
        # middle and at the end.  (e) is the same far above 2^33.
        bounds, pids = build_from_mapping_v(mapping_d())
        bounds, pids = list(bounds), list(pids)
        for at, p in ((len(pids), 8), (len(pids) // 2, 7), (len(pids) // 3, 4), (len(pids) // 3, 0), (0, 0)):
            bounds.insert(at, bounds[at])
            pids.insert(at, p)
        off = (2 ** 33 + 5) if name == "e" else 0
        return Part(np.array(bounds, np.int64) + off + offset, pids, D_NUM_PARTS)
    if name == "f":                             # about 100 000 ranges over 64 parts
        bounds, pids = build_from_mapping_v(mapping_runs(np.random.default_rng(6), 200000, np.arange(64), 3))
        return Part(bounds, pids, 64)
    raise KeyError(name)


def random_ids(rng, part, n):
    """n ids of [bounds[0], bounds[num_ranges]), the first ones on both sides of range bounds"""
    lo, hi = int(part.bounds[0]), int(part.bounds[-1])
    ids = rng.integers(lo, hi, n, dtype=np.int64)
    edges = np.unique(np.concatenate([part.bounds[:-1], part.bounds[1:] - 1]))
    edges = edges[(edges >= lo) & (edges < hi)]
    k = min(n, len(edges), 4096)
    ids[:k] = rng.permutation(edges)[:k]
    return rng.permutation(ids)


def owned_ids(part, p):
    """every id that part p owns, ascending"""
    r = np.flatnonzero(part.pids == p)
    if len(r) == 0:
        return np.zeros(0, np.int64)
    return np.concatenate([np.arange(part.bounds[k], part.bounds[k + 1]) for k in r]).astype(np.int64)


def local_ranges_of(part, p):
    ids, sizes = build_ranges_by_part_v(part.pids, part.num_parts)
    first = int(np.sum(sizes[:p]))
    return ids[first:first + int(sizes[p])].astype(np.uint64)


def interesting_parts(part):
    """local parts to test with: the part with the most ranges, the owners of the first and the last range,
    and a part that owns nothing where there is one"""
    counts = np.bincount(part.pids, minlength=part.num_parts)
    picks = sorted({int(np.argmax(counts)), int(part.pids[0]), int(part.pids[-1])})
    empty = np.flatnonzero(part.sizes == 0)
    return picks + ([int(empty[0])] if len(empty) else [])
