"""tests/dist_setup_refs.py against itself, no GPU: the loop form of every operation equals its vectorised
form on the case families the GPU tests use (partitions (a) .. (f), small and medium sizes), and properties
that follow from what the operations mean hold for both."""
import numpy as np
import pytest

import dist_setup_refs as dr

PARTS = ["a", "b", "c", "d", "e", "f"]
SIZES = [0, 1, 2, 257, 2049]


def _rng(*key):
    return np.random.default_rng(sum(map(ord, "".join(map(str, key)))))


def _eq(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8) if x.dtype.kind in "fc" else x,
                                                     y.view(np.uint8) if y.dtype.kind in "fc" else y)


_local_parts = dr.interesting_parts


@pytest.mark.parametrize("name", PARTS)
def test_find_range_against_a_linear_scan(name):
    part = dr.partition(name)
    ids = dr.random_ids(_rng(name), part, 3000)
    fast = dr.find_range_v(ids, part.bounds)
    for g, f in zip(ids[:400 if name == "f" else 3000], fast):
        linear = sum(1 for b in part.bounds[1:] if b <= g) if name != "f" else \
            int(np.count_nonzero(part.bounds[1:] <= g))
        assert dr.find_range(g, part.bounds) == linear == f
        assert part.bounds[f] <= g < part.bounds[f + 1]


def test_partition_fixtures_are_what_they_claim():
    d = dr.partition("d")
    assert d.num_empty == 2 and d.sizes[2] == 0 and d.sizes[7] == 0 and 7 in d.pids and 2 not in d.pids
    assert np.count_nonzero(np.diff(d.bounds) == 0) == 5
    assert np.bincount(d.pids).max() > 5                        # several non-adjacent ranges per part
    e = dr.partition("e")
    assert e.bounds[0] > 2 ** 33 and np.array_equal(e.starts, d.starts) and np.array_equal(e.sizes, d.sizes)
    assert 90000 < dr.partition("f").num_ranges < 110000
    assert not dr.has_ordered_parts(dr.partition("c").pids) and dr.has_ordered_parts(dr.partition("b").pids)


@pytest.mark.parametrize("n", SIZES + [100000])
def test_partition_builders(n):
    rng = _rng("builders", n)
    mapping = dr.mapping_runs(rng, n, dr.D_MAPPING_PARTS, 5)
    assert dr.count_ranges(mapping) == dr.count_ranges_v(mapping)
    b, p = dr.build_from_mapping(mapping)
    _eq((b, p), dr.build_from_mapping_v(mapping))
    assert len(p) == dr.count_ranges(mapping) and b[0] == 0 and b[-1] == n
    assert np.array_equal(np.repeat(p, np.diff(b)), mapping)    # the partition reproduces the mapping
    num_ranges = min(n, 3000)
    ranges = np.concatenate([[7], np.cumsum(rng.integers(0, 5, num_ranges))]) if n else np.zeros(0, np.int64)
    perm = rng.permutation(num_ranges).astype(np.int32)
    for m in (None, perm):
        got = dr.build_from_contiguous(ranges, m)
        _eq(got, dr.build_from_contiguous_v(ranges, m))
        assert got[0][0] == 0 and len(got[0]) == num_ranges + 1
    if n:
        for size in (0, 1, n - 1, n, n + 1, 7 * n + 3):
            r = dr.build_ranges_from_global_size(n if n < 3000 else 3000, size)
            _eq((r,), (dr.build_ranges_from_global_size_v(n if n < 3000 else 3000, size),))
            assert r[0] == 0 and r[-1] == size and np.diff(r).max() - np.diff(r).min() <= 1
            assert np.all(np.diff(np.diff(r)) <= 0)             # the larger parts come first


@pytest.mark.parametrize("name", PARTS)
def test_starting_indices_and_ranges_by_part(name):
    part = dr.partition(name)
    ranks, sizes, empty = dr.build_starting_indices(part.bounds, part.pids, part.num_parts)
    _eq((ranks, sizes), dr.build_starting_indices_v(part.bounds, part.pids, part.num_parts)[:2])
    assert empty == part.num_empty == int(np.count_nonzero(sizes == 0))
    assert sizes.sum() == part.bounds[-1] - part.bounds[0]
    ids, counts = dr.build_ranges_by_part_v(part.pids, part.num_parts)
    if name != "f":
        _eq((ids, counts), dr.build_ranges_by_part(part.pids, part.num_parts))
    assert np.array_equal(np.sort(ids), np.arange(part.num_ranges)) and counts.sum() == part.num_ranges
    length, first = np.diff(part.bounds), 0
    for p in range(part.num_parts):                             # ranks = exclusive scan of the part's lengths
        mine = ids[first:first + counts[p]]
        first += counts[p]
        assert np.all(part.pids[mine] == p) and np.all(np.diff(mine) > 0)
        assert np.array_equal(ranks[mine], np.cumsum(length[mine]) - length[mine])
        assert sizes[p] == length[mine].sum()
        assert np.array_equal(dr.local_ranges_of(part, p), mine.astype(np.uint64))
    assert dr.has_ordered_parts(part.pids) == dr.has_ordered_parts_v(part.pids)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 257, 2049])
def test_partition_helpers(n):
    rng = _rng("helpers", n)
    offsets = np.concatenate([[11], 11 + np.cumsum(rng.integers(0, 4, n))])       # equal starts occur
    se = np.stack([offsets[:-1], offsets[1:]], 1).reshape(-1)
    pids = rng.permutation(n).astype(np.int32)
    assert dr.check_consecutive_ranges(se) and dr.check_consecutive_ranges_v(se)
    if n:
        _eq((dr.compress_ranges(se),), (dr.compress_ranges_v(se),))
        assert np.array_equal(dr.compress_ranges(se), offsets)
    for order in (np.arange(n), np.arange(n)[::-1], rng.permutation(n)):
        s_in, p_in = se.reshape(-1, 2)[order].reshape(-1), pids[order]
        got = dr.sort_by_range_start(s_in, p_in)
        _eq(got, dr.sort_by_range_start_v(s_in, p_in))
        starts = got[0][0::2]
        assert np.all(np.diff(starts) >= 0)
        # stable: among equal starts the input positions ascend
        where = {int(p): k for k, p in enumerate(p_in)}
        pos = np.array([where[int(p)] for p in got[1]], np.int64)
        assert all(pos[k] < pos[k + 1] for k in range(n - 1) if starts[k] == starts[k + 1])
    for wrong in sorted({0, (n - 1) // 2, n - 2}) if n >= 2 else []:                # one wrong pair flips it
        bad = se.copy()
        bad[2 * wrong + 2] += 1
        assert not dr.check_consecutive_ranges(bad) and not dr.check_consecutive_ranges_v(bad)
    for wrong in sorted({1, n // 2, n - 1}) if n >= 2 else []:
        ordered = np.sort(pids)
        assert dr.has_ordered_parts(ordered) and dr.has_ordered_parts_v(ordered)
        ordered[wrong:] += 1
        ordered[wrong] -= 3                                      # now below its left neighbour only
        assert not dr.has_ordered_parts(ordered) and not dr.has_ordered_parts_v(ordered)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", PARTS)
def test_separate_local_nonlocal(name, n):
    rp = dr.partition(name)
    cp = dr.partition("c") if name == "b" else rp               # (b) rows with (c) columns: partitions differ
    rng = _rng("separate", name, n)
    rows, cols = dr.random_ids(rng, rp, n), dr.random_ids(rng, cp, n)
    if n > 4:
        rows[n // 2:n // 2 + 2], cols[n // 2:n // 2 + 2] = rows[0], cols[0]        # duplicates
    vals = dr.random_values(rng, n, np.float64)
    for lp in _local_parts(rp):
        out = dr.separate_local_nonlocal(rows, cols, vals, rp, cp, lp)
        _eq(out, dr.separate_local_nonlocal_v(rows, cols, vals, rp, cp, lp))
        lr, lc, lv, nr, nc, nv = out
        # together: a permutation of exactly the entries whose row lp owns, rows mapped to local indices
        mine = np.flatnonzero(np.isin(rows, dr.owned_ids(rp, lp)))
        assert len(lr) + len(nr) == len(mine)
        own_rows, own_cols = dr.owned_ids(rp, lp), dr.owned_ids(cp, lp)
        lmap_r = {int(g): k for k, g in enumerate(own_rows)}
        lmap_c = {int(g): k for k, g in enumerate(own_cols)}
        want = sorted((lmap_r[int(rows[i])], int(cols[i]), vals[i:i + 1].tobytes()) for i in mine)
        inv_c = {k: g for g, k in lmap_c.items()}
        got = [(int(r), inv_c[int(c)], v.tobytes()) for r, c, v in zip(lr, lc, lv)] + \
              [(int(r), int(c), v.tobytes()) for r, c, v in zip(nr, nc, nv)]
        assert sorted(got) == want
        assert all(int(c) not in lmap_c for c in nc)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", PARTS)
def test_vector_build_local(name, n):
    part = dr.partition(name)
    rng = _rng("vector", name, n)
    span = int(part.bounds[-1] - part.bounds[0])
    cells = rng.permutation(span * 3)[:min(n, span * 3)]        # distinct (row, col) pairs
    rows, cols = part.bounds[0] + cells // 3, cells % 3
    vals = dr.random_values(rng, len(rows), np.float32)
    for lp in _local_parts(part):
        size = int(part.sizes[lp])
        a = dr.vector_build_local(rows, cols, vals, part, lp, np.full((size, 5), np.float32(7)))
        b = dr.vector_build_local_v(rows, cols, vals, part, lp, np.full((size, 5), np.float32(7)))
        _eq((a,), (b,))
        own = {int(g): k for k, g in enumerate(dr.owned_ids(part, lp))}
        hits = [i for i in range(len(rows)) if int(rows[i]) in own]
        assert np.count_nonzero(a.view(np.uint32) != np.float32(7).view(np.uint32)) <= len(hits)
        for i in hits:
            assert a[own[int(rows[i])], cols[i]].tobytes() == vals[i].tobytes()


def _index_map(part, rank, rng, n):
    """what rank receives: n ids (with repeats) that other parts own"""
    ids = dr.random_ids(rng, part, 4 * n + 8)
    ids = ids[part.pids[dr.find_range_v(ids, part.bounds)] != rank][:n]
    if len(ids) > 3:
        ids[len(ids) // 2] = ids[0]
    return ids


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", PARTS)
def test_index_map(name, n):
    part = dr.partition(name)
    rng = _rng("index_map", name, n)
    for rank in _local_parts(part):
        recv = _index_map(part, rank, rng, n)
        out = dr.build_mapping(recv, part)
        _eq(out, dr.build_mapping_v(recv, part))
        pids, loc, glob, sizes = out
        assert set(glob.tolist()) == set(recv.tolist()) and sizes.sum() == len(glob) and np.all(sizes > 0)
        assert np.all(np.diff(pids) > 0) and rank not in pids
        owner = part.pids[dr.find_range_v(glob, part.bounds)] if len(glob) else np.zeros(0, np.int32)
        assert np.array_equal(owner, np.repeat(pids, sizes))
        assert all(np.all(np.diff(seg) > 0) for seg in np.split(glob, np.cumsum(sizes)[:-1]))
        for k, g in enumerate(glob):
            assert dr.owned_ids(part, int(owner[k]))[loc[k]] == g
        offsets = np.concatenate([[0], np.cumsum(sizes)])
        owned = dr.owned_ids(part, rank)
        lo, hi = int(part.bounds[0]), int(part.bounds[-1])
        queries = np.concatenate([dr.random_ids(rng, part, 300), owned[:50], glob[:50],
                                  [lo - 1, hi, lo - 2 ** 20, hi + 2 ** 20]])
        ranges, local_size = dr.local_ranges_of(part, rank), int(part.sizes[rank])
        for space in (0, 1, 2):
            lid = dr.map_to_local(queries, part, pids, glob, offsets, rank, space)
            _eq((lid,), (dr.map_to_local_v(queries, part, pids, glob, offsets, rank, space),))
            in_space = (np.isin(queries, owned) if space != 1 else np.zeros(len(queries), bool)) | \
                (np.isin(queries, glob) if space != 0 else np.zeros(len(queries), bool))
            assert np.array_equal(lid == -1, ~in_space)
            back = dr.map_to_global(lid, part.bounds, part.starts, local_size, ranges, glob, space)
            _eq((back,), (dr.map_to_global_v(lid, part.bounds, part.starts, local_size, ranges, glob, space),))
            assert np.array_equal(back[in_space], queries[in_space]) and np.all(back[~in_space] == -1)
            size = {0: local_size, 1: len(glob), 2: local_size + len(glob)}[space]
            every = np.arange(-2, size + 3)
            g = dr.map_to_global(every, part.bounds, part.starts, local_size, ranges, glob, space)
            _eq((g,), (dr.map_to_global_v(every, part.bounds, part.starts, local_size, ranges, glob, space),))
            assert np.array_equal(g == -1, (every < 0) | (every >= size))
            assert np.array_equal(dr.map_to_local_v(g[2:-3], part, pids, glob, offsets, rank, space), every[2:-3])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", PARTS)
def test_assembly(name, n):
    part = dr.partition(name)
    rng = _rng("assembly", name, n)
    rows, cols = dr.random_ids(rng, part, n), dr.random_ids(rng, part, n)
    vals = dr.random_values(rng, n, np.complex128)
    for lp in _local_parts(part):
        start = rng.integers(0, 9, part.num_parts).astype(np.int32)
        c1, c2 = start.copy(), start.copy()
        pos, orig = dr.count_non_owning_entries(rows, part, lp, c1)
        _eq((pos, orig, c1), dr.count_non_owning_entries_v(rows, part, lp, c2) + (c2,))
        owner = part.pids[dr.find_range_v(rows, part.bounds)] if n else np.zeros(0, np.int32)
        assert c1[lp] == start[lp]                              # owned entries contribute nothing
        bufs = dr.fill_send_buffers(rows, cols, vals, pos, orig)
        _eq(bufs, dr.fill_send_buffers_v(rows, cols, vals, pos, orig))
        # the non-owned entries grouped by owner, input order inside a group
        want = np.concatenate([np.flatnonzero(owner == p) for p in range(part.num_parts) if p != lp] +
                              [np.zeros(0, np.int64)]).astype(np.int64)
        _eq(bufs, (rows[want], cols[want], vals[want]))
        assert np.array_equal((c1 - start)[np.arange(part.num_parts) != lp],
                              np.bincount(owner[owner != lp], minlength=part.num_parts)[np.arange(part.num_parts) != lp])
