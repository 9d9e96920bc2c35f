"""The set-up kernels of distributed::Matrix / Vector::read_distributed, index_map and
assemble_rows_from_neighbors (csrc/dist_setup.hip: gkoc_dist_separate_local_nonlocal_*,
gkoc_dist_vector_build_local_*, gkoc_index_map_*, gkoc_assembly_*) through the C ABI against
tests/dist_setup_refs.py.

Indices are compared with np.array_equal, moved values bit for bit (random bit patterns: NaN payloads, -0.0).
Inputs are read back and compared after every call; every device output is pre-filled with a sentinel, is
longer than what the operation defines (the rest must keep the sentinel) and is followed by canaries; host
outputs are compared as well.  The partitions (a) .. (f) of dist_setup_refs.partition are shared by all entry
points.  All ids keep to the header's precondition (inside [bounds[0], bounds[num_ranges])) except the queries
of map_to_local, whose out-of-range answer is -1."""
import ctypes as C

import numpy as np
import pytest

import dist_setup_refs as dr
from binding_gpu import CANARY, SENTINEL, Dev, DevPartition, call as _call, grid_cap_rows, head_of, \
    out_buf as _out, same_bits, sync, tail_ok

pytestmark = pytest.mark.gpu

NP = {"i32": np.int32, "i64": np.int64}
LG = [("i32", "i32"), ("i32", "i64"), ("i64", "i64")]
VT = {4: np.float32, 8: np.float64, 16: np.complex128}
SIZES = [0, 1, 2, 255, 256, 257, 2047, 2048, 2049, 100003]
LARGE = 2048 * 2048 + 257
PAD = 4
CASES = [(ln, gn, name) for ln, gn in LG for name in ["a", "b", "c", "d", "f"] + (["e"] if gn == "i64" else [])]
_PARTS = {}


def _ints(gexec, n, t):
    return _out(gexec, n + PAD, t, fill=SENTINEL)


def _vals(gexec, n, t):
    return _out(gexec, n + PAD, t)              # NaN


def _head(out, n):
    return head_of(out, n + PAD, n, SENTINEL if out.dtype.kind == "i" else np.nan)


def _untouched(out, n):
    """an output of _ints / _vals(n) still holds its fill everywhere"""
    return len(head_of(out, n + PAD, 0, SENTINEL if out.dtype.kind == "i" else np.nan)) == 0


def _rng(*key):
    return np.random.default_rng(sum(map(ord, "".join(map(str, key)))))


def _vec(n):
    return n > 300                              # the loop references up to here, the vectorised ones above


def _part(gexec, ln, gn, name):
    """the host partition and its device copy (made once per type pair)"""
    if (ln, gn, name) not in _PARTS:
        part = dr.partition(name)
        _PARTS[(ln, gn, name)] = (part, DevPartition(gexec, NP[ln], NP[gn], part))
    return _PARTS[(ln, gn, name)]


def _local_parts(part, n):
    picks = dr.interesting_parts(part)
    return picks if n <= 300 else picks[:1]


def _unchanged(devs, hosts):
    return all(same_bits(d.get(), h) for d, h in zip(devs, hosts))


# ------------------------------------------------------------------------------ separate_local_nonlocal
def _separate(gexec, ln, gn, vs, rows, cols, vals, rp, cp, lp, vec):
    (rpart, drp), (cpart, dcp) = rp, cp
    lt, gt, nnz = NP[ln], NP[gn], len(rows)
    hosts = [rows.astype(gt), cols.astype(gt), vals]
    devs = [Dev(gexec, h) for h in hosts]
    state, n_l, n_n = C.c_void_p(5), C.c_int64(-5), C.c_int64(-5)
    _call(f"gkoc_dist_separate_local_nonlocal_count_{ln}_{gn}", gexec.stream, nnz, devs[0], devs[1], drp.ref,
          dcp.ref, C.c_int32(lp), C.byref(state), C.byref(n_l), C.byref(n_n))
    want = (dr.separate_local_nonlocal_v if vec else dr.separate_local_nonlocal)(rows, cols, vals, rpart, cpart, lp)
    if (n_l.value, n_n.value) != (len(want[0]), len(want[3])):
        _call("gkoc_dist_separate_state_free", gexec.stream, state)
        pytest.fail(f"counts {n_l.value}, {n_n.value}, reference {len(want[0])}, {len(want[3])}")
    assert nnz > 0 or state.value is None
    types = [lt, lt, vals.dtype, lt, gt, vals.dtype]
    sizes = [n_l.value] * 3 + [n_n.value] * 3
    outs = [(_vals if t == vals.dtype else _ints)(gexec, k, t) for k, t in zip(sizes, types)]
    _call(f"gkoc_dist_separate_local_nonlocal_fill_{ln}_{gn}", gexec.stream, nnz, *devs, C.c_size_t(vs), drp.ref,
          dcp.ref, state, *outs)
    sync()
    for k, (out, size, t, w) in enumerate(zip(outs, sizes, types, want)):
        got = _head(out, size)
        assert same_bits(got, w) if t == vals.dtype else np.array_equal(got, w.astype(t)), (k, nnz, lp)
    assert _unchanged(devs, hosts) and drp.unchanged() and dcp.unchanged()
    return want


def _entries(rng, rp, cp, n, vs):
    rows, cols = dr.random_ids(rng, rp, n), dr.random_ids(rng, cp, n)
    if n > 4:                                   # duplicate entries stay duplicates, in input order
        rows[n // 2:n // 2 + 2], cols[n // 2:n // 2 + 2] = rows[0], cols[0]
    return rows, cols, dr.random_values(rng, n, VT[vs])


@pytest.mark.parametrize("vs", list(VT))
@pytest.mark.parametrize("ln,gn,name", CASES)
def test_separate_local_nonlocal(gexec, ln, gn, name, vs):
    rp = _part(gexec, ln, gn, name)
    cp = _part(gexec, ln, gn, "c") if name == "b" else rp      # (b): the column partition differs
    for n in SIZES:
        rows, cols, vals = _entries(_rng("separate", name, n), rp[0], cp[0], n, vs)
        for lp in _local_parts(rp[0], n):
            _separate(gexec, ln, gn, vs, rows, cols, vals, rp, cp, lp, _vec(n))


def test_separate_local_nonlocal_beyond_the_grid_cap(gexec):
    assert LARGE + 1 > 2 * grid_cap_rows()
    rp = _part(gexec, "i32", "i64", "f")
    rows, cols, vals = _entries(_rng("separate large"), rp[0], rp[0], LARGE, 8)
    rows[-300:] = dr.owned_ids(rp[0], 5)[:300]                # owned rows at the very end, beyond the cap
    want = _separate(gexec, "i32", "i64", 8, rows, cols, vals, rp, rp, 5, True)
    assert len(want[0]) > 500 and len(want[3]) > 50000


# ------------------------------------------------------------------------------ vector_build_local
N_COLS, LD = 3, 5


def _vector_entries(rng, part, n, vs):
    span = int(part.bounds[-1] - part.bounds[0])
    cells = rng.permutation(span * N_COLS)[:min(n, span * N_COLS)]      # distinct (row, col) pairs
    return part.bounds[0] + cells // N_COLS, cells % N_COLS, dr.random_values(rng, len(cells), VT[vs])


def _vector_build_local(gexec, ln, gn, vs, rows, cols, vals, part, dpart, lp, vec):
    gt, size = NP[gn], int(part.sizes[lp])
    hosts = [rows.astype(gt), cols.astype(gt), vals]
    devs = [Dev(gexec, h) for h in hosts]
    out = _vals(gexec, size * LD, vals.dtype)
    _call(f"gkoc_dist_vector_build_local_{ln}_{gn}", gexec.stream, len(rows), *devs, C.c_size_t(vs), dpart.ref,
          C.c_int32(lp), out, LD)
    sync()
    want = np.full((size, LD), np.nan, vals.dtype)            # rows not owned, and the padding, keep the fill
    (dr.vector_build_local_v if vec else dr.vector_build_local)(rows, cols, vals, part, lp, want)
    assert same_bits(_head(out, size * LD), want.reshape(-1))
    assert _unchanged(devs, hosts) and dpart.unchanged()


@pytest.mark.parametrize("vs", list(VT))
@pytest.mark.parametrize("ln,gn,name", CASES)
def test_vector_build_local(gexec, ln, gn, name, vs):
    part, dpart = _part(gexec, ln, gn, name)
    for n in SIZES:
        rows, cols, vals = _vector_entries(_rng("vector", name, n), part, n, vs)
        for lp in _local_parts(part, n):
            _vector_build_local(gexec, ln, gn, vs, rows, cols, vals, part, dpart, lp, _vec(n))


# ------------------------------------------------------------------------------ index_map
def _received(rng, part, rank, n, targets=None):
    """n ids (with repeats) that rank receives: owned by other parts, or by `targets` only"""
    ids = dr.random_ids(rng, part, 4 * n + 8)
    owner = part.pids[dr.find_range_v(ids, part.bounds)]
    ids = ids[(owner != rank) if targets is None else np.isin(owner, targets)][:n]
    if len(ids) > 3:
        ids[len(ids) // 2] = ids[0]
    return ids


def _build_mapping(gexec, ln, gn, recv, part, dpart, vec):
    lt, gt, n = NP[ln], NP[gn], len(recv)
    d_recv = Dev(gexec, recv.astype(gt))
    state, n_u, n_p = C.c_void_p(5), C.c_int64(-5), C.c_int64(-5)
    _call(f"gkoc_index_map_build_mapping_count_{ln}_{gn}", gexec.stream, n, d_recv, dpart.ref, C.byref(state),
          C.byref(n_u), C.byref(n_p))
    want = (dr.build_mapping_v if vec else dr.build_mapping)(recv, part)
    if (n_u.value, n_p.value) != (len(want[2]), len(want[0])):
        _call("gkoc_index_map_mapping_state_free", gexec.stream, state)
        pytest.fail(f"counts {n_u.value}, {n_p.value}, reference {len(want[2])}, {len(want[0])}")
    assert n > 0 or state.value is None
    types, sizes = [np.int32, lt, gt, np.int64], [n_p.value, n_u.value, n_u.value, n_p.value]
    outs = [_ints(gexec, k, t) for k, t in zip(sizes, types)]
    _call(f"gkoc_index_map_build_mapping_fill_{ln}_{gn}", gexec.stream, dpart.ref, state, *outs)
    sync()
    for k, (out, size, t, w) in enumerate(zip(outs, sizes, types, want)):
        assert np.array_equal(_head(out, size), w.astype(t)), (k, n)
    assert same_bits(d_recv.get(), recv.astype(gt)) and dpart.unchanged()
    return want


def _map_to_local(gexec, ln, gn, queries, part, dpart, mapping, rank, space, vec):
    lt, gt = NP[ln], NP[gn]
    pids, _, glob, sizes = mapping
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    hosts = [queries.astype(gt), pids.astype(np.int32), glob.astype(gt), offsets]
    devs = [Dev(gexec, h) for h in hosts]
    out = _ints(gexec, len(queries), lt)
    _call(f"gkoc_index_map_map_to_local_{ln}_{gn}", gexec.stream, len(queries), devs[0], dpart.ref, len(pids),
          devs[1], devs[2], devs[3], C.c_int32(rank), C.c_int(space), out)
    sync()
    want = (dr.map_to_local_v if vec else dr.map_to_local)(queries, part, pids, glob, offsets, rank, space)
    got = _head(out, len(queries))
    assert np.array_equal(got, want.astype(lt)), (space, rank)
    assert _unchanged(devs, hosts) and dpart.unchanged()
    return want


def _map_to_global(gexec, ln, gn, lids, part, mapping, rank, space, vec):
    lt, gt = NP[ln], NP[gn]
    glob, ranges, local_size = mapping[2], dr.local_ranges_of(part, rank), int(part.sizes[rank])
    hosts = [lids.astype(lt), part.bounds.astype(gt), part.starts.astype(lt), ranges, glob.astype(gt)]
    devs = [Dev(gexec, h) for h in hosts]
    out = _ints(gexec, len(lids), gt)
    _call(f"gkoc_index_map_map_to_global_{ln}_{gn}", gexec.stream, len(lids), devs[0], devs[1], devs[2], local_size,
          devs[3], len(ranges), devs[4], len(glob), C.c_int(space), out)
    sync()
    want = (dr.map_to_global_v if vec else dr.map_to_global)(lids, part.bounds, part.starts, local_size, ranges,
                                                            glob, space)
    assert np.array_equal(_head(out, len(lids)), want.astype(gt)), (space, rank)
    assert _unchanged(devs, hosts)
    return want


def _outside(part):
    lo, hi = int(part.bounds[0]), int(part.bounds[-1])
    return np.array([lo - 1, hi, lo - 2 ** 20, hi + 2 ** 20, lo - 1, hi + 1], np.int64)


@pytest.mark.parametrize("ln,gn,name", CASES)
def test_build_mapping(gexec, ln, gn, name):
    part, dpart = _part(gexec, ln, gn, name)
    for n in SIZES:
        for rank in _local_parts(part, n):
            _build_mapping(gexec, ln, gn, _received(_rng("mapping", name, n, rank), part, rank, n), part, dpart,
                           _vec(n))


def test_build_mapping_beyond_the_grid_cap(gexec):
    """4.2 M received ids of 64 parts, every id many times: the second sort has 64 distinct keys and must keep
    the order of the first"""
    part, dpart = _part(gexec, "i64", "i64", "f")
    recv = _received(_rng("mapping large"), part, 5, LARGE)
    assert len(recv) == LARGE
    want = _build_mapping(gexec, "i64", "i64", recv, part, dpart, True)
    assert len(want[0]) == 63 and len(want[2]) > 150000


@pytest.mark.parametrize("ln,gn,name", CASES)
def test_map_to_local_and_global(gexec, ln, gn, name):
    """both directions in the three index spaces: queries on both sides of every range bound, owned ids,
    received ids, ids of target parts that were not received, ids outside the partition (-1, answered before
    the partition is read); every local id from -2 to 2 behind the end of the space, which takes
    find_local_range to the first and the last index of every range of a rank with several of them"""
    part, dpart = _part(gexec, ln, gn, name)
    rng = _rng("map", name)
    for rank in dr.interesting_parts(part):
        recv = _received(rng, part, rank, 400)
        mapping = (dr.build_mapping_v if name == "f" else dr.build_mapping)(recv, part)
        owned, local_size = dr.owned_ids(part, rank), int(part.sizes[rank])
        queries = np.concatenate([dr.random_ids(rng, part, 3000), owned[:200], owned[-200:], mapping[2],
                                  _outside(part)])
        for space in (0, 1, 2):
            lids = _map_to_local(gexec, ln, gn, queries, part, dpart, mapping, rank, space, True)
            small = _map_to_local(gexec, ln, gn, queries[-250:], part, dpart, mapping, rank, space, False)
            assert np.array_equal(small, lids[-250:]) and np.all(small[-6:] == -1)
            in_space = (np.isin(queries, owned) if space != 1 else np.zeros(len(queries), bool)) | \
                (np.isin(queries, mapping[2]) if space != 0 else np.zeros(len(queries), bool))
            assert np.array_equal(lids == -1, ~in_space)
            back = _map_to_global(gexec, ln, gn, lids, part, mapping, rank, space, True)
            assert np.array_equal(back[in_space], queries[in_space]) and np.all(back[~in_space] == -1)
            size = {0: local_size, 1: len(mapping[2]), 2: local_size + len(mapping[2])}[space]
            every = np.arange(-2, size + 3, dtype=np.int64)
            glob = _map_to_global(gexec, ln, gn, every, part, mapping, rank, space, True)
            assert np.array_equal(glob == -1, (every < 0) | (every >= size))
            _map_to_global(gexec, ln, gn, every[:150], part, mapping, rank, space, False)
            _map_to_global(gexec, ln, gn, every[-150:], part, mapping, rank, space, False)
        _map_to_local(gexec, ln, gn, queries[:0], part, dpart, mapping, rank, 2, False)     # n = 0
        _map_to_global(gexec, ln, gn, queries[:0], part, mapping, rank, 2, False)


@pytest.mark.parametrize("ln,gn", LG)
@pytest.mark.parametrize("name,rank,targets", [("b", 3, [1, 4]), ("c", 3, [1, 4]), ("d", 3, [1, 5]),
                                               ("d", 2, [1, 5]), ("b", 0, []), ("a", 0, [])])
def test_map_to_local_parts_that_are_not_targets(gexec, ln, gn, name, rank, targets):
    """every id of the partition is asked for.  Ids of a part that is no target - below the first target,
    between two, above the last - and ids of a target that were not received give -1 in the non-local space;
    in the combined space a received id sits at part_sizes[rank] + its flat position.  (d, 2): the rank owns
    nothing; no targets at all: the remote arrays are empty."""
    part, dpart = _part(gexec, ln, gn, name)
    recv = _received(_rng("targets", name), part, rank, 60, targets) if targets else np.zeros(0, np.int64)
    mapping = _build_mapping(gexec, ln, gn, recv, part, dpart, False)
    assert list(mapping[0]) == targets
    queries = np.concatenate([np.arange(part.bounds[0], part.bounds[-1]), _outside(part)])
    owner = part.pids[dr.find_range_v(queries[:-6], part.bounds)]
    got = {s: _map_to_local(gexec, ln, gn, queries, part, dpart, mapping, rank, s, False) for s in (0, 1, 2)}
    received = np.isin(queries[:-6], mapping[2])
    assert np.all(got[1][:-6][~received] == -1) and np.all(got[1][:-6][received] >= 0)
    for lo_hi in ((-1, min(targets, default=99)), (min(targets, default=0), max(targets, default=0)),
                  (max(targets, default=-1), 99)):
        asked = (owner > lo_hi[0]) & (owner < lo_hi[1]) & (owner != rank)
        assert not targets or asked.any()
        assert np.all(got[1][:-6][asked] == -1) and np.all(got[2][:-6][asked] == -1)
    assert np.array_equal(got[2][:-6][received], int(part.sizes[rank]) + got[1][:-6][received])
    assert np.array_equal(got[2][:-6][owner == rank], got[0][:-6][owner == rank])
    assert all(np.all(g[-6:] == -1) for g in got.values())


def test_map_to_local_and_global_beyond_the_grid_cap(gexec):
    part, dpart = _part(gexec, "i32", "i64", "f")
    rng = _rng("map large")
    mapping = dr.build_mapping_v(_received(rng, part, 5, 50000), part)
    queries = dr.random_ids(rng, part, LARGE)
    queries[-300:-6] = dr.owned_ids(part, 5)[:294]            # hits at the very end, beyond the cap
    queries[-6:] = _outside(part)
    lids = _map_to_local(gexec, "i32", "i64", queries, part, dpart, mapping, 5, 2, True)
    assert np.count_nonzero(lids >= 0) > 500000 and np.all(lids[-300:-6] >= 0) and np.all(lids[-6:] == -1)
    back = _map_to_global(gexec, "i32", "i64", lids, part, mapping, 5, 2, True)
    assert np.array_equal(back[lids >= 0], queries[lids >= 0])


# ------------------------------------------------------------------------------ assembly
def _assembly(gexec, ln, gn, vs, rows, cols, vals, part, dpart, lp, vec, seed):
    gt, nnz = NP[gn], len(rows)
    start = _rng("send_count", seed).integers(1, 9, part.num_parts).astype(np.int32)    # added to, not set
    hosts = [rows.astype(gt), cols.astype(gt), vals]
    devs = [Dev(gexec, h) for h in hosts]
    d_count = Dev(gexec, np.concatenate([start, np.full(3, int(CANARY), np.int32)]))
    pos, orig = _ints(gexec, nnz, gt), _ints(gexec, nnz, gt)
    _call(f"gkoc_assembly_count_non_owning_entries_{ln}_{gn}", gexec.stream, nnz, devs[0], dpart.ref, C.c_int32(lp),
          d_count, pos, orig)
    sync()
    count = start.copy()
    want_pos, want_orig = (dr.count_non_owning_entries_v if vec else dr.count_non_owning_entries)(rows, part, lp,
                                                                                                   count)
    got_count = d_count.get()
    assert tail_ok(got_count, part.num_parts) and np.array_equal(got_count[:part.num_parts], count)
    assert count[lp] == start[lp]                             # what local_part owns is not sent
    assert np.array_equal(_head(orig, nnz), want_orig.astype(gt))
    assert np.array_equal(_head(pos, nnz), want_pos.astype(gt))
    total = int(np.count_nonzero(want_orig >= 0))
    assert total == int((count - start).sum())
    srow, scol, sval = _ints(gexec, total, gt), _ints(gexec, total, gt), _vals(gexec, total, vals.dtype)
    _call("gkoc_assembly_fill_send_buffers_" + gn, gexec.stream, nnz, *devs, C.c_size_t(vs), pos, orig, srow, scol,
          sval)
    sync()
    want = (dr.fill_send_buffers_v if vec else dr.fill_send_buffers)(rows, cols, vals, want_pos, want_orig)
    assert np.array_equal(_head(srow, total), want[0].astype(gt))
    assert np.array_equal(_head(scol, total), want[1].astype(gt))
    assert same_bits(_head(sval, total), want[2])
    assert np.array_equal(_head(pos, nnz), want_pos.astype(gt)) and np.array_equal(_head(orig, nnz),
                                                                                   want_orig.astype(gt))
    assert _unchanged(devs, hosts) and dpart.unchanged()
    return total


@pytest.mark.parametrize("vs", list(VT))
@pytest.mark.parametrize("ln,gn,name", CASES)
def test_assembly_count_and_fill(gexec, ln, gn, name, vs):
    part, dpart = _part(gexec, ln, gn, name)
    for n in SIZES:
        rows, cols, vals = _entries(_rng("assembly", name, n), part, part, n, vs)
        for lp in _local_parts(part, n):
            _assembly(gexec, ln, gn, vs, rows, cols, vals, part, dpart, lp, _vec(n), n)


def test_assembly_beyond_the_grid_cap(gexec):
    part, dpart = _part(gexec, "i32", "i32", "f")
    rows, cols, vals = _entries(_rng("assembly large"), part, part, LARGE, 16)
    total = _assembly(gexec, "i32", "i32", 16, rows, cols, vals, part, dpart, 5, True, "large")
    assert total > 4000000


# ------------------------------------------------------------------------------ states, unsupported sizes
def _arena(gexec):
    """arena counters once everything handed back so far has been reclaimed: scratch goes back at the next
    scratch allocation, so synchronise and make one more small call (its own word is still out, every time)"""
    sync()
    d, result = Dev(gexec, np.array([1, 0], np.int32)), C.c_int(-5)
    _call("gkoc_partition_has_ordered_parts", gexec.stream, 2, d, C.byref(result))
    sync()
    info = gexec.arena_info()
    return info["num_allocations"], info["used_bytes"]


@pytest.mark.parametrize("ln,gn", LG)
def test_state_lifetimes(gexec, ln, gn):
    part, dpart = _part(gexec, ln, gn, "d")
    lt, gt, n, lp = NP[ln], NP[gn], 300, 3
    rows, cols, vals = _entries(_rng("states"), part, part, n, 8)
    recv = _received(_rng("states recv"), part, lp, n)
    devs = [Dev(gexec, rows.astype(gt)), Dev(gexec, cols.astype(gt)), Dev(gexec, vals), Dev(gexec, recv.astype(gt))]
    outs = [_ints(gexec, n, t) for t in (lt, lt, np.int64, lt, gt, np.int64)]
    m_outs = [_ints(gexec, n, t) for t in (np.int32, lt, gt, np.int64)]

    def separate(fill):
        state, a, b = C.c_void_p(0), C.c_int64(0), C.c_int64(0)
        _call(f"gkoc_dist_separate_local_nonlocal_count_{ln}_{gn}", gexec.stream, n, devs[0], devs[1], dpart.ref,
              dpart.ref, C.c_int32(lp), C.byref(state), C.byref(a), C.byref(b))
        assert state.value is not None and a.value + b.value > 0
        if fill:
            _call(f"gkoc_dist_separate_local_nonlocal_fill_{ln}_{gn}", gexec.stream, n, *devs[:3], C.c_size_t(8),
                  dpart.ref, dpart.ref, state, *outs)
        else:
            _call("gkoc_dist_separate_state_free", gexec.stream, state)

    def mapping(fill):
        state, a, b = C.c_void_p(0), C.c_int64(0), C.c_int64(0)
        _call(f"gkoc_index_map_build_mapping_count_{ln}_{gn}", gexec.stream, n, devs[3], dpart.ref, C.byref(state),
              C.byref(a), C.byref(b))
        assert state.value is not None and a.value > 0
        if fill:
            _call(f"gkoc_index_map_build_mapping_fill_{ln}_{gn}", gexec.stream, dpart.ref, state, *m_outs)
        else:
            _call("gkoc_index_map_mapping_state_free", gexec.stream, state)

    for fill in (True, False):                                # the warm-up round
        separate(fill), mapping(fill)
    before = _arena(gexec)
    for _ in range(200):
        for fill in (True, False):
            separate(fill), mapping(fill)
    assert _arena(gexec) == before
    # NULL: the free functions accept it, a fill call does nothing
    null = C.c_void_p(0)
    _call("gkoc_dist_separate_state_free", gexec.stream, null)
    _call("gkoc_index_map_mapping_state_free", gexec.stream, null)
    _call(f"gkoc_dist_separate_local_nonlocal_fill_{ln}_{gn}", gexec.stream, n, *devs[:3], C.c_size_t(8), dpart.ref,
          dpart.ref, null, *[_ints(gexec, n, t) for t in (lt, lt, np.int64, lt, gt, np.int64)])
    fresh = [_ints(gexec, n, t) for t in (np.int32, lt, gt, np.int64)]
    _call(f"gkoc_index_map_build_mapping_fill_{ln}_{gn}", gexec.stream, dpart.ref, null, *fresh)
    sync()
    assert all(_untouched(o, n) for o in fresh)               # nothing written
    assert _arena(gexec) == before


@pytest.mark.parametrize("ln,gn", LG)
def test_unsupported_value_size(gexec, ln, gn):
    """value_size 2: the not-supported status, nothing written; separate_fill still releases its state"""
    from ginkgo_amd._lib import NotSupported
    part, dpart = _part(gexec, ln, gn, "d")
    lt, gt, n, lp = NP[ln], NP[gn], 300, 3
    rows, cols, _ = _entries(_rng("unsupported"), part, part, n, 8)
    vals = np.arange(n, dtype=np.float16)
    devs = [Dev(gexec, rows.astype(gt)), Dev(gexec, cols.astype(gt)), Dev(gexec, vals)]

    def separate(vs):
        state, a, b = C.c_void_p(0), C.c_int64(0), C.c_int64(0)
        _call(f"gkoc_dist_separate_local_nonlocal_count_{ln}_{gn}", gexec.stream, n, devs[0], devs[1], dpart.ref,
              dpart.ref, C.c_int32(lp), C.byref(state), C.byref(a), C.byref(b))
        outs = [_ints(gexec, n, t) for t in (lt, lt, np.int64, lt, gt, np.int64)]
        try:
            _call(f"gkoc_dist_separate_local_nonlocal_fill_{ln}_{gn}", gexec.stream, n, devs[0], devs[1],
                  Dev(gexec, np.zeros(n, np.int64)), C.c_size_t(vs), dpart.ref, dpart.ref, state, *outs)
        finally:
            sync()
        return outs

    separate(8)
    before = _arena(gexec)
    for _ in range(3):
        with pytest.raises(NotSupported):
            separate(2)
    assert _arena(gexec) == before
    outs = [_ints(gexec, n, t) for t in (lt, lt, np.int64, lt, gt, np.int64)]
    state, a, b = C.c_void_p(0), C.c_int64(0), C.c_int64(0)
    _call(f"gkoc_dist_separate_local_nonlocal_count_{ln}_{gn}", gexec.stream, n, devs[0], devs[1], dpart.ref,
          dpart.ref, C.c_int32(lp), C.byref(state), C.byref(a), C.byref(b))
    with pytest.raises(NotSupported):
        _call(f"gkoc_dist_separate_local_nonlocal_fill_{ln}_{gn}", gexec.stream, n, *devs, C.c_size_t(2), dpart.ref,
              dpart.ref, state, *outs)
    sync()
    assert all(_untouched(o, n) for o in outs)

    out = _vals(gexec, int(part.sizes[lp]) * LD, np.float16)
    with pytest.raises(NotSupported):
        _call(f"gkoc_dist_vector_build_local_{ln}_{gn}", gexec.stream, n, devs[0], Dev(gexec, (cols % 3).astype(gt)),
              devs[2], C.c_size_t(2), dpart.ref, C.c_int32(lp), out, LD)
    sync()
    assert _untouched(out, int(part.sizes[lp]) * LD)

    count = np.zeros(part.num_parts, np.int32)
    pos, orig = dr.count_non_owning_entries_v(rows, part, lp, count)
    bufs = [_ints(gexec, n, gt), _ints(gexec, n, gt), _vals(gexec, n, np.float16)]
    with pytest.raises(NotSupported):
        _call("gkoc_assembly_fill_send_buffers_" + gn, gexec.stream, n, *devs, C.c_size_t(2),
              Dev(gexec, pos.astype(gt)), Dev(gexec, orig.astype(gt)), *bufs)
    sync()
    assert all(_untouched(o, n) for o in bufs)


# ------------------------------------------------------------------------------ the two distributed paths
@pytest.mark.parametrize("it", list(NP))
def test_split_agrees_with_separate_and_build_mapping(gexec, it):
    """include/gko_cdna4.h says of gkoc_dist_split_*, the path ginkgo_amd/distributed.py takes, that recv_gidx
    is index_map's ordering for contiguous partitions: for every rank of a contiguous partition, the split of
    the rank's rows gives the remote_global_idxs of build_mapping on the non-local columns of
    separate_local_nonlocal, and the same local block entry for entry"""
    t, rng = NP[it], _rng("two paths")
    part = dr.partition("b")
    n = int(part.bounds[-1])
    dpart = DevPartition(gexec, t, t, part)
    per_row = rng.integers(0, 12, n)
    per_row[5] = 0
    coo_rows = np.repeat(np.arange(n), per_row)
    coo_cols = np.concatenate([np.sort(rng.choice(n, k, replace=False)) for k in per_row]).astype(np.int64)
    coo_vals = rng.uniform(-1, 1, len(coo_rows))
    ptrs = np.concatenate([[0], np.cumsum(per_row)])
    for r in range(part.num_parts):
        lo, hi = int(part.bounds[r]), int(part.bounds[r + 1])
        # path 1: the rank's rows as Csr with global columns, split
        mine = slice(int(ptrs[lo]), int(ptrs[hi]))
        hosts = [(ptrs[lo:hi + 1] - ptrs[lo]).astype(t), coo_cols[mine].astype(t), coo_vals[mine]]
        devs = [Dev(gexec, h) for h in hosts]
        rows_r = hi - lo
        col_map, l_ptrs, nl_full = (Dev(gexec, np.zeros(k, t)) for k in (n + 1, rows_r + 1, rows_r + 1))
        cnt = [C.c_int64(-5) for _ in range(4)]
        _call("gkoc_dist_split_count_" + it, gexec.stream, rows_r, devs[0], devs[1], lo, hi, n, col_map, l_ptrs,
              nl_full, *[C.byref(c) for c in cnt])
        n_halo, nnz_l, nnz_nl, n_nl_rows = (c.value for c in cnt)
        l_cols, l_vals = _ints(gexec, nnz_l, t), _vals(gexec, nnz_l, np.float64)
        nl_rows, nl_ptrs, nl_cols = _ints(gexec, n_nl_rows, t), _ints(gexec, n_nl_rows + 1, t), _ints(gexec, nnz_nl, t)
        nl_vals, recv_gidx = _vals(gexec, nnz_nl, np.float64), _ints(gexec, n_halo, t)
        _call(f"gkoc_dist_split_fill_f64_{it}", gexec.stream, rows_r, *devs, lo, hi, n, col_map, l_ptrs, nl_full,
              l_cols, l_vals, nl_rows, nl_ptrs, nl_cols, nl_vals, recv_gidx)
        sync()
        assert _unchanged(devs, hosts)
        # path 2: the whole matrix as triplets, separated for local_part = r, the index map of what is left
        want = _separate(gexec, it, it, 8, coo_rows, coo_cols, coo_vals, (part, dpart), (part, dpart), r, True)
        mapping = _build_mapping(gexec, it, it, want[4], part, dpart, True)
        assert np.array_equal(_head(recv_gidx, n_halo), mapping[2].astype(t))
        assert (nnz_l, nnz_nl) == (len(want[0]), len(want[3]))
        local_ptrs = l_ptrs.get().astype(np.int64)
        assert np.array_equal(np.repeat(np.arange(rows_r), np.diff(local_ptrs)), want[0])
        assert np.array_equal(_head(l_cols, nnz_l), want[1].astype(t))
        assert same_bits(_head(l_vals, nnz_l), want[2])
        # and the non-local block: the same entries, columns as positions in recv_gidx
        rows_nl = np.repeat(nl_rows.get()[:n_nl_rows].astype(np.int64), np.diff(nl_ptrs.get()[:n_nl_rows + 1]))
        assert np.array_equal(rows_nl, want[3])
        assert np.array_equal(mapping[2][_head(nl_cols, nnz_nl).astype(np.int64)], want[4])
        assert same_bits(_head(nl_vals, nnz_nl), want[5])
