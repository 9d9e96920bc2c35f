"""experimental::distributed::Partition's kernels and the partition helpers (csrc/dist_setup.hip:
gkoc_partition_*, gkoc_partition_helpers_*) through the C ABI against tests/dist_setup_refs.py.

Everything is integers: every comparison is np.array_equal.  Inputs are read back and compared bit for bit
after the call; every device output is pre-filled with a sentinel, is longer than what the operation defines
(the rest must keep the sentinel) and is followed by canaries; host outputs are compared too.  The large cases
(a little above 2048^2 ids, about 2.1 M ranges) lie beyond the grid cap of the launchers and take the scan
through three levels; they are compared element for element with the vectorised references."""
import ctypes as C

import numpy as np
import pytest

import dist_setup_refs as dr
from binding_gpu import SENTINEL, Dev, call as _call, grid_cap_rows, head_of, out_buf as _out, same_bits, sync

pytestmark = pytest.mark.gpu

NP = {"i32": np.int32, "i64": np.int64}
LG = [("i32", "i32"), ("i32", "i64"), ("i64", "i64")]
SIZES = [0, 1, 2, 255, 256, 257, 2047, 2048, 2049, 100003]
LARGE = 2048 * 2048 + 257
PAD = 4                                         # entries behind the defined output that must keep the sentinel


def _ints(gexec, n, t):
    return _out(gexec, n + PAD, t, fill=SENTINEL)


def _head(out, n):
    return head_of(out, n + PAD, n)


def _rng(*key):
    return np.random.default_rng(sum(map(ord, "".join(map(str, key)))))


def _pick(n, loop, vec):
    return loop if n <= 300 else vec


def partition_names(gn):
    return ["a", "b", "c", "d", "f"] + (["e"] if gn == "i64" else [])


# ------------------------------------------------------------------------------ count_ranges / build_from_mapping
def _from_mapping(gexec, gn, mapping):
    n = len(mapping)
    d_map = Dev(gexec, mapping)
    count = C.c_int64(-5)
    _call("gkoc_partition_count_ranges", gexec.stream, n, d_map, C.byref(count))
    assert count.value == _pick(n, dr.count_ranges, dr.count_ranges_v)(mapping)
    bounds, pids = _ints(gexec, count.value + 1, NP[gn]), _ints(gexec, count.value, np.int32)
    _call("gkoc_partition_build_from_mapping_" + gn, gexec.stream, n, d_map, bounds, pids)
    sync()
    want_b, want_p = _pick(n, dr.build_from_mapping, dr.build_from_mapping_v)(mapping)
    got_b, got_p = _head(bounds, count.value + 1), _head(pids, count.value)
    assert same_bits(d_map.get(), mapping)
    return got_b, got_p, want_b, want_p


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("gn", list(NP))
def test_count_ranges_and_build_from_mapping(gexec, gn, n):
    for parts, run in ((dr.D_MAPPING_PARTS, 5), ([3], 1), (np.arange(64), 1)):
        mapping = dr.mapping_runs(_rng("mapping", n, run), n, parts, run)
        got_b, got_p, want_b, want_p = _from_mapping(gexec, gn, mapping)
        assert np.array_equal(got_b, want_b) and np.array_equal(got_p, want_p)
        assert got_b[0] == 0 and got_b[-1] == n           # n = 0: range_bounds[0] = 0 is all that is written


@pytest.mark.parametrize("gn", list(NP))
def test_build_from_mapping_beyond_the_grid_cap(gexec, gn):
    assert LARGE + 1 > 2 * grid_cap_rows()
    mapping = dr.mapping_runs(_rng("large mapping"), LARGE, np.arange(64), 3)
    mapping[-300:] = 5                                    # the last range starts and ends beyond the cap
    got_b, got_p, want_b, want_p = _from_mapping(gexec, gn, mapping)
    assert np.array_equal(got_b, want_b) and np.array_equal(got_p, want_p)
    assert len(got_p) > grid_cap_rows()


# ------------------------------------------------------------------------------ build_from_contiguous
@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("gn", list(NP))
def test_build_from_contiguous(gexec, gn, mapped):
    for num_ranges in [0, 1, 2, 7, 255, 256, 257, 2049, 100003]:
        rng = _rng("contiguous", num_ranges)
        # ranges[0] is not zero: bounds[0] = 0 comes from the kernel, not from the input
        ranges = np.concatenate([[7], 7 + np.cumsum(rng.integers(0, 5, num_ranges))]).astype(NP[gn])
        mapping = rng.permutation(num_ranges).astype(np.int32) if mapped else None
        d_ranges, d_map = Dev(gexec, ranges), (Dev(gexec, mapping) if mapped else None)
        bounds, pids = _ints(gexec, num_ranges + 1, NP[gn]), _ints(gexec, num_ranges, np.int32)
        _call("gkoc_partition_build_from_contiguous_" + gn, gexec.stream, num_ranges, d_ranges, d_map, bounds, pids)
        sync()
        want_b, want_p = _pick(num_ranges, dr.build_from_contiguous, dr.build_from_contiguous_v)(ranges, mapping)
        assert np.array_equal(_head(bounds, num_ranges + 1), want_b)
        assert np.array_equal(_head(pids, num_ranges), want_p)
        assert same_bits(d_ranges.get(), ranges) and (not mapped or same_bits(d_map.get(), mapping))


@pytest.mark.parametrize("gn", list(NP))
def test_build_ranges_from_global_size(gexec, gn):
    ctype = {"i32": C.c_int32, "i64": C.c_int64}[gn]
    for num_parts in [1, 2, 7, 255, 256, 257, 2049, 100003]:
        sizes = [0, 1, num_parts - 1, num_parts, num_parts + 1, 7 * num_parts + 3]
        sizes += [2 ** 31 - 1] if gn == "i32" else [2 ** 40 + 5]
        for size in sizes:
            ranges = _ints(gexec, num_parts + 1, NP[gn])
            _call("gkoc_partition_build_ranges_from_global_size_" + gn, gexec.stream, C.c_int32(num_parts),
                  ctype(size), ranges)
            sync()
            want = _pick(num_parts, dr.build_ranges_from_global_size, dr.build_ranges_from_global_size_v)(
                num_parts, size)
            assert np.array_equal(_head(ranges, num_parts + 1), want), (num_parts, size)


# ------------------------------------------------------------------------------ starting indices, ranges by part
def _starting_indices(gexec, ln, gn, bounds, pids, num_parts, vec):
    num_ranges = len(pids)
    d_bounds, d_pids = Dev(gexec, bounds.astype(NP[gn])), Dev(gexec, pids.astype(np.int32))
    ranks, sizes = _ints(gexec, num_ranges, NP[ln]), _ints(gexec, num_parts, NP[ln])
    empty = C.c_int32(-5)
    _call(f"gkoc_partition_build_starting_indices_{ln}_{gn}", gexec.stream, d_bounds, d_pids, num_ranges,
          C.c_int32(num_parts), C.byref(empty), ranks, sizes)
    sync()
    want = (dr.build_starting_indices_v if vec else dr.build_starting_indices)(bounds, pids, num_parts)
    assert np.array_equal(_head(ranks, num_ranges), want[0])
    assert np.array_equal(_head(sizes, num_parts), want[1])
    assert empty.value == want[2]
    assert same_bits(d_bounds.get(), bounds.astype(NP[gn])) and same_bits(d_pids.get(), pids.astype(np.int32))


def _ranges_by_part(gexec, pids, num_parts, vec):
    num_ranges = len(pids)
    d_pids = Dev(gexec, pids.astype(np.int32))
    ids, sizes = _ints(gexec, num_ranges, np.int64), _ints(gexec, num_parts, np.int64)   # (uint64 ids as int64)
    _call("gkoc_partition_build_ranges_by_part", gexec.stream, d_pids, num_ranges, C.c_int32(num_parts), ids, sizes)
    sync()
    want = (dr.build_ranges_by_part_v if vec else dr.build_ranges_by_part)(pids, num_parts)
    assert np.array_equal(_head(ids, num_ranges), want[0])
    assert np.array_equal(_head(sizes, num_parts), want[1])
    assert same_bits(d_pids.get(), pids.astype(np.int32))


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e", "f"])
@pytest.mark.parametrize("ln,gn", LG)
def test_build_starting_indices(gexec, ln, gn, name):
    if name == "e" and gn == "i32":
        part = dr.partition("d", offset=2 ** 30)          # (e) needs 64 bits; the same ranges high in 32 bits
    else:
        part = dr.partition(name)
    _starting_indices(gexec, ln, gn, part.bounds, part.pids, part.num_parts, name == "f")


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "f"])
def test_build_ranges_by_part(gexec, name):
    part = dr.partition(name)
    _ranges_by_part(gexec, part.pids, part.num_parts, name == "f")


@pytest.mark.parametrize("ln,gn", LG)
def test_partition_builders_without_ranges_or_parts(gexec, ln, gn):
    """num_ranges = 0: every part is empty, sizes are zero, ranks are not touched; num_parts = 0 writes nothing"""
    for num_parts in (0, 1, 3):
        _starting_indices(gexec, ln, gn, np.zeros(1, np.int64), np.zeros(0, np.int32), num_parts, False)
        _ranges_by_part(gexec, np.zeros(0, np.int32), num_parts, False)
    for num_ranges in (1, 2, 257):                        # one part that owns everything, and one that owns nothing
        bounds = np.arange(num_ranges + 1, dtype=np.int64) * 3
        _starting_indices(gexec, ln, gn, bounds, np.zeros(num_ranges, np.int32), 1, False)
        _starting_indices(gexec, ln, gn, bounds, np.ones(num_ranges, np.int32), 2, False)
        _ranges_by_part(gexec, np.ones(num_ranges, np.int32), 2, False)


@pytest.mark.parametrize("ln,gn", [("i64", "i64"), ("i32", "i32")])
def test_starting_indices_and_ranges_by_part_beyond_the_grid_cap(gexec, ln, gn):
    """about 2.1 M ranges of 64 parts: one range per thread would stop at the cap, the sort has few distinct
    keys (its stability decides the ranks) and the scan has three levels"""
    num_ranges = grid_cap_rows() + 257
    rng = _rng("large ranges")
    pids = rng.integers(0, 64, num_ranges).astype(np.int32)
    pids[pids == 17] = 18                                 # an empty part
    bounds = np.concatenate([[0], np.cumsum(rng.integers(0, 3, num_ranges))])
    _starting_indices(gexec, ln, gn, bounds, pids, 64, True)
    if ln == "i64":
        _ranges_by_part(gexec, pids, 64, True)


# ------------------------------------------------------------------------------ has_ordered_parts
def _ordered(gexec, pids):
    d = Dev(gexec, pids.astype(np.int32))
    result = C.c_int(-5)
    _call("gkoc_partition_has_ordered_parts", gexec.stream, len(pids), d, C.byref(result))
    assert same_bits(d.get(), pids.astype(np.int32)) and result.value in (0, 1)
    assert bool(result.value) == dr.has_ordered_parts_v(pids)
    return bool(result.value)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 255, 256, 257, 2049, 100003, 2 * 1024 * 2048 + 257])
def test_has_ordered_parts(gexec, n):
    pids = np.sort(_rng("ordered", n).integers(0, 50, n)).astype(np.int32)
    assert _ordered(gexec, pids)
    assert _ordered(gexec, np.zeros(n, np.int32))
    for wrong in sorted({1, n // 2, n - 1}) if n >= 2 else []:       # exactly one pair out of order
        bad = pids + 1
        bad[wrong:] += 3
        bad[wrong] = bad[wrong - 1] - 1
        assert np.count_nonzero(np.diff(bad) < 0) == 1
        assert not _ordered(gexec, bad)
    for name in ("b", "c", "d"):
        assert _ordered(gexec, dr.partition(name).pids) == (name == "b")


# ------------------------------------------------------------------------------ partition helpers
def _pairs(rng, n, gn, base):
    """n consecutive (start, end) pairs; zero-length ranges give equal starts"""
    offsets = base + np.concatenate([[11], 11 + np.cumsum(rng.integers(0, 4, n))])
    return np.stack([offsets[:-1], offsets[1:]], 1).reshape(-1).astype(NP[gn]), offsets.astype(NP[gn])


@pytest.mark.parametrize("order", ["sorted", "reversed", "random"])
@pytest.mark.parametrize("gn", list(NP))
def test_sort_by_range_start(gexec, gn, order):
    for n in [0, 1, 2, 3, 255, 256, 257, 2047, 2048, 2049, 100003]:
        rng = _rng("sort", n, order)
        for base in [0] + ([2 ** 33 + 5] if gn == "i64" else [2 ** 30]):     # the sort's upper key bits
            se, _ = _pairs(rng, n, gn, base)
            perm = {"sorted": np.arange(n), "reversed": np.arange(n)[::-1], "random": rng.permutation(n)}[order]
            se_in = se.reshape(-1, 2)[perm].reshape(-1)
            pids_in = rng.permutation(n).astype(np.int32)       # distinct: the ids tell equal starts apart
            d_se, d_pids = _out(gexec, 2 * n, NP[gn], fill=SENTINEL), _out(gexec, n, np.int32, fill=SENTINEL)
            d_se.t[:se_in.nbytes] = Dev(gexec, se_in).t[:se_in.nbytes]
            d_pids.t[:pids_in.nbytes] = Dev(gexec, pids_in).t[:pids_in.nbytes]
            _call("gkoc_partition_helpers_sort_by_range_start_" + gn, gexec.stream, n, d_se, d_pids)
            sync()
            want_se, want_pids = _pick(n, dr.sort_by_range_start, dr.sort_by_range_start_v)(se_in, pids_in)
            assert np.array_equal(head_of(d_se, 2 * n, 2 * n), want_se), (n, base)
            assert np.array_equal(head_of(d_pids, n, n), want_pids), (n, base)   # equal starts: input order kept


@pytest.mark.parametrize("gn", list(NP))
def test_check_consecutive_and_compress_ranges(gexec, gn):
    def check(se):
        d = Dev(gexec, se)
        result = C.c_int(-5)
        _call("gkoc_partition_helpers_check_consecutive_ranges_" + gn, gexec.stream, len(se) // 2, d,
              C.byref(result))
        assert same_bits(d.get(), se) and result.value in (0, 1)
        assert bool(result.value) == dr.check_consecutive_ranges_v(se) == dr.check_consecutive_ranges(se)
        return bool(result.value)

    for n in [0, 1, 2, 3, 255, 256, 257, 2049, 100003]:
        se, offsets = _pairs(_rng("consecutive", n), n, gn, 0)
        assert check(se)                                  # 0 or 1 pair: true
        for wrong in sorted({0, (n - 1) // 2, n - 2}) if n >= 2 else []:   # the first, a middle, the last pair
            bad = se.copy()
            bad[2 * wrong + 2] += 1
            assert not check(bad)
            bad[2 * wrong + 2] -= 2
            assert not check(bad)
        d_se = Dev(gexec, se)
        # num_parts = 0 has no pair to take offsets[0] from: n_offsets = 0 writes nothing
        n_offsets = n + 1 if n else 0
        out = _ints(gexec, n_offsets, NP[gn])
        _call("gkoc_partition_helpers_compress_ranges_" + gn, gexec.stream, n_offsets, d_se, out)
        sync()
        got = _head(out, n_offsets)
        if n:
            assert np.array_equal(got, _pick(n, dr.compress_ranges, dr.compress_ranges_v)(se))
            assert np.array_equal(got, offsets)
        assert same_bits(d_se.get(), se)
