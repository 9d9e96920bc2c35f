"""The cached column-offset plan of the CSR SpMV (csrc/csr_offsets.hpp, launcher in csrc/csr_spmv.hip, plan cache in
csrc/csr_structure.hip).  The matrices, the host model of the plan and the helpers are tests/csr_offsets_cases.py (checked on the CPU by
tests/test_csr_offsets_cases_cpu.py); the routes that drop a plan are tests/test_csr_offsets_routes_gpu.py.

Index arrays come from the library's allocator even when tiny (only those ever get a plan).  Every product is
compared BIT FOR BIT (NaN positions included) with the sequential oracle and with the same product under
GKOC_TUNE_CSR_OFFSETS = 2 (the row-segment kernel alone), runs twice with the same bits, and the plan's own
counters (gkoc_csr_plan_info) must show that the offsets kernel did the work: the fallback cannot pass alone.
"""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import csr_offsets_cases as oc
import csr_spmv_cases as sc
from csr_offsets_cases import (KEY, KEY_LONG_ROWS, KEY_SEGS_PER_WAVE, arena_csr, arena_tensor, band_rows, bits,
                               check_all_modes, from_rows, key, plain, plan_info, plan_info_at, reference, run,
                               two_structures)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- matrices (host, int32)
def stencil27(oracle, g, dtype, seed=0):
    rp, ci, v = oracle.stencil_csr(3, g)
    rng = np.random.default_rng(seed)
    v = (v * rng.uniform(0.5, 1.5, len(v))).astype(dtype)
    return (g ** 3, g ** 3), rp, ci, v


STENCILS = ["27pt-3", "27pt-5", "27pt-12", "tri-65", "tri-130", "band-100x300"]


def stencil_case(oracle, name, dtype):
    if name.startswith("27pt"):
        return stencil27(oracle, int(name.split("-")[1]), dtype)
    if name.startswith("tri"):
        n = int(name.split("-")[1])
        return from_rows(band_rows(n, n, (-1, 0, 1)), n, dtype)
    return from_rows(band_rows(100, 300, (-2, 0, 3, 150, 199)), 300, dtype)


# ---------------------------------------------------------------- 1. stencils
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", STENCILS)
def test_stencils(gexec, oracle, name, dtype):
    """27-point at g = 3 (one partial segment), 5 (the last segment has 61 rows), 12 (segments span x-lines and
    planes); tridiagonal n = 65, 130; a non-square band: every segment is eligible"""
    m = stencil_case(oracle, name, np.dtype(dtype))
    check_all_modes(gexec, oracle, m, eligible=-(-m[0][0] // 64))


def test_fused_dot_two_segments_per_wave(gexec, oracle):
    """from 65536 segments on a wave owns TWO segments (plan_segments) and adds both to its part of <b, c>: a
    tridiagonal matrix of 65536 * 64 + 70 rows (65538 segments, the last one partial): the smallest size with that
    path.  c
    against the oracle, c and the dot against the row-segment kernel's bits."""
    dtype = np.dtype(np.float64)
    n = 65536 * 64 + 70
    r = np.arange(n, dtype=np.int64)
    cols = np.stack((r - 1, r, r + 1), axis=1)
    keep = (cols >= 0) & (cols < n)
    rp = np.zeros(n + 1, np.int32)
    rp[1:] = np.cumsum(keep.sum(axis=1))
    ci = cols[keep].astype(np.int32)
    rng = np.random.default_rng(8)
    v = rng.uniform(0.5, 1.5, len(ci)).astype(dtype)
    b = rng.uniform(-1, 1, n).astype(dtype)
    a = arena_csr(gexec, (n, n), rp, ci, v)
    with key(1):
        got = run(gexec, a, b, "dot", None)
        info = plan_info(a)
    assert info["state"] == 1 and info["eligible"] == info["segments"] == 65538 and info["products"] == 2, info
    with key(2):
        old = run(gexec, a, b, "dot", None)
    assert np.array_equal(bits(got), bits(old))
    assert np.array_equal(bits(got[:n]), bits(oracle.csr_spmv(rp, ci, v, b)))


# ---------------------------------------------------------------- 2. eligibility edges
def edge_rows(n_offsets, spoil):
    """192 rows, three segments.  Segment 0: a band.  Segment 1: rows that use n_offsets distinct offsets between
    them (row r stores the diagonal and offsets 2 (r % 16) + 2, + 3 ... so that the union is exactly n_offsets).
    Segment 2: a band, optionally with an unsorted row or a duplicated column."""
    n = 192
    rows = band_rows(n, 400, (-1, 0, 1))
    offs = [0] + [2 + i for i in range(n_offsets - 1)]
    for r in range(64, 128):
        k = (r - 64) % (n_offsets - 3)
        rows[r] = [r + o for o in offs[k:k + 4]]
    if spoil == "unsorted":
        rows[150] = [151, 149, 150]
    elif spoil == "duplicate":
        rows[150] = [149, 150, 150]
    return rows


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n_offsets,spoil,eligible", [(32, None, 3), (33, None, 2), (32, "unsorted", 2),
                                                      (32, "duplicate", 2)])
def test_eligibility_edges(gexec, oracle, n_offsets, spoil, eligible, dtype):
    """exactly 32 offsets: eligible; 33: not; an unsorted row or a duplicated column: that segment is not.  The
    segments that are not eligible are multiplied by the row-segment kernel in the same product."""
    rows = edge_rows(n_offsets, spoil)
    got_offsets = {c - r for r in range(64, 128) for c in rows[r]}
    assert len(got_offsets) == n_offsets
    check_all_modes(gexec, oracle, from_rows(rows, 400, np.dtype(dtype)), eligible, modes=("plain", "adv", "beta0"))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_empty_rows_in_an_eligible_segment(gexec, oracle, dtype):
    rows = band_rows(130, 130, (-1, 0, 1))
    for r in (0, 5, 6, 63, 64, 100, 129):
        rows[r] = []
    check_all_modes(gexec, oracle, from_rows(rows, 130, np.dtype(dtype)), eligible=3)


# ---------------------------------------------------------------- 3. absent slots
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_absent_slots_do_not_touch_the_sum(gexec, oracle, dtype):
    """x[64] = inf and x[0] = nan: only the rows that store those columns change (an absent slot adds nothing,
    not 0 * x); x all -0.0 under positive values: the oracle's signed zeros"""
    dtype = np.dtype(dtype)
    n = 130
    m = from_rows(band_rows(n, n, (-1, 0, 1)), n, dtype)
    b = np.random.default_rng(3).uniform(-1, 1, n).astype(dtype)
    b[64], b[0] = np.inf, np.nan
    check_all_modes(gexec, oracle, m, eligible=3, b=b)
    ref = oracle.csr_spmv(m[1], m[2], m[3], b)
    assert set(np.flatnonzero(~np.isfinite(ref))) == {0, 1, 63, 64, 65}
    shape, rp, ci, v = m
    check_all_modes(gexec, oracle, (shape, rp, ci, np.abs(v)), eligible=3, b=np.full(n, -0.0, dtype))


# ---------------------------------------------------------------- 4. invalidation
@pytest.mark.parametrize("how", ["memcpy_h2d", "structure_changed", "free"])
def test_invalidation(gexec, oracle, how):
    from ginkgo_amd import _lib
    dtype = np.dtype(np.float64)
    m1, m2 = two_structures(dtype)
    assert np.array_equal(m1[1], m2[1]) and not np.array_equal(m1[2], m2[2])
    b = np.random.default_rng(9).uniform(-1, 1, m1[0][1]).astype(dtype)
    with key(1):
        a = arena_csr(gexec, *m1)
        assert np.array_equal(bits(plain(gexec, a, b)), bits(oracle.csr_spmv(m1[1], m1[2], m1[3], b)))
        assert plan_info(a)["state"] == 1 and plan_info(a)["products"] == 2
        gexec.synchronize()
        if how == "memcpy_h2d":
            _lib.call("gkoc_memcpy_h2d", C.c_void_p(a.col_idxs.data_ptr()), m2[2].ctypes.data_as(C.c_void_p),
                      C.c_size_t(m2[2].nbytes), gexec.stream)
            gexec.synchronize()
        elif how == "structure_changed":
            a.col_idxs.copy_(torch.from_numpy(m2[2]))
            a.structure_changed()
        else:
            old = (a.row_ptrs.data_ptr(), a.col_idxs.data_ptr())
            del a
            gc.collect()
            assert plan_info_at(*old)["state"] == -1, "gkoc_free drops the plan of the arrays it frees"
            a = arena_csr(gexec, *m2)
        assert plan_info(a)["state"] == -1, "the old plan is gone"
        got = plain(gexec, a, b)
        assert np.array_equal(bits(got), bits(oracle.csr_spmv(m2[1], m2[2], m2[3], b)))
        info = plan_info(a)
        assert info["state"] == 1 and info["products"] == 2 and info["eligible"] == 3, info


def test_sort_by_column_index_drops_the_plan(gexec, oracle):
    dtype = np.dtype(np.float64)
    m, _ = two_structures(dtype)
    b = np.random.default_rng(9).uniform(-1, 1, m[0][1]).astype(dtype)
    with key(1):
        a = arena_csr(gexec, *m)
        plain(gexec, a, b)
        assert plan_info(a)["state"] == 1
        a.sort_by_column_index()
        assert plan_info(a)["state"] == -1
        assert np.array_equal(bits(plain(gexec, a, b)), bits(oracle.csr_spmv(m[1], m[2], m[3], b)))


# ---------------------------------------------------------------- 5. default timing
def test_default_builds_at_the_second_product(gexec, oracle):
    import ginkgo_amd as g
    dtype = np.dtype(np.float64)
    m = stencil27(oracle, 5, dtype)
    b = np.random.default_rng(2).uniform(-1, 1, m[0][1]).astype(dtype)
    ref = oracle.csr_spmv(m[1], m[2], m[3], b)
    with key(0):
        a = arena_csr(gexec, *m)
        db = g.Dense.from_numpy(gexec, b.reshape(-1, 1))
        states = []
        for _ in range(3):
            dc = g.Dense.from_numpy(gexec, np.full((len(ref), 1), np.nan, dtype))
            a.apply(db, dc)
            assert np.array_equal(bits(dc.to_numpy().reshape(-1)), bits(ref))
            info = plan_info(a)
            states.append((info["state"], info["products"]))
        assert states == [(0, 0), (1, 1), (1, 2)], states


# ---------------------------------------------------------------- 6. stream capture
@pytest.mark.parametrize("built_before", [False, True])
def test_stream_capture(gexec, oracle, built_before):
    """a first product inside a capture builds nothing and is right; a plan built before is used inside a capture
    (no synchronisation: the capture would fail)"""
    import ginkgo_amd as g
    dtype = np.dtype(np.float64)
    m = stencil27(oracle, 5, dtype)
    b = np.random.default_rng(4).uniform(-1, 1, m[0][1]).astype(dtype)
    ref = oracle.csr_spmv(m[1], m[2], m[3], b)
    with key(1):
        a = arena_csr(gexec, *m)
        db = g.Dense.from_numpy(gexec, b.reshape(-1, 1))
        dc = g.Dense.from_numpy(gexec, np.full((len(ref), 1), np.nan, dtype))
        if built_before:
            a.apply(db, dc)
            assert plan_info(a)["state"] == 1
        torch.cuda.synchronize()
        dc.fill(np.nan)
        side = torch.cuda.Stream(device=gexec.device)
        graph = torch.cuda.CUDAGraph()
        side.wait_stream(torch.cuda.current_stream(gexec.device))
        with torch.cuda.graph(graph, stream=side):
            a.apply(db, dc)
        torch.cuda.current_stream(gexec.device).wait_stream(side)
        info = plan_info(a)
        assert (info["state"], info["products"]) == ((1, 2) if built_before else (0, 0)), info
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(dc.to_numpy().reshape(-1)), bits(ref))
        del graph
        # the next eager product builds (or keeps using) the plan
        dc.fill(np.nan)
        a.apply(db, dc)
        assert np.array_equal(bits(dc.to_numpy().reshape(-1)), bits(ref))
        assert plan_info(a)["state"] == 1


# ---------------------------------------------------------------- 7. foreign pointers
def test_foreign_pointers_never_get_a_plan(gexec, oracle):
    import ginkgo_amd as g
    dtype = np.dtype(np.float64)
    shape, rp, ci, v = stencil27(oracle, 5, dtype)
    b = np.random.default_rng(6).uniform(-1, 1, shape[1]).astype(dtype)
    with key(1):
        a = g.Csr(gexec, shape, torch.from_numpy(v).to(gexec.device), torch.from_numpy(ci).to(gexec.device),
                  torch.from_numpy(rp).to(gexec.device))
        for _ in range(2):
            assert np.array_equal(bits(plain(gexec, a, b)), bits(oracle.csr_spmv(rp, ci, v, b)))
        assert plan_info(a)["state"] == -1


# ================================================================ kernel and launcher edges (csr_offsets_cases.py)
CASES = list(oc.builders())


def built(name, dtype):
    if name.startswith("full-"):
        _, t, lead = name.split("-")
        return oc.full_stage(np.dtype(t), int(lead))
    return oc.builders()[name](np.dtype(dtype))


# ---------------------------------------------------------------- 8. every builder, every mode
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", CASES)
def test_cases(gexec, oracle, name, dtype):
    """banded(D): the ND = 8 / ND = 32 dispatch on both sides of D = 8, every multiple of 8 and its successor, 32 and
    33; mixed_segments; tall (absent slots clamped on both sides of x; the 300-row one is rejected by the share
    rule); 1 / 63 / 64 / 65 rows; the 50 % share from both sides.  What the plan reports comes from plan_model."""
    check_all_modes(gexec, oracle, built(name, dtype))


@pytest.mark.parametrize("name", oc.full_stage_names())
def test_full_stage(gexec, oracle, name):
    """64 rows x 32 entries = the stage's capacity, from every k0 % E: len = CAP .. CAP + E - 1 (the clamp and the
    NL-th load of a lane)"""
    m = built(name, None)
    a = check_all_modes(gexec, oracle, m, eligible=3)
    assert plan_info(a)["products"] == 6


# ---------------------------------------------------------------- 9. two segments per wave
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["mixed", "full", "banded-9", "rows-65"])
def test_two_segments_per_wave(gexec, oracle, name, dtype):
    """GKOC_TUNE_CSR_SEGS_PER_WAVE = 2 on small matrices, the modes without the dot: 8 (mixed), 3 (full stage,
    banded) and 2 segments, so the last wave owns two segments and owns one; in mixed_segments a wave's first
    segment has nothing to load while its second has"""
    if name == "full":
        m = oc.full_stage(np.dtype(dtype), 16 // np.dtype(dtype).itemsize - 1)
    else:
        m = built(name, dtype)
    with key(2, KEY_SEGS_PER_WAVE):
        check_all_modes(gexec, oracle, m, modes=("plain", "adv", "beta0"))


# ---------------------------------------------------------------- 10. rejected plans
@pytest.mark.parametrize("k,n", [s for s in oc.SHARES if s != (2, 4)])
def test_rejected_plans(gexec, oracle, k, n):
    dtype = np.dtype(np.float64)
    m = oc.share(k, n, dtype)
    shape, rp, ci, v = m
    rng = np.random.default_rng(12)
    b, c0 = rng.uniform(-1, 1, shape[1]).astype(dtype), rng.uniform(-1, 1, shape[0]).astype(dtype)
    a = arena_csr(gexec, *m)
    with key(1):
        for mode in ("plain", "adv"):                       # four products
            got = run(gexec, a, b, mode, c0)
            assert np.array_equal(bits(got), bits(reference(oracle, m, b, mode, c0))), mode
        info = plan_info(a)
        assert (info["state"], info["bytes"], info["products"]) == (2, 0, 0), info
        assert (info["eligible"], info["segments"]) == (k, n), info
        a.structure_changed()
        assert plan_info(a)["state"] == -1
        got = plain(gexec, a, b)                            # two products: analysed again, rejected again
        assert np.array_equal(bits(got), bits(reference(oracle, m, b, "plain", c0)))
        info = plan_info(a)
        assert (info["state"], info["bytes"], info["products"], info["eligible"]) == (2, 0, 0, k), info


def test_half_of_the_segments_is_enough(gexec, oracle):
    a = check_all_modes(gexec, oracle, oc.share(2, 4), modes=("plain", "adv", "beta0"))
    info = plan_info(a)
    assert (info["state"], info["eligible"], info["segments"], info["products"]) == (1, 2, 4, 6), info


# ---------------------------------------------------------------- 11. hub rows beside the plan
def hub_case(dtype):
    shape, rp, ci, v = oc.hub(np.dtype(dtype))
    m = sc.Mat(rp, ci, v, np.diff(rp), shape)
    rng = np.random.default_rng(21)
    b = rng.uniform(-1, 1, shape[1]).astype(dtype)
    c0 = rng.uniform(-1, 1, shape[0]).astype(dtype)
    return m, b, c0


def hub_product(ex, oracle, a, m, b, c0, mode):
    """one mode, twice; rows of at most GKOC_CSR_LONG_ROW entries bit-equal to the oracle, row 70 within D eps S
    (csr_spmv_cases.judge); plain and beta = 0 start from NaN in every row, row 70 and its segment included"""
    got = run(ex, a, b, mode, c0)
    if mode == "plain":
        ref = sc.reference(oracle, m, b)
    else:
        beta = 1.5 if mode == "adv" else 0.0
        ref = sc.reference(oracle, m, b, -0.75, beta, c0 if mode == "adv" else np.zeros_like(c0))
    assert list(ref.hubs) == [oc.HUB_ROW]
    sc.judge(got, ref, m)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_hub_rows_plan_used_then_long_rows_off(gexec, oracle, dtype):
    """built and multiplied with the long-row path at its default: three kernels write disjoint rows of c, the
    plan's skip bits hold the long flags (with_long).  Then GKOC_TUNE_CSR_LONG_ROWS = 0: the flags the plan was
    built with are not the product's, the plan is not used and its counter stands still."""
    m, b, c0 = hub_case(dtype)
    a = arena_csr(gexec, m.shape, m.rp, m.ci, m.v)
    with key(1):
        done = 0
        for mode in ("plain", "adv", "beta0"):
            hub_product(gexec, oracle, a, m, b, c0, mode)
            done += 2
            info = plan_info(a)
            assert (info["state"], info["eligible"], info["segments"], info["products"]) == (1, 3, 4, done), info
        with key(0, KEY_LONG_ROWS):
            for mode in ("plain", "adv", "beta0"):
                hub_product(gexec, oracle, a, m, b, c0, mode)
                info = plan_info(a)
                assert (info["state"], info["products"]) == (1, done), info
        hub_product(gexec, oracle, a, m, b, c0, "adv")       # and used again with the flags back
        assert plan_info(a)["products"] == done + 2


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_hub_rows_plan_built_without_long_rows(gexec, oracle, dtype):
    """built under GKOC_TUNE_CSR_LONG_ROWS = 0 (skip bits without long flags), then the key at its default: the
    long-flagged segment would be multiplied twice or not at all, so the plan is not used"""
    m, b, c0 = hub_case(dtype)
    a = arena_csr(gexec, m.shape, m.rp, m.ci, m.v)
    with key(1):
        with key(0, KEY_LONG_ROWS):
            hub_product(gexec, oracle, a, m, b, c0, "adv")
            info = plan_info(a)
            assert (info["state"], info["eligible"], info["products"]) == (1, 3, 2), info
        for mode in ("plain", "adv", "beta0"):
            hub_product(gexec, oracle, a, m, b, c0, mode)
            info = plan_info(a)
            assert (info["state"], info["products"]) == (1, 2), info


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_hub_rows_fused_dot(gexec, oracle, dtype):
    """gkoc_x_csr_spmv_dot on a (square) matrix with a hub row: the product goes through the plan and the
    long-row kernels, the dot is a pass of its own with the bits of Dense.compute_dot(b, c)"""
    import ginkgo_amd as g
    dtype = np.dtype(dtype)
    (n, _), rp, ci, v = oc.hub(dtype, square=True)
    m = sc.Mat(rp, ci, v, np.diff(rp), (n, n))
    model = oc.plan_model(rp, ci)
    assert (model.eligible, model.state) == (model.segments - 1, 1)
    b = np.random.default_rng(22).uniform(-1, 1, n).astype(dtype)
    a = arena_csr(gexec, (n, n), rp, ci, v)
    with key(1):
        got = run(gexec, a, b, "dot", None)
        info = plan_info(a)
    assert (info["state"], info["eligible"], info["products"]) == (1, model.eligible, 2), info
    ref = sc.reference(oracle, m, b)
    sc.judge(got[:n], ref, m)
    db, dc = g.Dense.from_numpy(gexec, b.reshape(-1, 1)), g.Dense.from_numpy(gexec, got[:n].reshape(-1, 1))
    dot = g.Dense.from_numpy(gexec, np.full((1, 1), np.nan, dtype))
    db.compute_dot(dc, dot)
    assert np.array_equal(bits(got[n:]), bits(dot.to_numpy().reshape(-1)))


# ---------------------------------------------------------------- 12. values are read live
def test_values_are_read_live(gexec, oracle):
    from ginkgo_amd import _lib
    dtype = np.dtype(np.float64)
    m = oc.mixed_segments(dtype)
    shape, rp, ci, v = m
    rng = np.random.default_rng(13)
    b = rng.uniform(-1, 1, shape[1]).astype(dtype)
    a = arena_csr(gexec, *m)
    with key(1):
        assert np.array_equal(bits(plain(gexec, a, b)), bits(oracle.csr_spmv(rp, ci, v, b)))
        done = 2
        for how in ("memcpy_h2d", "memset", "copy_"):
            new = rng.uniform(-2, 2, len(v)).astype(dtype)
            gexec.synchronize()
            if how == "memcpy_h2d":
                _lib.call("gkoc_memcpy_h2d", C.c_void_p(a.values.data_ptr()), new.ctypes.data_as(C.c_void_p),
                          C.c_size_t(new.nbytes), gexec.stream)
            elif how == "memset":
                new = np.zeros_like(new)
                _lib.call("gkoc_memset", C.c_void_p(a.values.data_ptr()), C.c_int(0), C.c_size_t(new.nbytes),
                          gexec.stream)
            else:
                a.values.copy_(torch.from_numpy(new))
            gexec.synchronize()
            assert plan_info(a)["state"] == 1, how
            got = plain(gexec, a, b)
            done += 2
            assert np.array_equal(bits(got), bits(oracle.csr_spmv(rp, ci, new, b))), how
            info = plan_info(a)
            assert (info["state"], info["products"]) == (1, done), (how, info)


def test_one_structure_several_value_arrays(gexec, oracle):
    """two Csr objects over the SAME row_ptrs / col_idxs tensors with value arrays of their own: one plan, both
    right.  A third whose values start one element into an arena allocation (not 16-byte aligned): the
    row-segment kernel multiplies it, and the plan's counter does not move."""
    import ginkgo_amd as g
    from ginkgo_amd.executor import MEM_VALUES
    dtype = np.dtype(np.float64)
    m = oc.mixed_segments(dtype)
    shape, rp, ci, v = m
    rng = np.random.default_rng(14)
    b = rng.uniform(-1, 1, shape[1]).astype(dtype)
    v2, v3 = rng.uniform(-2, 2, len(v)).astype(dtype), rng.uniform(-2, 2, len(v)).astype(dtype)
    a1 = arena_csr(gexec, *m)
    a2 = g.Csr(gexec, shape, arena_tensor(gexec, v2, MEM_VALUES), a1.col_idxs, a1.row_ptrs)
    block = arena_tensor(gexec, np.concatenate(([0.0], v3)).astype(dtype), MEM_VALUES)
    a3 = g.Csr(gexec, shape, block[1:], a1.col_idxs, a1.row_ptrs)
    assert a3.values.data_ptr() % 16 != 0 and a1.values.data_ptr() % 16 == 0 and a2.values.data_ptr() % 16 == 0
    with key(1):
        done = 0
        for a, vals in ((a1, v), (a2, v2), (a1, v), (a2, v2)):
            assert np.array_equal(bits(plain(gexec, a, b)), bits(oracle.csr_spmv(rp, ci, vals, b)))
            done += 2
            info = plan_info(a)
            assert (info["state"], info["products"]) == (1, done), info
        assert np.array_equal(bits(plain(gexec, a3, b)), bits(oracle.csr_spmv(rp, ci, v3, b)))
        info = plan_info(a1)
        assert (info["state"], info["products"]) == (1, done), info


# ---------------------------------------------------------------- 13. eviction
def _arena_figures(ex):
    ex.synchronize()
    info = ex.arena_info()
    return info["num_allocations"], info["used_bytes"]


def test_eviction_at_the_cache_cap(gexec, oracle):
    """130 live matrices under key 18 = 1 in a cache of 128 plans (offsets_cache_cap): the OLDEST plans make
    room - at least the first two, more if plans of earlier tests are still alive, and always a prefix of the
    arrival order; a matrix whose plan was evicted is multiplied again, right, and has a plan again; every buffer
    of every plan goes back to the allocator (the graveyard is emptied by the release that follows)."""
    dtype = np.dtype(np.float64)
    n_mat = oc.CACHE_CAP + 2
    shape, rp, ci, v = oc.rows_n(65, dtype)
    b = np.random.default_rng(15).uniform(-1, 1, shape[1]).astype(dtype)

    def round_():
        mats = []
        with key(1):
            for i in range(n_mat):
                a = arena_csr(gexec, shape, rp, ci, v * (1 + i))
                assert np.array_equal(bits(plain(gexec, a, b)), bits(oracle.csr_spmv(rp, ci, v * (1 + i), b))), i
                assert plan_info(a)["state"] == 1
                mats.append(a)
            states = [plan_info(a)["state"] for a in mats]
            gone = states.count(-1)
            assert gone >= n_mat - oc.CACHE_CAP and states == [-1] * gone + [1] * (n_mat - gone), states
            for i in range(3):
                got = plain(gexec, mats[i], b)
                assert np.array_equal(bits(got), bits(oracle.csr_spmv(rp, ci, v * (1 + i), b))), i
                info = plan_info(mats[i])
                # (a NEW plan for each of the three: the plan of mats[2] left when mats[0] came back at the latest)
                assert info["state"] == 1 and info["products"] == 2, (i, info)
        return gone

    gone = round_()                       # the warm-up round: the allocator's chunks, the long-row cache's slots
    gc.collect()
    before = _arena_figures(gexec)
    assert round_() == gone
    gc.collect()
    assert _arena_figures(gexec) == before


# ---------------------------------------------------------------- 14. degenerate shapes
def test_no_columns_is_never_keyed(gexec, oracle):
    """n_cols = 0 (no entries; every pointer valid, so n_cols alone decides): the launcher does not key the
    arrays at all - state -1 after two products, and c = 0"""
    from ginkgo_amd import _lib
    from ginkgo_amd.executor import MEM_INDICES, MEM_VALUES, MEM_VECTOR
    dtype = np.dtype(np.float64)
    n = 70
    rp = arena_tensor(gexec, np.zeros(n + 1, np.int32), MEM_INDICES)
    ci = arena_tensor(gexec, np.zeros(4, np.int32), MEM_INDICES)
    v = arena_tensor(gexec, np.zeros(4, dtype), MEM_VALUES)
    x = arena_tensor(gexec, np.zeros(4, dtype), MEM_VECTOR)
    with key(1):
        for _ in range(2):
            y = arena_tensor(gexec, np.full(n, np.nan, dtype), MEM_VECTOR)
            _lib.call("gkoc_csr_spmv_f64_i32", gexec.stream, n, 0, rp, ci, v, x, 1, y, 1, 1)
            gexec.synchronize()
            assert np.array_equal(bits(y.cpu().numpy()), bits(np.zeros(n, dtype)))
        assert plan_info_at(rp.data_ptr(), ci.data_ptr())["state"] == -1


# ---------------------------------------------------------------- 15. fuzz
@pytest.mark.parametrize("seed", oc.FUZZ_SEEDS)
def test_fuzz(gexec, oracle, seed):
    """state, segments and the eligible count from plan_model; plain and advanced, double"""
    check_all_modes(gexec, oracle, oc.fuzz(seed), modes=("plain", "adv"))
