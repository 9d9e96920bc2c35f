"""The cached column-offset plan of the CSR SpMV (csrc/csr_offsets.hpp, launcher in csrc/csr_spmv.hip).

Index arrays come from the library's allocator even when tiny (only those ever get a plan).  Every product is
compared BIT FOR BIT (NaN positions included) with the sequential oracle and with the same product under
GKOC_TUNE_CSR_OFFSETS = 2 (the row-segment kernel alone), runs twice with the same bits, and the plan's own
counters (gkoc_csr_plan_info) must show that the offsets kernel did the work: the fallback cannot pass alone.
"""
import contextlib
import ctypes as C
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KEY = 18          # GKOC_TUNE_CSR_OFFSETS
TORCH_T = {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32}
BITS = {np.dtype(np.float64): np.uint64, np.dtype(np.float32): np.uint32}


@contextlib.contextmanager
def key(value):
    from ginkgo_amd import _lib
    was = C.c_int64(0)
    _lib.call("gkoc_tune_get", C.c_int(KEY), C.byref(was))
    _lib.call("gkoc_tune_set", C.c_int(KEY), C.c_int64(value))
    try:
        yield
    finally:
        _lib.call("gkoc_tune_set", C.c_int(KEY), C.c_int64(was.value))


def arena_tensor(ex, arr, role):
    """a tensor over a gkoc_malloc_role allocation of its own, whatever its size (executor._ArenaBlock)"""
    from ginkgo_amd.executor import _ArenaBlock, _TYPESTR
    arr = np.ascontiguousarray(arr)
    src = torch.from_numpy(arr)
    with torch.cuda.device(ex.device):
        block = _ArenaBlock(arr.nbytes, role, arr.shape, _TYPESTR[src.dtype])
        t = torch.as_tensor(block, device=ex.device)
    assert t.data_ptr() == block.ptr
    t.copy_(src)
    return t


def arena_csr(ex, shape, rp, ci, v):
    import ginkgo_amd as g
    from ginkgo_amd.executor import MEM_INDICES, MEM_VALUES
    return g.Csr(ex, shape, arena_tensor(ex, v, MEM_VALUES), arena_tensor(ex, ci.astype(np.int32), MEM_INDICES),
                 arena_tensor(ex, rp.astype(np.int32), MEM_INDICES))


def plan_info(a):
    return plan_info_at(a.row_ptrs.data_ptr(), a.col_idxs.data_ptr())


def plan_info_at(row_ptrs, col_idxs):
    from ginkgo_amd import _lib
    st, el, ns, by, pr = C.c_int(-9), C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
    _lib.call("gkoc_csr_plan_info", C.c_void_p(row_ptrs), C.c_void_p(col_idxs),
              C.byref(st), C.byref(el), C.byref(ns), C.byref(by), C.byref(pr))
    return {"state": st.value, "eligible": el.value, "segments": ns.value, "bytes": by.value, "products": pr.value}


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(BITS[x.dtype])


# ---------------------------------------------------------------- matrices (host, int32)
def from_rows(rows, n_cols, dtype, seed=0):
    """rows: list of column lists in STORAGE order; values uniform in +-[0.5, 1.5)"""
    rp = np.zeros(len(rows) + 1, np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.array([c for r in rows for c in r], np.int32)
    rng = np.random.default_rng(seed)
    v = (rng.uniform(0.5, 1.5, len(ci)) * rng.choice([-1.0, 1.0], len(ci))).astype(dtype)
    return (len(rows), n_cols), rp, ci, v


def band_rows(n, n_cols, offsets):
    return [[r + o for o in offsets if 0 <= r + o < n_cols] for r in range(n)]


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


# ---------------------------------------------------------------- products
def run(ex, a, b, mode, c0):
    """one product, twice from the same input (the same bits): the result"""
    import ginkgo_amd as g
    n, dtype = a.size[0], b.dtype
    db = g.Dense.from_numpy(ex, b.reshape(-1, 1))
    outs = []
    for _ in range(2):
        if mode == "dot":
            from ginkgo_amd import _lib
            es = dtype.itemsize
            nbytes = _lib.lib().gkoc_x_workspace_bytes(C.c_int64(n), C.c_size_t(es))
            work = ex.alloc(((nbytes + es - 1) // es,), TORCH_T[dtype])
            dc = g.Dense.from_numpy(ex, np.full((n, 1), np.nan, dtype))
            dot = g.Dense.from_numpy(ex, np.full((1, 1), np.nan, dtype))
            a.apply_dot(db, dc, dot, work)
            outs.append(np.concatenate((dc.to_numpy().reshape(-1), dot.to_numpy().reshape(-1))))
            continue
        c_init = np.full((n, 1), np.nan, dtype) if mode in ("plain", "beta0") else c0.reshape(-1, 1)
        dc = g.Dense.from_numpy(ex, c_init)
        if mode == "plain":
            a.apply(db, dc)
        else:
            alpha, beta = (-0.75, 1.5) if mode == "adv" else (-0.75, 0.0)
            a.apply(g.scalar(ex, alpha, dc.dtype), db, g.scalar(ex, beta, dc.dtype), dc)
        outs.append(dc.to_numpy().reshape(-1))
    assert np.array_equal(bits(outs[0]), bits(outs[1])), "the same product twice: different bits"
    return outs[0]


def reference(oracle, m, b, mode, c0):
    _, rp, ci, v = m
    if mode in ("plain", "dot"):
        return oracle.csr_spmv(rp, ci, v, b)
    alpha, beta = (-0.75, 1.5) if mode == "adv" else (-0.75, 0.0)
    c = c0 if mode == "adv" else np.zeros_like(c0)      # beta = 0 never reads c
    return oracle.csr_spmv(rp, ci, v, b, alpha, beta, c)


def check_all_modes(ex, oracle, m, eligible, modes=("plain", "adv", "beta0", "dot"), b=None):
    """every mode through the plan (built by the first product: key 1), against the oracle and against key 2"""
    shape, rp, ci, v = m
    rng = np.random.default_rng(5)
    if b is None:
        b = rng.uniform(-1, 1, shape[1]).astype(v.dtype)
    c0 = rng.uniform(-1, 1, shape[0]).astype(v.dtype)
    a = arena_csr(ex, shape, rp, ci, v)
    n_seg = -(-shape[0] // 64)
    done = 0
    for mode in modes:
        if mode == "dot" and (shape[0] != shape[1] or eligible != n_seg):
            continue        # (square matrices; the fused entry takes the plan where every segment is eligible)
        with key(1):
            got = run(ex, a, b, mode, c0)
            info = plan_info(a)
        done += 2
        assert info["state"] == 1 and info["segments"] == n_seg and info["eligible"] == eligible, (mode, info)
        assert info["products"] == done, (mode, info)
        with key(2):
            old = run(ex, a, b, mode, c0)
        assert plan_info(a)["products"] == done
        assert np.array_equal(bits(got), bits(old)), mode
        ref = reference(oracle, m, b, mode, c0)
        assert np.array_equal(bits(got[:shape[0]]), bits(ref)), mode
    return a


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
def two_structures(dtype):
    """the same row pointers and entry count, other columns"""
    n = 130
    first = band_rows(n, n + 8, (-1, 0, 1))
    second = [[c + 2 if c > r else c for c in row] for r, row in enumerate(first)]
    return from_rows(first, n + 8, dtype, seed=1), from_rows(second, n + 8, dtype, seed=1)


def plain(ex, a, b):
    return run(ex, a, b, "plain", None)


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
