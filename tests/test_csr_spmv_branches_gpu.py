"""Every branch of the CSR SpMV launchers (csrc/csr_spmv.hip; what they remember about a matrix is kept by
csrc/csr_structure.hip) at the smallest size that selects it; the list of branches, the condition that selects each
and the test that reaches it are in docs/binding_kernel_tests.md, "CSR SpMV launcher branches".

Rows of at most GKOC_CSR_LONG_ROW = 4096 entries: bit-identical to the sequential oracle.  Longer rows, where a
kernel sums them in another order: |got - exact| <= D eps S against an np.longdouble sum, D = ceil(len / 64) + 80
(tests/csr_spmv_cases.py has the derivation), and for double one-column products also the statistical bound the
older tests use.  Every product is run twice and must give the same bits.  The largest |got - exact| / (eps S) of
every test is recorded with util.record_perf (and printed with `pytest -s`).
"""
import contextlib
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import csr_spmv_cases as cc
from util import record_perf

pytestmark = pytest.mark.gpu

KEY_XCD_MAP, KEY_LOAD_GROUPS, KEY_MULTI_CHUNK, KEY_LONG_ROWS, KEY_SEGS_PER_WAVE = 0, 2, 6, 12, 13
TORCH_T = {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32}


@contextlib.contextmanager
def tuned(*pairs):
    """gkoc_tune_set(key, value) for every pair; the values found are put back whatever happens"""
    from ginkgo_amd import _lib
    old = []
    try:
        for key, value in pairs:
            was = C.c_int64(0)
            _lib.call("gkoc_tune_get", C.c_int(key), C.byref(was))
            old.append((key, was.value))
            _lib.call("gkoc_tune_set", C.c_int(key), C.c_int64(value))
        yield
    finally:
        for key, value in reversed(old):
            _lib.call("gkoc_tune_set", C.c_int(key), C.c_int64(value))


@pytest.fixture
def ratios(request):
    seen = {}
    yield seen
    for case, ratio in seen.items():
        record_perf("csr_spmv_branches", test=request.node.name, case=case, ratio=ratio)
        print(f"\n[ratio] {request.node.name} {case}: {ratio:.3f}", end="")


def keep(ratios, case, ratio):
    ratios[case] = max(ratios.get(case, 0.0), ratio)


def _allocations(ex):
    """live allocations of the arena, with Python's dead objects collected and the device idle"""
    gc.collect()
    ex.synchronize()
    return ex.arena_info()["num_allocations"]


def csr_of(g, ex, m, unaligned=False):
    if not unaligned:
        return g.Csr.from_arrays(ex, m.shape, m.rp, m.ci, m.v)
    # one element in front: the arrays start 8 (4) bytes behind an aligned address - no vector loads
    vals = ex.to_device(np.concatenate((np.zeros(1, m.v.dtype), m.v)))[1:]
    cols = ex.to_device(np.concatenate((np.zeros(1, m.ci.dtype), m.ci)))[1:]
    return g.Csr(ex, m.shape, vals, cols, ex.to_device(m.rp))


def apply(g, ex, a, db, dc, alpha, beta):
    if alpha is None:
        a.apply(db, dc)
    else:
        a.apply(g.scalar(ex, alpha, dc.dtype), db, g.scalar(ex, beta, dc.dtype), dc)


def product(g, ex, a, b, c_init, alpha=None, beta=None, sb=None, sc=None):
    """c_init -> alpha A b + beta c (A b without alpha), twice from the same input: the same bits"""
    db = g.Dense.from_numpy(ex, b.reshape(len(b), -1), stride=sb)
    outs = []
    for _ in range(2):
        dc = g.Dense.from_numpy(ex, c_init.reshape(len(c_init), -1), stride=sc)
        apply(g, ex, a, db, dc, alpha, beta)
        outs.append(dc.to_numpy())
    assert np.array_equal(outs[0], outs[1]), "the same product twice: different bits"
    return outs[0]


def modes(c0):
    """(name, alpha, beta, c on entry, c of the statistical bound): plain over NaN, advanced, beta = 0 over NaN"""
    nan = np.full_like(c0, np.nan)
    return (("plain", None, None, nan, None), ("adv", -0.75, 1.5, c0, c0), ("beta0", -0.75, 0.0, nan, None))


def vectors(m, k, seed, dtype=None):
    rng = np.random.default_rng(seed)
    t = dtype or m.v.dtype
    return rng.uniform(-1, 1, (m.shape[1], k)).astype(t), rng.uniform(-1, 1, (m.shape[0], k)).astype(t)


def fused_dot(g, ex, a, b):
    """gkoc_x_csr_spmv_dot_* through Csr.apply_dot, twice (the same bits): c, the dot, and Dense.compute_dot of b
    with that c"""
    from ginkgo_amd import _lib
    n, dtype = a.size[0], b.dtype
    es = dtype.itemsize
    nbytes = _lib.lib().gkoc_x_workspace_bytes(C.c_int64(n), C.c_size_t(es))
    work = ex.alloc(((nbytes + es - 1) // es,), TORCH_T[dtype])
    db = g.Dense.from_numpy(ex, b.reshape(n, 1))
    outs = []
    for _ in range(2):
        dc = g.Dense.from_numpy(ex, np.full(n, np.nan, dtype))
        dot = g.Dense.from_numpy(ex, np.full((1, 1), np.nan, dtype))
        a.apply_dot(db, dc, dot, work)
        sep = db.compute_dot(dc, g.Dense.from_numpy(ex, np.full((1, 1), np.nan, dtype)))
        outs.append((dc.to_numpy(), dot.to_numpy()[0, 0], sep.to_numpy()[0, 0]))
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1], "the same call twice: different bits"
    return outs[0]


def assert_fused_dot(ratios, case, dot, b, c):
    """the fused kernel's own dot against the np.longdouble dot of b with the c it produced (the bound is derived
    in test_fused_dot_with_hub_rows)"""
    n = len(c)
    p = b.reshape(n).astype(np.longdouble) * c.reshape(n).astype(np.longdouble)
    scale, eps = np.abs(p).sum(), cc.eps_of(c.dtype)
    err = abs(np.longdouble(dot) - p.sum())
    keep(ratios, case, float(err / (eps * scale)))
    assert err <= (-(-n // 64) + 16) * eps * scale, (case, float(err / (eps * scale)))


# ---------------------------------------------------------------- a. long rows, two and more right-hand sides
@pytest.mark.parametrize("idx", [np.int32, np.int64])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_long_rows_two_columns(gexec, oracle, ratios, dtype, idx):
    """csr_spmv_multi_kernel's own wave-cooperative sum (two columns, aligned streams: launch_csr_pair - even
    strides load b as pairs, an odd ldb one by one) and the one-pass-per-column fallback of an unaligned view
    (launch_csr_single with nrhs = 2, <1,4>, the row-segment kernel's wave path); rows of 4097, 9000 and 5000
    entries, one of exactly 4096 that stays bit-exact"""
    import ginkgo_amd as g
    m = cc.case_a(dtype, idx)
    b, c0 = vectors(m, 2, 11)
    aligned, view = csr_of(g, gexec, m), csr_of(g, gexec, m, unaligned=True)
    for name, alpha, beta, c_init, _ in modes(c0):
        ref = cc.reference(oracle, m, b, alpha, beta, c_init)
        for a, route, strides in ((aligned, "pair", ((2, 2), (4, 6), (3, 2))), (view, "columns one by one", ((2, 2),))):
            for sb, sc in strides:
                got = product(g, gexec, a, b, c_init, alpha, beta, sb, sc)
                keep(ratios, f"{route} {name}", cc.judge(got, ref, m))


@pytest.mark.parametrize("idx", [np.int32, np.int64])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_long_rows_three_and_four_columns_keep_entry_order(gexec, oracle, dtype, idx):
    """the fragment kernels (launch_csr_columns) add the products of a row in entry order whatever its length:
    ALL rows, the hub rows of 4097, 9000 and 5000 entries included, are bit-identical to the sequential oracle"""
    import ginkgo_amd as g
    m = cc.case_a(dtype, idx)
    a = csr_of(g, gexec, m)
    for k in (3, 4):
        b, c0 = vectors(m, k, 12 + k)
        for name, alpha, beta, c_init, _ in modes(c0):
            ref = cc.reference(oracle, m, b, alpha, beta, c_init)
            got = product(g, gexec, a, b, c_init, alpha, beta)
            assert cc.judge(got, ref, m, bitwise=tuple(ref.hubs)) == 0.0, (k, name)
            assert np.array_equal(got, ref.seq)


# ---------------------------------------------------------------- b. mixed precision over the threshold
@pytest.mark.parametrize("idx", [np.int32, np.int64])
def test_mixed_precision_long_rows(gexec, oracle, ratios, idx):
    """launch_csr_mixed (float values, double vectors and arithmetic) on rows of 4097, 9000 and 5000 entries: one
    and three columns (the kernel walks the columns one after the other, so the hub rows of every column take the
    wave path), plain and advanced, vector loads and - an unaligned view - <1,4>; the reference is the double
    oracle on the widened values"""
    import ginkgo_amd as g
    m = cc.case_a(np.float32, idx)
    for a, route in ((csr_of(g, gexec, m), "vector loads"), (csr_of(g, gexec, m, unaligned=True), "unaligned")):
        assert a.dtype == torch.float32
        for k in (1, 3):
            b, c0 = vectors(m, k, 20 + k, np.float64)
            for name, alpha, beta, c_init, c_stat in modes(c0):
                ref = cc.reference(oracle, m, b, alpha, beta, c_init)
                got = product(g, gexec, a, b, c_init, alpha, beta)
                assert got.dtype == np.float64
                keep(ratios, f"{route} {k} col {name}", cc.judge(got, ref, m))
                cc.judge_statistical(got, ref, m, b, c_stat, advanced=alpha is not None)


# ---------------------------------------------------------------- c. the flagged-segment kernels
@pytest.mark.parametrize("idx", [np.int32, np.int64])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_flagged_segments_kernels(gexec, oracle, ratios, dtype, idx):
    """csr_flagged_segments_kernel + csr_long_rows_fold_kernel on create_submatrix column views (ldb = 3,
    ldc = 5): ten rows beyond 4096 in one segment - the first eight are cut into chunks (bound), the ninth and
    tenth go through the stage in rounds in entry order (bit-exact, like the 63 ordinary neighbours, a 4096-entry
    and a 170-entry row among them) -, one hub in a last segment of 20 rows; beta = 0 over NaN in c; the columns
    of c next to the view keep their bits"""
    import ginkgo_amd as g
    m = cc.case_c(dtype, idx)
    n, ncols = m.shape
    a = csr_of(g, gexec, m)
    b3, c5 = vectors(m, 3, 30)
    c5 = np.concatenate((c5, c5[:, :2] + 1), axis=1)
    b = np.ascontiguousarray(b3[:, 1])
    for name, alpha, beta, c_init, c_stat in modes(np.ascontiguousarray(c5[:, 2])):
        ref = cc.reference(oracle, m, b, alpha, beta, c_init)
        wide_in = c5.copy()
        wide_in[:, 2] = c_init
        outs = []
        for _ in range(2):
            db = g.Dense.from_numpy(gexec, b3, stride=3).create_submatrix((0, ncols), (1, 2))
            wide = g.Dense.from_numpy(gexec, wide_in, stride=5)
            dc = wide.create_submatrix((0, n), (2, 3))
            assert (db.ld, dc.ld) == (3, 5)
            apply(g, gexec, a, db, dc, alpha, beta)
            outs.append(wide.to_numpy())
        assert np.array_equal(outs[0], outs[1], equal_nan=True)
        assert np.array_equal(np.delete(outs[0], 2, axis=1), np.delete(c5, 2, axis=1))
        got = outs[0][:, 2]
        keep(ratios, name, cc.judge(got, ref, m, bitwise=cc.C_STAGED))
        if dtype == np.float64:
            cc.judge_statistical(got, ref, m, b, c_stat, advanced=alpha is not None)


# ---------------------------------------------------------------- d. the list cap
@pytest.mark.parametrize("n_seg", [cc.LONG_LIST_CAP + 1, cc.LONG_LIST_CAP])
def test_flagged_list_cap(gexec, oracle, ratios, n_seg):
    """one 4097-entry row in every one of n_seg segments.  4097 segments are one more than the list holds: the
    launcher leaves the matrix to the row-segment kernel alone - the same kernel as with key 12 = 0, the same
    bits.  4096 segments fill the list: the flagged path, within the bound."""
    import ginkgo_amd as g
    m = cc.case_d(n_seg)
    b, _ = vectors(m, 1, 40)
    nan = np.full(m.shape[0], np.nan, m.v.dtype)
    ref = cc.reference(oracle, m, b)
    a = csr_of(g, gexec, m)
    got = product(g, gexec, a, b, nan)
    keep(ratios, f"{n_seg} segments", cc.judge(got, ref, m))
    if n_seg > cc.LONG_LIST_CAP:
        with tuned((KEY_LONG_ROWS, 0)):
            plain = product(g, gexec, a, b, nan)
        assert np.array_equal(got, plain)


# ---------------------------------------------------------------- e. the launcher's per-matrix cache
def test_cache_stale_flags(gexec, oracle, ratios):
    """the cache is keyed by (device, row_ptrs, n_rows): one Csr over fixed allocations is rewritten in place to
    matrices whose hub rows sit elsewhere, so the flag set of the first product goes stale - hubs in flagged
    segments 0 and 3; none (flagged segments without a long row); hubs in the unflagged segments 1 and 4 (the
    row-segment kernel's wave path next to flagged segments of short rows); ten hubs in segment 0, still flagged
    (chunks for eight, the stage in rounds for two).  Every product is right for the CURRENT contents.  Then
    the arrays go away and a different matrix of the same n_rows comes through Csr.from_arrays - torch's
    allocator usually hands out the same address again (not asserted)."""
    import ginkgo_amd as g
    mats = [cc.case_e(i) for i in range(4)]
    cap = max(len(m.ci) for m in mats)
    dev = gexec.device
    rp_t = torch.zeros(cc.E_ROWS + 1, dtype=torch.int32, device=dev)
    ci_t = torch.zeros(cap, dtype=torch.int32, device=dev)
    v_t = torch.zeros(cap, dtype=torch.float64, device=dev)
    a = g.Csr(gexec, mats[0].shape, v_t, ci_t, rp_t)
    b, c0 = vectors(mats[0], 1, 50)
    for i, m in enumerate(mats):
        rp_t.copy_(torch.from_numpy(m.rp))
        ci_t[:len(m.ci)].copy_(torch.from_numpy(m.ci))
        v_t[:len(m.v)].copy_(torch.from_numpy(m.v))
        for name, alpha, beta, c_init, c_stat in modes(c0):
            ref = cc.reference(oracle, m, b, alpha, beta, c_init)
            got = product(g, gexec, a, b, c_init, alpha, beta)
            keep(ratios, f"rewrite {i + 1}", cc.judge(got, ref, m, bitwise=cc.E_STAGED if i == 3 else ()))
            cc.judge_statistical(got, ref, m, b, c_stat, advanced=alpha is not None)
    old = rp_t.data_ptr()
    del a, rp_t, ci_t, v_t
    m = cc.case_e(4)
    a = csr_of(g, gexec, m)
    record_perf("csr_spmv_branches", test="test_cache_stale_flags", address_reused=a.row_ptrs.data_ptr() == old)
    for name, alpha, beta, c_init, _ in modes(c0):
        ref = cc.reference(oracle, m, b, alpha, beta, c_init)
        keep(ratios, "next matrix", cc.judge(product(g, gexec, a, b, c_init, alpha, beta), ref, m))


def test_cache_eviction(gexec, oracle, ratios):
    """130 matrices with a hub row, all alive, are more than the 128 the cache holds: the oldest entries make
    room (their flags and chunk buffers are freed), and the first three matrices, multiplied again, are looked
    at again.  Every product is right.

    Release accounting: after 128 arrivals a cache of 128 holds only this test's matrices, and each of them owns
    the same three buffers (flags, list, the stream's chunk sums).  So every later arrival - first products number
    129 and 130, then the three matrices that are multiplied again - frees exactly what it takes: the arena's
    allocation count, taken after the product with its temporaries dropped, stays what it was after number 128."""
    import ginkgo_amd as g
    count = cc.LONG_CACHE_CAP + 2
    mats = [cc.case_evict(i) for i in range(count)]
    b, _ = vectors(mats[0], 1, 60)
    nan = np.full(mats[0].shape[0], np.nan)
    alive = [csr_of(g, gexec, m) for m in mats]
    assert len({a.row_ptrs.data_ptr() for a in alive}) == count
    full = None
    for nth, i in enumerate(list(range(count)) + [0, 1, 2]):
        ref = cc.reference(oracle, mats[i], b)
        keep(ratios, "all", cc.judge(product(g, gexec, alive[i], b, nan), ref, mats[i]))
        if nth + 1 == cc.LONG_CACHE_CAP:
            full = _allocations(gexec)
        elif nth + 1 > cc.LONG_CACHE_CAP:
            assert _allocations(gexec) == full, (nth + 1, i)


def test_cache_forgets_on_free(gexec, oracle, ratios):
    """row pointers from gkoc_malloc: gkoc_free drops the cache entry of the pointer (csr_long_rows_forget), so a
    new matrix in a new allocation - the arena usually hands out the same block - is looked at afresh.

    Release accounting: the entry's flags, list and chunk sums go with the pointer - the arena's allocation count
    after gkoc_free(p) is the one taken before gkoc_malloc of the round (after a warm-up round: what the library
    keeps per stream)."""
    import ginkgo_amd as g
    from ginkgo_amd import _lib
    n, ncols = 64 * 2 + 5, 6000
    b = np.random.default_rng(70).uniform(-1, 1, ncols)
    db = g.Dense.from_numpy(gexec, b)
    ptrs = []

    def products(m, p, ci_t, v_t):
        outs = []
        for _ in range(2):
            dc = g.Dense.from_numpy(gexec, np.full(n, np.nan))
            _lib.call("gkoc_csr_spmv_f64_i32", gexec.stream, n, ncols, p, ci_t, v_t, db.values, 1, dc.values, 1, 1)
            outs.append(dc.to_numpy())
        return outs

    def round_(seed, hubs, case):
        m = cc.hub_matrix(seed, n, ncols, hubs)
        ci_t, v_t = gexec.to_device(m.ci), gexec.to_device(m.v)
        before = _allocations(gexec)
        p = C.c_void_p()
        _lib.call("gkoc_malloc", C.byref(p), C.c_size_t(m.rp.nbytes))
        try:
            _lib.call("gkoc_memcpy_h2d", p, m.rp.ctypes.data_as(C.c_void_p), C.c_size_t(m.rp.nbytes), gexec.stream)
            ref = cc.reference(oracle, m, b)
            outs = products(m, p, ci_t, v_t)
            assert np.array_equal(outs[0], outs[1])
            if case:
                keep(ratios, case, cc.judge(outs[0], ref, m))
        finally:
            gexec.synchronize()
            _lib.call("gkoc_free", p)
        after = _allocations(gexec)
        assert case is None or after == before, (case, before, after)
        return p.value

    rounds = ((300, ((7, 5000),)), (301, ((64 + 9, 4097), (n - 1, 4500))))
    round_(*rounds[0], None)      # (warm-up)
    for seed, hubs in rounds:
        ptrs.append(round_(seed, hubs, f"matrix {len(ptrs) + 1}"))
    record_perf("csr_spmv_branches", test="test_cache_forgets_on_free", address_reused=ptrs[0] == ptrs[1])


CAPTURE_CASES = ["first seen in the capture", "multiplied before", "multiplied before on the capture stream"]


@pytest.mark.parametrize("before", CAPTURE_CASES)
def test_cache_stream_capture(gexec, oracle, ratios, before):
    """the one-column product captured with torch.cuda.graph and replayed twice, b rewritten in place between
    the replays.  A matrix first seen inside the capture cannot be scanned (the scan's answer needs a
    synchronisation) and one whose chunk buffer for the capturing stream does not exist yet cannot get one: both
    are multiplied by the row-segment kernel alone.  A matrix that the capturing stream has multiplied before
    takes the flagged kernels into the graph.  The matrix stays alive and cached while the graph is replayed
    (include/gko_cdna4.h, GKOC_TUNE_CSR_LONG_ROWS); afterwards an eager product is still right."""
    import ginkgo_amd as g
    m = cc.case_capture(CAPTURE_CASES.index(before))
    n, ncols = m.shape
    a = csr_of(g, gexec, m)
    rng = np.random.default_rng(80)
    bs = [rng.uniform(-1, 1, ncols) for _ in range(3)]
    refs = [cc.reference(oracle, m, b) for b in bs]
    db = g.Dense.from_numpy(gexec, bs[0])
    dy = g.Dense.from_numpy(gexec, np.full(n, np.nan))
    side = torch.cuda.Stream(device=gexec.device)
    if before == "multiplied before":
        a.apply(db, dy)
    elif before == "multiplied before on the capture stream":
        side.wait_stream(torch.cuda.current_stream(gexec.device))
        with torch.cuda.stream(side):
            a.apply(db, dy)
    torch.cuda.synchronize()
    dy.fill(np.nan)
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream(gexec.device))
    with torch.cuda.graph(graph, stream=side):
        a.apply(db, dy)
    torch.cuda.current_stream(gexec.device).wait_stream(side)
    for b, ref in zip(bs[:2], refs[:2]):
        db.values.copy_(torch.from_numpy(b.reshape(-1, 1)))
        dy.fill(np.nan)
        graph.replay()
        torch.cuda.synchronize()
        got = dy.to_numpy()
        keep(ratios, "replay", cc.judge(got, ref, m))
        cc.judge_statistical(got, ref, m, b)
    got = product(g, gexec, a, bs[2], np.full(n, np.nan))
    keep(ratios, "eager afterwards", cc.judge(got, refs[2], m))
    del graph


# ---------------------------------------------------------------- f. the fused product and dot with hub rows
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fused_dot_with_hub_rows(gexec, oracle, ratios, dtype, aligned):
    """gkoc_x_csr_spmv_dot_* on a square matrix with hub rows.  Key 12 = 1 (default): launch_csr_dot multiplies
    through launch_csr - flagged kernels - and takes the dot as a pass of its own, so the dot has the bits of
    Dense.compute_dot(b, c).  Key 12 = 0: the fused kernel, whose wave path sums the hub rows and whose unaligned
    instantiation is <1,4>; its dot is formed by another tree (a partial sum per wave, then fold_partials) and is
    held to (ceil(n / 64) + 16) eps sum |b_i c_i| of the np.longdouble dot of the c it produced: one rounding for
    the product, at most two additions in a lane, six levels of wave_sum, and the fold of ceil(n / 64) wave sums
    has at most that many additions on its longest path whatever its tree."""
    import ginkgo_amd as g
    m = cc.case_f(dtype)
    a = csr_of(g, gexec, m, unaligned=not aligned)
    b, _ = vectors(m, 1, 90)
    ref = cc.reference(oracle, m, b)
    for key12 in (1, 0):
        with tuned((KEY_LONG_ROWS, key12)):
            c, dot, sep = fused_dot(g, gexec, a, b)
        keep(ratios, f"c key12={key12}", cc.judge(c, ref, m))
        if dtype == np.float64:
            cc.judge_statistical(c, ref, m, b)
        print(f"\n[dot] {dtype.__name__} aligned={aligned} key12={key12}: fused {dot!r} separate {sep!r}", end="")
        if key12 == 1:
            assert dot == sep
        else:
            assert_fused_dot(ratios, "dot key12=0", dot, b, c)


# ---------------------------------------------------------------- g. "Results never depend on them"
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_load_groups_key_changes_nothing(gexec, oracle, dtype):
    """GKOC_TUNE_CSR_LOAD_GROUPS (key 2) = 0, 1, 3, 4 - <EV,1> (the default at this size), <1,8>, <2,4> of
    launch_csr_single and both layouts of launch_csr_pair - on 700 rows with empty rows and a row of 700 entries:
    the bits of the default run, which are the oracle's"""
    import ginkgo_amd as g
    m = cc.hub_matrix(110, 700, 700, ((0, 0), (64, 0), (699, 0), (5, 700)), dtype, max_short=39)
    a = csr_of(g, gexec, m)
    for k in (1, 2):
        b, c0 = vectors(m, k, 111 + k)
        for name, alpha, beta, c_init, _ in modes(c0):
            default = product(g, gexec, a, b, c_init, alpha, beta)
            assert np.array_equal(default, cc.reference(oracle, m, b, alpha, beta, c_init).seq)
            for value in (0, 1, 3, 4):
                with tuned((KEY_LOAD_GROUPS, value)):
                    assert np.array_equal(product(g, gexec, a, b, c_init, alpha, beta), default), (k, name, value)


def test_multi_rhs_chunk_key_changes_nothing(gexec, oracle):
    """GKOC_TUNE_MULTI_XCD_CHUNK_ROWS (key 6) = 0, 64, 1024, 4096 at 2, 3 and 8 columns: 44 807 rows are more than
    one period (8 XCDs x 4096 rows) of the chunked workgroup order plus a tail that keeps the plain order"""
    import ginkgo_amd as g
    m = cc.banded_matrix(120, 64 * 700 + 7, 9)
    a = csr_of(g, gexec, m)
    for k in (2, 3, 8):
        b, c0 = vectors(m, k, 121 + k)
        for name, alpha, beta, c_init, _ in modes(c0)[:2]:
            default = product(g, gexec, a, b, c_init, alpha, beta)
            assert np.array_equal(default, cc.reference(oracle, m, b, alpha, beta, c_init).seq)
            for value in (0, 64, 1024, 4096):
                with tuned((KEY_MULTI_CHUNK, value)):
                    assert np.array_equal(product(g, gexec, a, b, c_init, alpha, beta), default), (k, name, value)


@pytest.mark.parametrize("per_row", [60, 39])
def test_float_rows_of_forty_and_more_take_one_entry_per_lane(gexec, oracle, per_row):
    """float values and at least 40 entries per row on average: the launcher picks <1,8> by itself (the count
    comes with the first product's look at the row pointers); 39 per row stay with <EV,1>.  Either way the
    oracle's bits, plain and advanced."""
    import ginkgo_amd as g
    m = cc.hub_matrix(130 + per_row, 300, 300, tuple((r, per_row) for r in range(300)), np.float32)
    assert (len(m.ci) >= 40 * 300) == (per_row == 60)
    a = csr_of(g, gexec, m)
    b, c0 = vectors(m, 1, 131)
    for name, alpha, beta, c_init, _ in modes(c0):
        got = product(g, gexec, a, b, c_init, alpha, beta)
        assert np.array_equal(got, cc.reference(oracle, m, b, alpha, beta, c_init).seq), name


# ---------------------------------------------------------------- h. the size rules
def test_size_rules_two_million_rows(gexec, oracle):
    """32 768 segments and five rows more: the launcher's own rule picks <PE,PU>; key 0 = 1 adds the
    XCD-contiguous wave order (at least 8192 waves); key 13 = 2 with key 0 = 1 walks two segments per wave in
    that order (16 385 waves).  All three have the oracle's bits."""
    import ginkgo_amd as g
    m = cc.banded_matrix(140, 64 * 32768 + 5, 5)
    a = csr_of(g, gexec, m)
    b, _ = vectors(m, 1, 141)
    nan = np.full(m.shape[0], np.nan)
    want = oracle.csr_spmv(m.rp, m.ci, m.v, b[:, 0].copy())
    for pairs in ((), ((KEY_XCD_MAP, 1),), ((KEY_SEGS_PER_WAVE, 2), (KEY_XCD_MAP, 1))):
        with tuned(*pairs):
            assert np.array_equal(product(g, gexec, a, b, nan)[:, 0], want), pairs


def test_automatic_xcd_map_with_hub_rows(gexec, oracle, ratios):
    """8192 segments and two hub rows, default keys: flagged segments and at least 8192 waves switch the
    XCD-contiguous wave order on by themselves"""
    import ginkgo_amd as g
    m = cc.case_h_auto()
    a = csr_of(g, gexec, m)
    b, c0 = vectors(m, 1, 150)
    for name, alpha, beta, c_init, c_stat in modes(c0):
        ref = cc.reference(oracle, m, b, alpha, beta, c_init)
        got = product(g, gexec, a, b, c_init, alpha, beta)
        keep(ratios, name, cc.judge(got, ref, m))
        cc.judge_statistical(got, ref, m, b, c_stat, advanced=alpha is not None)
        # key 0 = 2 ("never") only changes which wave takes which segment: the same bits
        with tuned((KEY_XCD_MAP, 2)):
            assert np.array_equal(product(g, gexec, a, b, c_init, alpha, beta), got), name
    # the fused product and dot reads key 0 as well (XCD order only with key 0 = 1 and 8192 waves)
    ref = cc.reference(oracle, m, b)
    with tuned((KEY_LONG_ROWS, 0), (KEY_XCD_MAP, 1)):
        c, dot, _ = fused_dot(g, gexec, a, b)
    keep(ratios, "fused dot, key 0 = 1", cc.judge(c, ref, m))
    with tuned((KEY_LONG_ROWS, 0)):
        c1, dot1, _ = fused_dot(g, gexec, a, b)
    assert np.array_equal(c, c1)
    assert_fused_dot(ratios, "dot, key 0 = 1", dot, b, c)
    assert_fused_dot(ratios, "dot, key 0 = 0", dot1, b, c1)


# ---------------------------------------------------------------- i. 64-bit offsets into b
@pytest.mark.parametrize("nrhs", [3, 4, 8])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fragment_kernels_64_bit_offsets(gexec, oracle, dtype, nrhs):
    """the fragment kernels index b with 64 bits when n_cols * ldb >= 2^32.  They never receive n_cols, so the
    C ABI reaches that instantiation with a small matrix: n_cols declared as 2^30 with ldb = 4 (8 for eight
    columns), b allocated for the 1200 columns that are stored.  The same call with n_cols one lower (32-bit
    offsets for ldb = 4) and with the true n_cols = 1200 (32-bit offsets also for ldb = 8): all equal to the
    oracle.  645 rows, an empty row, a row of 600 entries (past the staging capacity of a wave)."""
    import ginkgo_amd as g
    from ginkgo_amd import _lib
    n, ncols = 16 * 40 + 5, 1200
    m = cc.hub_matrix(160, n, ncols, ((0, 0), (1, 600), (n - 2, 0)), dtype, max_short=39)
    b, c0 = vectors(m, nrhs, 161 + nrhs)
    a = csr_of(g, gexec, m)
    suf = "f64_i32" if dtype == np.float64 else "f32_i32"
    alpha, beta = g.scalar(gexec, -0.75, TORCH_T[np.dtype(dtype)]), g.scalar(gexec, 1.5, TORCH_T[np.dtype(dtype)])
    want = oracle.csr_spmv(m.rp, m.ci, m.v, b)
    want_adv = oracle.csr_spmv(m.rp, m.ci, m.v, b, alpha=-0.75, beta=1.5, c=c0)
    # eight columns with an odd ldb = 9: the one-column-per-lane kernel of rounds 3-4 (csr_spmv_frag_kernel),
    # 64-bit offsets from n_cols = ceil(2^32 / 9) on
    cases = [(8 if nrhs == 8 else 4, 1 << 30)] + ([(9, -(-(1 << 32) // 9))] if nrhs == 8 else [])
    for ldb, big in cases:
        assert big * ldb >= 1 << 32 and ((big - 1) * ldb < 1 << 32 or ldb == 8)
        db = g.Dense.from_numpy(gexec, b, stride=ldb)
        for declared in (big, big - 1, ncols):
            dc = g.Dense.from_numpy(gexec, np.full_like(c0, np.nan))
            _lib.call("gkoc_csr_spmv_" + suf, gexec.stream, n, declared, a.row_ptrs, a.col_idxs, a.values, db.values,
                      ldb, dc.values, nrhs, nrhs)
            assert np.array_equal(dc.to_numpy(), want), (ldb, declared)
            dc = g.Dense.from_numpy(gexec, c0)
            _lib.call("gkoc_csr_advanced_spmv_" + suf, gexec.stream, n, declared, alpha.values, a.row_ptrs, a.col_idxs,
                      a.values, db.values, ldb, beta.values, dc.values, nrhs, nrhs)
            assert np.array_equal(dc.to_numpy(), want_adv), (ldb, declared)
