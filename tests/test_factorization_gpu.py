"""ILU(0) / IC(0) on the device (factorization.Ilu / Ic, the Ilu / Ic preconditioners) against the numpy
loops of tests/factorization_refs.py and tests/trs_refs.py.  Results are compared with np.array_equal: the
kernels promise the reference's rounding."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import ginkgo_amd as g
import factorization_refs as fr
import trs_refs as tr

pytestmark = pytest.mark.gpu

TYPES = [(np.float64, np.int32), (np.float64, np.int64), (np.float32, np.int32), (np.float32, np.int64)]
TYPE_IDS = ["f64-i32", "f64-i64", "f32-i32", "f32-i64"]
KINDS = ["ilu", "ic"]


# ------------------------------------------------------------------ helpers
def csr_arrays(m):
    return [t.cpu().numpy() for t in (m.row_ptrs, m.col_idxs, m.values)]


def device_csr(gexec, rp, ci, v):
    n = len(rp) - 1
    return g.Csr.from_arrays(gexec, (n, n), rp, ci, v)


def generate(gexec, kind, a, **params):
    f = (g.factorization.Ilu if kind == "ilu" else g.factorization.Ic).build()
    for k, val in params.items():
        f = getattr(f, "with_" + k)(val)
    return f.on(gexec).generate(a)


def factors_of(kind, fact):
    """the arrays of L and U (ilu) or of L (ic)"""
    if kind == "ilu":
        return csr_arrays(fact.get_l_factor()) + csr_arrays(fact.get_u_factor())
    return csr_arrays(fact.get_l_factor())


def reference(kind, rp, ci, v):
    return fr.ilu_factors(rp, ci, v) if kind == "ilu" else fr.ic_factor(rp, ci, v)


def same(got, want, itype, equal_nan=False):
    """index arrays of the reference are kept in int32 and shared by the index types"""
    assert len(got) == len(want)
    for p, q in zip(got, want):
        q = q.astype(itype) if q.dtype.kind == "i" else q
        assert p.dtype == q.dtype and p.shape == q.shape
        assert np.array_equal(p, q, equal_nan=equal_nan and q.dtype.kind == "f")


@functools.lru_cache(maxsize=None)
def wide_threshold(gexec):
    rp, ci, v = tr.from_rows([[(0, 1.0)]])
    return g.LowerTrs.build().on(gexec).generate(device_csr(gexec, rp, ci, v)).wide_threshold


@functools.lru_cache(maxsize=None)
def case_matrix(name, spd, w=None):
    """scipy matrices of the cases: symmetric patterns, strictly diagonally dominant values (symmetric with
    spd, independent in the two triangles without)"""
    rng = np.random.default_rng(len(name) * 11 + 3)
    if name == "one":
        return sp.csr_matrix(np.array([[2.0]]))
    if name == "diagonal":
        return sp.diags(rng.uniform(1, 2, 300)).tocsr()
    if name == "chain":
        return fr.from_lower_pattern(fr.chain_pattern(2500), rng, spd)
    if name == "tiers":
        return fr.from_lower_pattern(fr.tiers_pattern(w, rng), rng, spd)
    if name == "stencil":
        return fr.stencil27(12)
    if name == "random":
        return fr.from_lower_pattern(fr.random_pattern(4000, rng), rng, spd)
    if name == "small":
        return fr.from_lower_pattern(fr.random_pattern(300, rng, 3), rng, spd)
    raise KeyError(name)


_REFS = {}      # reference factors, computed once per (case, kind, value type) and left unchanged


def check_case(gexec, kind, name, a, dtype, itype):
    rp, ci, v = fr.arrays(a, itype, dtype)
    dev = device_csr(gexec, rp, ci, v)
    fact = generate(gexec, kind, dev)
    for got, kept in zip(csr_arrays(dev), (rp, ci, v)):
        assert np.array_equal(got, kept), "generate changed the caller's matrix"
    key = (name, kind, dtype)
    if key not in _REFS:
        _REFS[key] = reference(kind, *fr.arrays(a, np.int32, dtype))
        for arr in _REFS[key]:
            arr.setflags(write=False)
    ref = _REFS[key]
    assert all(np.isfinite(x).all() for x in ref)
    same(factors_of(kind, fact), ref, itype)
    return fact


# ------------------------------------------------------------------ factors, bit for bit
@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("name", ["one", "diagonal", "chain", "stencil", "random"])
@pytest.mark.parametrize("kind", KINDS)
def test_factors_match_reference(gexec, kind, name, dtype, itype):
    fact = check_case(gexec, kind, name, case_matrix(name, kind == "ic"), dtype, itype)
    levels = {"one": 1, "diagonal": 1, "chain": 2500, "stencil": 78}.get(name)
    if levels:
        schedule = g.LowerTrs.build().on(gexec).generate(fact.get_l_factor())
        assert schedule.num_levels == levels
        if name != "stencil":
            assert schedule.num_launches == 1


@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_tiers_wide_wide_narrow(gexec, kind, dtype, itype):
    w = wide_threshold(gexec)
    a = case_matrix("tiers", kind == "ic", w)
    assert a.shape[0] < 13000
    fact = check_case(gexec, kind, "tiers", a, dtype, itype)
    schedule = g.LowerTrs.build().on(gexec).generate(fact.get_l_factor())
    assert schedule.num_levels == 42 and schedule.num_launches == 3


def boundary_lengths():
    limits = g.factorization.row_limits()
    assert 1 <= len(limits) <= 4 and limits == sorted(set(limits)) and limits[0] >= 8
    # the first and the last length of every path, and a row that is streamed in several rounds
    return sorted({x for limit in limits for x in (limit, limit + 1)} | {300, 5 * limits[-1] - 20})


@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_hub_rows_at_every_path_boundary(gexec, kind, dtype, itype):
    """the kernels pick their path from the LONGEST row, so every length gets a matrix of its own in
    which one hub row has exactly that many entries (ic: in its lower triangle) and no other more than 4"""
    for length in boundary_lengths():
        if kind == "ilu":
            n_lower = (length - 1) // 2
            n_upper = length - 1 - n_lower
        else:
            n_lower, n_upper = length - 1, 2
        n, hub = n_lower + n_upper + 60, n_lower + 20
        rng = np.random.default_rng(length)
        a = fr.from_lower_pattern(fr.hub_pattern(n, hub, n_lower, n_upper), rng, kind == "ic")
        stored = np.diff((sp.tril(a, format="csr") if kind == "ic" else a).indptr)
        assert stored.max() == stored[hub] == length and np.sort(stored)[-2] <= 4
        check_case(gexec, kind, "hub%d" % length, a, dtype, itype)


@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("name", ["chain", "blocks"])
def test_planted_factors(gexec, name, dtype, itype):
    """dyadic entries, A = L U (A = L L^T) exactly: the factors come back exactly, whatever the reference says"""
    rng = np.random.default_rng(21)
    a, lo, up = fr.planted_chain(600, rng) if name == "chain" else fr.planted_blocks(60, rng)
    rp, ci, v = fr.on_pattern(a, (lo != 0) | (up != 0), itype, dtype)
    fact = generate(gexec, "ilu", device_csr(gexec, rp, ci, v))
    assert np.array_equal(fr.dense_of(*csr_arrays(fact.get_l_factor())), lo.astype(dtype))
    assert np.array_equal(fr.dense_of(*csr_arrays(fact.get_u_factor())), up.astype(dtype))
    spd, low = fr.planted_cholesky(lo)
    rp, ci, v = fr.on_pattern(spd, (low != 0) | (low != 0).T, itype, dtype)
    fact = generate(gexec, "ic", device_csr(gexec, rp, ci, v))
    assert np.array_equal(fr.dense_of(*csr_arrays(fact.get_l_factor())), low.astype(dtype))
    assert np.array_equal(fr.dense_of(*csr_arrays(fact.get_lt_factor())), low.T.astype(dtype))


@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
def test_layout_of_the_factors(gexec, dtype, itype):
    a = case_matrix("small", True)
    n = a.shape[0]
    rp, ci, v = fr.arrays(a, itype, dtype)
    dev = device_csr(gexec, rp, ci, v)
    ilu = generate(gexec, "ilu", dev)
    l_rp, l_ci, l_v, u_rp, u_ci, u_v = factors_of("ilu", ilu)
    assert np.array_equal(l_ci[l_rp[1:] - 1], np.arange(n)) and (l_v[l_rp[1:] - 1] == 1).all()
    assert np.array_equal(u_ci[u_rp[:-1]], np.arange(n))
    assert ilu.get_l_factor().size == ilu.get_u_factor().size == (n, n) and ilu.get_size() == (n, n)
    # Ic: L^T is the transpose of L bit for bit, or absent
    ic = generate(gexec, "ic", dev, both_factors=True)
    lower = sp.csr_matrix(tuple(csr_arrays(ic.get_l_factor()))[::-1], shape=(n, n))
    upper = lower.T.tocsr()
    upper.sort_indices()
    got = csr_arrays(ic.get_lt_factor())
    same(got, (upper.indptr, upper.indices, upper.data), itype)
    alone = generate(gexec, "ic", dev, both_factors=False)
    assert alone.get_lt_factor() is None
    same(csr_arrays(alone.get_l_factor()), csr_arrays(ic.get_l_factor()), itype)


# ------------------------------------------------------------------ input handling
def shuffled(rp, ci, v, rng, upper_only=False):
    ci, v = ci.copy(), v.copy()
    for r in range(len(rp) - 1):
        lo, hi = rp[r], rp[r + 1]
        if upper_only:
            lo += np.searchsorted(ci[lo:hi], r) + 1
        p = rng.permutation(hi - lo)
        ci[lo:hi], v[lo:hi] = ci[lo:hi][p], v[lo:hi][p]
    return ci, v


@pytest.mark.parametrize("kind", KINDS)
def test_unsorted_input_is_sorted_unless_told_not_to(gexec, kind):
    a = case_matrix("small", kind == "ic")
    rp, ci, v = fr.arrays(a)
    ref = reference(kind, rp, ci, v)
    ci_u, v_u = shuffled(rp, ci, v, np.random.default_rng(8))
    assert not np.array_equal(ci_u, ci)
    dev = device_csr(gexec, rp, ci_u, v_u)
    same(factors_of(kind, generate(gexec, kind, dev)), ref, np.int32)
    assert np.array_equal(dev.col_idxs.cpu().numpy(), ci_u), "generate changed the caller's matrix"
    # sorted input and skip_sorting: the same factors
    same(factors_of(kind, generate(gexec, kind, device_csr(gexec, rp, ci, v), skip_sorting=True)), ref, np.int32)
    if kind == "ilu":
        # skip_sorting on rows whose UPPER entries are out of order (lower parts and pivots are where the
        # kernel expects them): U keeps the storage order, so nothing was sorted
        ci_u, v_u = shuffled(rp, ci, v, np.random.default_rng(9), upper_only=True)
        fact = generate(gexec, kind, device_csr(gexec, rp, ci_u, v_u), skip_sorting=True)
        want = fr.split_l_u(rp, ci_u, v_u)
        got = factors_of(kind, fact)
        for k in (0, 1, 3, 4):
            assert np.array_equal(got[k], want[k])
        assert not np.array_equal(got[4], ref[4])


@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
def test_missing_diagonals_become_explicit_zeros(gexec, dtype, itype):
    """rows 5, 57 and 199 lose their diagonal entry; each has a lower neighbour k with (k, i) stored, so the
    ILU pivot is filled by -a_ik a_ki and everything stays finite; the IC pivot is the root of a negative
    number, and the NaNs are where the reference has them"""
    a = case_matrix("small", True)
    rp, ci, v = fr.arrays(a, itype, dtype)
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    gone = np.isin(rows, (5, 57, 199)) & (rows == ci)
    assert gone.sum() == 3 and all(rp[i + 1] - rp[i] > 1 and ci[rp[i]] < i for i in (5, 57, 199))
    zeroed = v.copy()
    zeroed[gone] = 0
    rp_m = np.zeros_like(rp)
    rp_m[1:] = np.cumsum(np.bincount(rows[~gone], minlength=n))
    dev = device_csr(gexec, rp_m, ci[~gone], v[~gone])
    ref = fr.ilu_factors(rp, ci, zeroed)
    assert all(np.isfinite(x).all() for x in ref)
    same(factors_of("ilu", generate(gexec, "ilu", dev)), ref, itype)
    ref = fr.ic_factor(rp, ci, zeroed)
    assert np.isnan(ref[2]).any()
    same(factors_of("ic", generate(gexec, "ic", dev)), ref, itype, equal_nan=True)


def test_an_fbcsr_system_matrix(gexec):
    rng = np.random.default_rng(12)
    blocks = sp.random(40, 40, 0.1, random_state=rng, format="csr")
    blocks = blocks + blocks.T + sp.eye(40)
    a = sp.kron(blocks, np.ones((3, 3)), format="csr")
    a.data = rng.uniform(-1, 1, a.nnz)
    a = (a + a.T + sp.diags(np.full(120, 40.0))).tocsr()
    fb = g.Fbcsr.from_scipy(gexec, sp.bsr_matrix(a, blocksize=(3, 3)))
    csr = fb.convert_to_csr()
    for kind in KINDS:
        f1, f2 = generate(gexec, kind, fb), generate(gexec, kind, csr)
        for p, q in zip(factors_of(kind, f1), factors_of(kind, f2)):
            assert p.size and np.array_equal(p, q) and np.isfinite(p).all()
        m1 = (g.Ilu if kind == "ilu" else g.Ic).build().on(gexec).generate(fb)
        for p, q in zip(factors_of(kind, m1.factorization), factors_of(kind, f2)):
            assert np.array_equal(p, q)


@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
def test_a_zero_pivot_gives_the_reference_non_finite_entries(gexec, dtype, itype):
    a = case_matrix("small", False).tolil()
    a[0, :], a[1, :] = 0, 0
    a[:, 0], a[:, 1] = 0, 0
    a[0, 1] = a[1, 0] = a[1, 1] = 1.0
    a[2, 1] = a[1, 2] = 0.5
    a = a.tocsr()
    rp, ci, v = fr.arrays(a, itype, dtype)
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    # the pattern keeps the (0, 0) entry, as an explicit zero
    assert not ((rows == 0) & (ci == 0)).any()
    fact = generate(gexec, "ilu", device_csr(gexec, rp, ci, v))
    filled = a.tolil()
    filled[0, 0] = 1.0
    rp_f, ci_f, v_f = fr.arrays(filled.tocsr(), itype, dtype)
    v_f[0] = 0
    ref = fr.ilu_factors(rp_f, ci_f, v_f)
    assert not np.isfinite(ref[2]).all() and not np.isfinite(ref[5]).all()
    same(factors_of("ilu", fact), ref, itype, equal_nan=True)
    # the call succeeded; the next factorization on this executor is right
    check_case(gexec, "ilu", "small", case_matrix("small", False), dtype, itype)


def test_invalid_arguments_are_refused_and_the_device_stays_usable(gexec):
    from ginkgo_amd._lib import call, lib
    a = case_matrix("small", False)
    rp, ci, v = fr.arrays(a)
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    dev = device_csr(gexec, rp, ci, v)
    st = gexec.stream

    def schedule(m, upper=False):
        h = C.c_void_p()
        call("gkoc_%s_trs_generate_i32" % ("upper" if upper else "lower"), st, m.size[0], m.row_ptrs, m.col_idxs,
             C.byref(h))
        return h

    low = sp.tril(a, format="csr")
    dev_low = device_csr(gexec, *fr.arrays(low))
    # a row (57) without its diagonal; a lower triangle with one entry right of a diagonal (row 57 again)
    keep = ~((rows == 57) & (ci == 57))
    rp_m = np.zeros_like(rp)
    rp_m[1:] = np.cumsum(np.bincount(rows[keep], minlength=n))
    dev_missing = device_csr(gexec, rp_m, ci[keep], v[keep])
    extra = low.tolil()
    extra[57, 58] = 0.25
    dev_extra = device_csr(gexec, *fr.arrays(extra.tocsr()))
    handles = {m: schedule(m) for m in (dev, dev_low, dev_missing, dev_extra)}
    upper = schedule(dev, upper=True)
    try:
        full, tri = handles[dev], handles[dev_low]
        bad = [("gkoc_ilu_factorize_f64_i32", C.c_void_p(0), n, dev),             # a null structure
               ("gkoc_ilu_factorize_f64_i32", upper, n, dev),                      # of the upper triangle
               ("gkoc_ilu_factorize_f64_i32", full, n - 1, dev),                   # of another n
               ("gkoc_ilu_factorize_f64_i32", tri, n, dev),                        # of another nnz
               ("gkoc_ilu_factorize_f64_i32", full, -1, dev),
               ("gkoc_ilu_factorize_f64_i32", handles[dev_missing], n, dev_missing),   # a row without a diagonal
               ("gkoc_ic_factorize_f64_i32", C.c_void_p(0), n, dev_low),
               ("gkoc_ic_factorize_f64_i32", upper, n, dev_low),
               ("gkoc_ic_factorize_f64_i32", tri, n - 1, dev_low),
               ("gkoc_ic_factorize_f64_i32", full, n, dev_low),
               ("gkoc_ic_factorize_f64_i32", handles[dev_missing], n, dev_missing),
               ("gkoc_ic_factorize_f64_i32", handles[dev_extra], n, dev_extra),    # diagonal not last
               ("gkoc_ic_factorize_f64_i32", full, n, dev)]                        # the same, a full matrix
        for name, handle, n_, m in bad:
            before = m.values.cpu().numpy().copy()
            with pytest.raises(g.GkoError):
                call(name, st, handle, n_, m.row_ptrs, m.col_idxs, m.values)
            assert np.array_equal(m.values.cpu().numpy(), before), name + " wrote values before it refused"
        for name in ("gkoc_ilu_factorize_f64_i32", "gkoc_ic_factorize_f64_i32"):
            for kw in (dict(rp_=None), dict(ci_=None), dict(v_=None)):
                args = dict(rp_=dev_low.row_ptrs, ci_=dev_low.col_idxs, v_=dev_low.values)
                args.update(kw)
                with pytest.raises(g.GkoError):
                    call(name, st, tri, n, args["rp_"], args["ci_"], args["v_"])
        with pytest.raises(g.GkoError):
            call("gkoc_factorization_row_limits", None, None)
        l_rp = gexec.alloc((n + 1,), dev.row_ptrs.dtype)
        l_v = gexec.alloc((a.nnz + n,), dev.values.dtype)
        with pytest.raises(g.GkoError):
            call("gkoc_factorization_initialize_l_u_f64_i32", st, -1, dev.row_ptrs, dev.col_idxs, dev.values,
                 l_rp, l_v, l_rp, l_v)
        with pytest.raises(g.GkoError):
            call("gkoc_factorization_initialize_l_u_f64_i32", st, n, dev.row_ptrs, dev.col_idxs, dev.values,
                 l_rp, l_v, l_rp, None)
        with pytest.raises(g.GkoError):
            call("gkoc_factorization_initialize_l_f64_i32", st, n, dev.row_ptrs, dev.col_idxs, dev.values,
                 l_rp, None, C.c_int(0))
        # nothing of the above reached the values: valid calls on the same arrays are still right
        call("gkoc_ilu_factorize_f64_i32", st, full, n, dev.row_ptrs, dev.col_idxs, dev.values)
        assert np.array_equal(dev.values.cpu().numpy(), fr.ilu0(rp, ci, v))
        call("gkoc_ic_factorize_f64_i32", st, tri, n, dev_low.row_ptrs, dev_low.col_idxs, dev_low.values)
        assert np.array_equal(dev_low.values.cpu().numpy(), fr.ic0(*fr.arrays(low)))
    finally:
        for h in list(handles.values()) + [upper]:
            lib().gkoc_trs_struct_destroy(h)
    # the classes refuse what Ginkgo's refuse
    for cls in (g.factorization.Ilu, g.factorization.Ic, g.Ilu, g.Ic):
        with pytest.raises(g.NotSupported):
            cls.build().on(gexec).generate(g.Dense.create(gexec, (4, 4)))
        with pytest.raises(g.NotSupported):
            cls.build().on(gexec).generate(dev.convert_to_ell())
        wide = g.Csr.from_arrays(gexec, (2, 3), np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32),
                                 np.ones(2))
        with pytest.raises(g.DimensionMismatch):
            cls.build().on(gexec).generate(wide)
        cplx = g.Csr.from_arrays(gexec, (2, 2), np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32),
                                 np.ones(2, np.complex128))
        with pytest.raises(g.NotSupported):
            cls.build().on(gexec).generate(cplx)


@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
def test_split_entries_directly(gexec, dtype, itype):
    """initialize_l_u / initialize_l (they write values; the index arrays are the Sor set-up's) on an unsorted
    matrix with rows that lack a diagonal: storage order is kept, a missing diagonal counts as 1, diag_sqrt
    takes the root, and the index arrays handed in are left alone"""
    from ginkgo_amd._lib import IT, VT, call
    a = case_matrix("small", True)
    rp, ci, v = fr.arrays(a, itype, dtype)
    ci, v = shuffled(rp, ci, v, np.random.default_rng(4))
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    keep = ~(np.isin(rows, (0, 100, n - 1)) & (rows == ci))
    rp_m = np.zeros_like(rp)
    rp_m[1:] = np.cumsum(np.bincount(rows[keep], minlength=n))
    ci, v = ci[keep], v[keep]
    dev = device_csr(gexec, rp_m, ci, v)
    suf = "%s_%s" % (VT[dev.dtype], IT[dev.col_idxs.dtype])
    src = (gexec.stream, n, dev.row_ptrs, dev.col_idxs, dev.values)
    want = fr.split_l_u(rp_m, ci, v)
    l_rp, l_ci, l_v, u_rp, u_ci, u_v = (gexec.to_device(np.full_like(x, 9)) for x in want)
    call("gkoc_factorization_initialize_row_ptrs_l_u_" + suf[4:], gexec.stream, n, dev.row_ptrs, dev.col_idxs,
         l_rp, u_rp)
    call("gkoc_sor_initialize_weighted_l_u_" + suf, *src, C.c_double(1.0), l_rp, l_ci, l_v, u_rp, u_ci, u_v)
    call("gkoc_factorization_initialize_l_u_" + suf, *src, l_rp, l_v, u_rp, u_v)
    same([t.cpu().numpy() for t in (l_rp, l_ci, l_v, u_rp, u_ci, u_v)], want, itype)
    for root in (0, 1):
        want = fr.split_l(rp_m, ci, v, bool(root))
        l_v.fill_(9)
        call("gkoc_factorization_initialize_l_" + suf, *src, l_rp, l_v, C.c_int(root))
        same([t.cpu().numpy() for t in (l_rp, l_ci, l_v)], want, itype)


# ------------------------------------------------------------------ the preconditioners
def strided(gexec, array, ld, fill=0.0):
    """(Dense view of `array` inside a store with row stride ld, the store)"""
    n, k = array.shape
    full = np.full((n, ld), fill, array.dtype)
    full[:, :k] = array
    store = gexec.to_device(full)
    return g.Dense(gexec, store[:, :k]), store


def transposed(rp, ci, v):
    n = len(rp) - 1
    t = sp.csr_matrix((v, ci, rp), shape=(n, n)).T.tocsr()
    t.sort_indices()
    return t.indptr.astype(rp.dtype), t.indices.astype(ci.dtype), t.data


@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("kind", ["ilu", "ilu-reverse", "ic"])
def test_apply_is_the_two_reference_solves(gexec, kind, dtype, itype):
    a = case_matrix("small", kind == "ic")
    rp, ci, v = fr.arrays(a, itype, dtype)
    n = len(rp) - 1
    dev = device_csr(gexec, rp, ci, v)
    if kind == "ic":
        lower = fr.ic_factor(rp, ci, v)
        upper = transposed(*lower)
        m = g.Ic.build().on(gexec).generate(dev)
        assert isinstance(m.factorization, g.factorization.Ic)
    else:
        f = fr.ilu_factors(rp, ci, v)
        lower, upper = f[:3], f[3:]
        m = g.Ilu.build().with_reverse_apply(kind == "ilu-reverse").on(gexec).generate(dev)
        assert isinstance(m.factorization, g.factorization.Ilu)

    def ref(b):
        if kind == "ilu-reverse":
            return tr.trs_solve(*lower, tr.trs_solve(*upper, b, upper=True))
        return tr.trs_solve(*upper, tr.trs_solve(*lower, b), upper=True)

    for nrhs in (1, 3):
        b = np.random.default_rng(nrhs).uniform(-1, 1, (n, nrhs)).astype(dtype)
        want = ref(b)
        assert np.isfinite(want).all()
        bd, _ = strided(gexec, b, nrhs + 3, fill=7.0)
        xd, store = strided(gexec, np.full_like(b, np.nan), nrhs + 2, fill=np.nan)
        m.apply(bd, xd)
        full = store.cpu().numpy()
        assert np.isnan(full[:, nrhs:]).all(), "the apply wrote into the padding of x"
        assert np.array_equal(full[:, :nrhs], want)
        # advanced apply on the same strided vectors
        x0 = np.random.default_rng(5).uniform(-1, 1, (n, nrhs)).astype(dtype)
        xd, store = strided(gexec, x0, nrhs + 2, fill=np.nan)
        m.apply(g.Dense.from_numpy(gexec, np.array([[-1.0]], dtype)), bd,
                g.Dense.from_numpy(gexec, np.array([[2.0]], dtype)), xd)
        full = store.cpu().numpy()
        assert np.isnan(full[:, nrhs:]).all()
        assert np.array_equal(full[:, :nrhs], dtype(2) * x0 + dtype(-1) * want)


def criteria():
    return (g.stop.Iteration.build().with_max_iters(1000),
            g.stop.ResidualNorm.build().with_reduction_factor(1e-10))


@pytest.fixture(scope="module")
def model_problem(gexec, oracle):
    rp, ci, v = oracle.stencil_csr(3, 12)
    n = 12 ** 3
    a = g.Csr.from_arrays(gexec, (n, n), rp, ci, v)
    b = np.random.default_rng(3).uniform(-1, 1, n)
    return a, sp.csr_matrix((v, ci, rp), shape=(n, n)), b


def solve_with(gexec, cls, a, b, precond, **params):
    f = cls.build().with_criteria(*criteria()).with_preconditioner(precond)
    for k, v in params.items():
        f = getattr(f, "with_" + k)(v)
    solver = f.on(gexec).generate(a)
    x = g.Dense.from_numpy(gexec, np.zeros_like(b))
    solver.apply(g.Dense.from_numpy(gexec, b), x)
    return solver, x.to_numpy()[:, 0]


def test_cg_with_ic_and_ilu_beats_scalar_jacobi(gexec, model_problem):
    a, a_host, b = model_problem
    factories = {"Ic": lambda: g.Ic.build(), "Ilu": lambda: g.Ilu.build(),
                 "Jacobi": lambda: g.Jacobi.build().with_max_block_size(1),
                 "SSOR": lambda: g.Sor.build().with_relaxation_factor(1.0).with_symmetric(True)}
    graph = {k: solve_with(gexec, g.Cg, a, b, f()) for k, f in factories.items()}
    print("iterations:", {k: s.num_iterations for k, (s, _) in graph.items()})
    for k in ("Ic", "Ilu", "Jacobi"):
        s, x = graph[k]
        assert s.has_converged and s.num_iterations < 1000, k
        assert np.linalg.norm(b - a_host @ x) <= 1e-9 * np.linalg.norm(b), k
    assert graph["Ic"][0].num_iterations < graph["Jacobi"][0].num_iterations
    assert graph["Ilu"][0].num_iterations < graph["Jacobi"][0].num_iterations
    # captured iterations (the default at this size) against plain launches
    plain = {k: solve_with(gexec, g.Cg, a, b, factories[k](), hip_graph=False) for k in ("Ic", "Ilu", "Jacobi")}
    for k in plain:
        assert plain[k][0].has_converged and plain[k][0].num_iterations == graph[k][0].num_iterations, k
    control = np.array_equal(graph["Jacobi"][1], plain["Jacobi"][1])
    print("scalar Jacobi bit-equal between graph and plain launches:", control)
    if control:
        assert np.array_equal(graph["Ic"][1], plain["Ic"][1])
        assert np.array_equal(graph["Ilu"][1], plain["Ilu"][1])


def test_other_solvers_and_generated_preconditioners(gexec, model_problem):
    a, a_host, b = model_problem
    rp, ci, v = csr_arrays(a)
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    # an unsymmetric perturbation of the stencil: every off-diagonal shrunk by up to 20 %, independently in
    # the two triangles, so the rows stay diagonally dominant
    v = np.where(rows == ci, v, v * np.random.default_rng(7).uniform(0.8, 1.0, v.size))
    u, u_host = g.Csr.from_arrays(gexec, (n, n), rp, ci, v), sp.csr_matrix((v, ci, rp), shape=(n, n))
    assert abs(u_host - u_host.T).max() > 0.01
    for cls in (g.Gmres, g.Bicgstab):
        s, x = solve_with(gexec, cls, u, b, g.Ilu.build())
        assert s.has_converged and s.num_iterations < 1000, cls.__name__
        assert np.linalg.norm(b - u_host @ x) <= 1e-8 * np.linalg.norm(b), cls.__name__
    # prebuilt factorization objects, generated preconditioners
    ilu = g.Ilu.build().with_reverse_apply(False).on(gexec).generate(
        g.factorization.Ilu.build().with_skip_sorting(True).on(gexec).generate(a))
    ic = g.Ic.build().on(gexec).generate(
        g.factorization.Ic.build().with_both_factors(False).on(gexec).generate(a))
    for m in (ilu, ic):
        f = g.Cg.build().with_criteria(*criteria()).with_generated_preconditioner(m).on(gexec)
        s = f.generate(a)
        x = g.Dense.from_numpy(gexec, np.zeros_like(b))
        s.apply(g.Dense.from_numpy(gexec, b), x)
        assert s.get_preconditioner() is m and s.has_converged
        assert np.linalg.norm(b - a_host @ x.to_numpy()[:, 0]) <= 1e-9 * np.linalg.norm(b)
