"""GeneralIsai / SpdIsai on the device against the numpy Gauss-Jordan of tests/isai_general_refs.py, and as
preconditioners and smoothers.  Values are compared with np.array_equal: the kernel promises the reference's
rounding, pivots included."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import ginkgo_amd as g
import factorization_refs as fr
import isai_general_refs as gr
from ginkgo_amd import _lib
from ginkgo_amd._lib import call
from test_factorization_gpu import (TYPES, TYPE_IDS, criteria, csr_arrays, model_problem,  # noqa: F401
                                    shuffled, solve_with, strided)

pytestmark = pytest.mark.gpu

KINDS = ["general", "spd"]
# (case, power, the kinds it runs for)
CASES = [("one", 1, KINDS), ("diagonal", 1, KINDS), ("stencil6", 1, KINDS), ("stencil5", 2, KINDS),
         ("convection", 1, KINDS[:1]), ("weak", 1, KINDS[:1])]
CASE_PARAMS = [(name, power, kind) for name, power, kinds in CASES for kind in kinds]
LONGEST = {("stencil6", "spd"): 14, ("stencil6", "general"): 27, ("stencil5", "spd"): 63, ("stencil5", "general"): 125}


# ------------------------------------------------------------------ helpers
def cls_of(kind):
    return g.SpdIsai if kind == "spd" else g.GeneralIsai


def device_csr(gexec, rp, ci, v):
    """a device matrix of copies: the shared host arrays are read-only"""
    n = len(rp) - 1
    return g.Csr.from_arrays(gexec, (n, n), np.array(rp), np.array(ci), np.array(v))


def generate(gexec, kind, a, **params):
    f = cls_of(kind).build()
    for k, val in params.items():
        f = getattr(f, "with_" + k)(val)
    return f.on(gexec).generate(a)


_MATRICES, _REFS = {}, {}   # computed once per key and left unchanged; the tests copy what they change


def frozen(arrays):
    for x in arrays:
        x.setflags(write=False)
    return tuple(arrays)


def case_arrays(name, kind, dtype):
    """(rp, ci, v), int32 indices, of the system matrix of a case"""
    key = (name, kind if name.startswith("hub") else None, dtype)
    if key not in _MATRICES:
        if name == "one":
            a = (np.array([0, 1], np.int32), np.array([0], np.int32), np.array([2.0], dtype))
        elif name == "diagonal":
            a = (np.arange(301, dtype=np.int32), np.arange(300, dtype=np.int32),
                 np.random.default_rng(3).uniform(1, 2, 300).astype(dtype))
        elif name.startswith("stencil"):
            a = fr.arrays(fr.stencil27(int(name[7:])), np.int32, dtype)
        elif name == "convection":
            a = gr.convection(8, dtype)
        elif name == "small":
            a = gr.convection(4, dtype)
        elif name == "weak":
            a = gr.weak_diagonal(dtype=dtype)
        elif name.startswith("hub"):
            a = gr.hub(int(name[3:]), kind == "spd", dtype=dtype)
        else:
            raise KeyError(name)
        _MATRICES[key] = frozen(a)
    return _MATRICES[key]


def pattern_of(rp, ci, kind, power):
    return gr.lower_pattern_power(rp, ci, power) if kind == "spd" else gr.pattern_power(rp, ci, power)


def reference(name, kind, dtype, power):
    """(w_rp, w_ci, w_v) of the reference, int32 indices"""
    key = (name, kind, dtype, power)
    if key not in _REFS:
        rp, ci, v = case_arrays(name, kind, dtype)
        w_rp, w_ci = pattern_of(rp, ci, kind, power)
        _REFS[key] = frozen([w_rp, w_ci, gr.general_inverse(rp, ci, v, w_rp, w_ci, kind == "spd")])
    return _REFS[key]


def check_against(gexec, kind, arrays, want, itype, power):
    """generate on the device matrix of `arrays` and compare W with `want` = (w_rp, w_ci, w_v)"""
    rp, ci, v = arrays[0].astype(itype), arrays[1].astype(itype), arrays[2]
    dev = device_csr(gexec, rp, ci, v)
    m = generate(gexec, kind, dev, sparsity_power=power)
    for got, kept in zip(csr_arrays(dev), (rp, ci, v)):
        assert np.array_equal(got, kept, equal_nan=True), "generate changed the caller's matrix"
    inv = m.get_approximate_inverse()
    assert isinstance(inv, g.Csr) and inv.size == dev.size and m.get_size() == dev.size
    got = csr_arrays(inv)
    assert got[0].dtype == got[1].dtype == itype and got[2].dtype == v.dtype
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    if power == 1 and kind == "general":
        # A's own index arrays, shared and not copied
        assert inv.row_ptrs.data_ptr() == dev.row_ptrs.data_ptr() and inv.col_idxs.data_ptr() == dev.col_idxs.data_ptr()
    # masks first: which rows are the identity's, then the bits
    assert np.array_equal(gr.identity_rows(*got), gr.identity_rows(*want))
    assert np.array_equal(got[2], want[2])
    return m


def check_case(gexec, name, kind, dtype, itype, power):
    want = reference(name, kind, dtype, power)
    assert np.isfinite(want[2]).all()
    return check_against(gexec, kind, case_arrays(name, kind, dtype), want, itype, power)


# ------------------------------------------------------------------ values and pattern, bit for bit
@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("name,power,kind", CASE_PARAMS, ids=["%s-p%d-%s" % c for c in CASE_PARAMS])
def test_inverse_matches_reference(gexec, name, power, kind, dtype, itype):
    check_case(gexec, name, kind, dtype, itype, power)
    w_rp, w_ci, w_v = reference(name, kind, dtype, power)
    lengths = np.diff(w_rp)
    if (name, kind) in LONGEST:
        assert int(lengths.max()) == LONGEST[(name, kind)]
    if (name, kind) == ("stencil5", "general"):
        # both kernels of one call: rows on either side of 64 entries
        assert (lengths <= 64).any() and (lengths > 64).any()
    if name not in ("one", "diagonal"):
        assert not gr.identity_rows(w_rp, w_ci, w_v).any()


def boundary_lengths():
    limits = g.isai.general_row_limits()
    assert 1 <= len(limits) <= 4 and limits == sorted(set(limits)) and limits[0] >= 8 and limits[-1] >= 128
    return sorted({x for limit in limits[:-1] for x in (limit, limit + 1)} | {64, 65, limits[-1]})


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_hub_rows_at_every_path_boundary(gexec, kind, dtype):
    """the paths are chosen from the LONGEST pattern row, so every length gets a matrix of its own in which one
    hub row (spd: its lower part) has exactly that many entries and no other more than 3"""
    lengths = boundary_lengths()
    assert {64, 65, 128} <= set(lengths) and len(lengths) >= 5
    for length in lengths:
        name = "hub%d" % length
        stored = np.diff(reference(name, kind, dtype, 1)[0])
        assert stored.max() == length and np.sort(stored)[-2] <= 3
        check_case(gexec, name, kind, dtype, np.int32, 1)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_a_row_above_the_cap_is_refused_before_anything_is_written(gexec, kind, dtype):
    cap = g.isai.general_row_limits()[-1]
    rp, ci, v = gr.hub(cap + 1, kind == "spd", dtype=dtype)
    with pytest.raises(g.NotSupported, match=r"%d\D+%d" % (cap + 1, cap)):
        generate(gexec, kind, device_csr(gexec, rp, ci, v))
    w_rp, w_ci = pattern_of(rp, ci, kind, 1)
    assert np.diff(w_rp).max() == cap + 1
    suffix = "f64_i32" if dtype == np.float64 else "f32_i32"
    a, pattern = [gexec.to_device(np.array(x)) for x in (rp, ci, v)], [gexec.to_device(x) for x in (w_rp, w_ci)]
    w = gexec.to_device(np.full(len(w_ci), 9.0, dtype))
    with pytest.raises(g.NotSupported):
        call("gkoc_isai_generate_general_inverse_" + suffix, gexec.stream, len(rp) - 1, C.c_int(kind == "spd"),
             *a, *pattern, w)
    assert (w.cpu().numpy() == 9.0).all(), "w_v was written before the refusal"
    # the device stays usable
    check_case(gexec, "hub%d" % cap, kind, dtype, np.int32, 1)


# ------------------------------------------------------------------ the rules
def test_a_singular_block_gives_the_identity_row(gexec):
    """rows 10 and 11 of A are equal and store the columns 10 and 11 only: every block that holds both is
    singular, its elimination meets an exact zero pivot"""
    dense = np.diag(np.full(40, 4.0)) + np.diag(np.full(39, -1.0), 1) + np.diag(np.full(39, -1.5), -1)
    dense[10:12] = 0
    dense[10:12, 10:12] = 1
    for dtype in (np.float64, np.float32):
        rp, ci, v = fr.arrays(sp.csr_matrix(dense), np.int32, dtype)
        want = (rp, ci, gr.general_inverse(rp, ci, v, rp, ci, False))
        identity = gr.identity_rows(*want)
        assert np.isfinite(want[2]).all() and list(np.flatnonzero(identity)) == [10, 11]
        check_against(gexec, "general", (rp, ci, v), want, np.int32, 1)


def test_spd_with_a_negative_diagonal_gives_the_references_identity_rows(gexec):
    rp, ci, v = (x.copy() for x in fr.arrays(fr.stencil27(4)))
    rows = np.repeat(np.arange(64), np.diff(rp))
    v[(rows == 21) & (ci == 21)] = -26.0
    for power in (1, 2):
        w_rp, w_ci = gr.lower_pattern_power(rp, ci, power)
        want = (w_rp, w_ci, gr.general_inverse(rp, ci, v, w_rp, w_ci, True))
        identity = gr.identity_rows(*want)
        assert np.isfinite(want[2]).all() and identity[21] and 1 <= identity.sum() < 64
        check_against(gexec, "spd", (rp, ci, v), want, np.int32, power)


@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
def test_a_nan_gives_the_references_identity_rows(gexec, dtype, itype):
    rp, ci, v = (x.copy() for x in case_arrays("small", None, dtype))
    rows = np.repeat(np.arange(64), np.diff(rp))
    v[(rows == 21) & (ci == 22)] = np.nan
    for kind in KINDS:
        for power in (1, 2):
            w_rp, w_ci = pattern_of(rp, ci, kind, power)
            want = (w_rp, w_ci, gr.general_inverse(rp, ci, v, w_rp, w_ci, kind == "spd"))
            identity = gr.identity_rows(*want)
            # every row whose block holds the entry (21, 22); with the lower pattern of power 1 that is row 22 alone
            assert np.isfinite(want[2]).all() and 1 <= identity.sum() < 64 and identity[22]
            check_against(gexec, kind, (rp, ci, v), want, itype, power)


# ------------------------------------------------------------------ input handling
@pytest.mark.parametrize("kind", KINDS)
def test_unsorted_input_is_sorted_unless_told_not_to(gexec, kind):
    rp, ci, v = case_arrays("small", None, np.float64)
    ci_u, v_u = shuffled(rp, ci, v, np.random.default_rng(8))
    assert not np.array_equal(ci_u, ci)
    dev = device_csr(gexec, rp, ci_u, v_u)
    for power in (1, 2):
        want = reference("small", kind, np.float64, power)
        got = csr_arrays(generate(gexec, kind, dev, sparsity_power=power).get_approximate_inverse())
        assert all(np.array_equal(p, q) for p, q in zip(got, want))
        assert np.array_equal(dev.col_idxs.cpu().numpy(), ci_u) and np.array_equal(dev.values.cpu().numpy(), v_u), \
            "generate changed the caller's matrix"
    got = csr_arrays(generate(gexec, kind, device_csr(gexec, rp, ci, v), sparsity_power=2,
                              skip_sorting=True).get_approximate_inverse())
    assert all(np.array_equal(p, q) for p, q in zip(got, want))
    # unsorted input and skip_sorting: nothing was sorted, and the entry refuses unsorted rows
    with pytest.raises(g.GkoError):
        generate(gexec, kind, dev, skip_sorting=True)


def test_an_fbcsr_input_and_what_the_classes_refuse(gexec):
    rp, ci, v = case_arrays("small", None, np.float64)
    a = sp.csr_matrix((v, ci, rp), shape=(64, 64))
    for kind in KINDS:
        for block in (1, 2):
            fb = g.Fbcsr.from_scipy(gexec, sp.bsr_matrix(a, blocksize=(block, block)))
            csr = fb.convert_to_csr()
            m1, m2 = generate(gexec, kind, fb, sparsity_power=2), generate(gexec, kind, csr, sparsity_power=2)
            host = csr_arrays(csr)
            w_rp, w_ci = pattern_of(host[0], host[1], kind, 2)
            want = (w_rp, w_ci, gr.general_inverse(*host, w_rp, w_ci, kind == "spd"))
            got1, got2 = csr_arrays(m1.get_approximate_inverse()), csr_arrays(m2.get_approximate_inverse())
            for p, q, r in zip(got1, got2, want):
                assert p.size and np.array_equal(p, q) and np.array_equal(p, r)
    good = device_csr(gexec, rp, ci, v)
    for cls in (g.GeneralIsai, g.SpdIsai):
        for power in (0, -1):
            with pytest.raises(g.GkoError):
                cls.build().with_sparsity_power(power).on(gexec).generate(good)
        with pytest.raises(g.NotSupported):
            cls.build().on(gexec).generate(g.Dense.create(gexec, (4, 4)))
        with pytest.raises(g.NotSupported):
            cls.build().on(gexec).generate(good.convert_to_ell())
        wide = g.Csr.from_arrays(gexec, (2, 3), np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32), np.ones(2))
        with pytest.raises(g.DimensionMismatch):
            cls.build().on(gexec).generate(wide)
        cplx = g.Csr.from_arrays(gexec, (2, 2), np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32),
                                 np.ones(2, np.complex128))
        with pytest.raises(g.NotSupported):
            cls.build().on(gexec).generate(cplx)
        # a row without its diagonal: no pattern row may lack it
        hollow = g.Csr.from_arrays(gexec, (2, 2), np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32), np.ones(2))
        with pytest.raises(g.GkoError):
            cls.build().on(gexec).generate(hollow)


def test_invalid_arguments_are_refused_and_the_device_stays_usable(gexec):
    entry = "gkoc_isai_generate_general_inverse_f64_i32"
    st = gexec.stream
    rp, ci, v = (x.copy() for x in case_arrays("small", None, np.float64))
    n = len(rp) - 1
    w_rp, w_ci, w_want = reference("small", "general", np.float64, 2)
    l_rp, l_ci, l_want = reference("small", "spd", np.float64, 2)

    def dev(*arrays):
        return [gexec.to_device(np.array(x)) for x in arrays]

    def without(rp_, ci_, row, col):
        """the index arrays without the entry (row, col)"""
        rows_ = np.repeat(np.arange(n), np.diff(rp_))
        keep = ~((rows_ == row) & (ci_ == col))
        assert keep.sum() == len(ci_) - 1
        out = np.zeros_like(rp_)
        out[1:] = np.cumsum(np.bincount(rows_[keep], minlength=n))
        return out, ci_[keep]

    def swapped(rp_, ci_, row):
        """the first two entries of `row` exchanged"""
        out = ci_.copy()
        assert rp_[row + 1] - rp_[row] >= 2
        out[rp_[row]], out[rp_[row] + 1] = ci_[rp_[row] + 1], ci_[rp_[row]]
        return out

    a, pattern, lower = dev(rp, ci, v), dev(w_rp, w_ci), dev(l_rp, l_ci)
    ci_out = w_ci.copy()
    ci_out[w_rp[31] - 1] = n
    ci_neg = w_ci.copy()
    ci_neg[w_rp[30]] = -1
    a_out = ci.copy()
    a_out[rp[31] - 1] = n
    rp_bad = w_rp.copy()
    assert w_rp[11] > w_rp[10]
    rp_bad[10], rp_bad[11] = w_rp[11], w_rp[10]
    rp_first = w_rp.copy()
    rp_first[0] = 1
    a_rp_bad = rp.copy()
    a_rp_bad[10], a_rp_bad[11] = rp[11], rp[10]
    bad = [("an unsorted pattern row", 0, a, dev(w_rp, swapped(w_rp, w_ci, 17))),
           ("an unsorted row of A", 0, dev(rp, swapped(rp, ci, 17), v), pattern),
           ("a pattern row without its diagonal", 0, a, dev(*without(w_rp, w_ci, 40, 40))),
           ("a pattern row without its diagonal (spd)", 1, a, dev(*without(l_rp, l_ci, 40, 40))),
           ("spd with an upper entry", 1, a, pattern),
           ("a column >= n in the pattern", 0, a, dev(w_rp, ci_out)),
           ("a negative column in the pattern", 0, a, dev(w_rp, ci_neg)),
           ("a column >= n in A", 0, dev(rp, a_out, v), pattern),
           ("pattern row pointers that descend", 0, a, dev(rp_bad, w_ci)),
           ("pattern row pointers that start at 1", 0, a, dev(rp_first, w_ci)),
           ("row pointers of A that descend", 0, dev(a_rp_bad, ci, v), pattern),
           ("a negative size", 0, a, pattern)]
    w = gexec.to_device(np.full(len(w_ci), 9.0))
    for what, spd, a_, p_ in bad:
        n_ = -1 if what == "a negative size" else n
        with pytest.raises(g.GkoError) as raised:
            call(entry, st, n_, C.c_int(spd), *a_, *p_, w)
        assert not isinstance(raised.value, g.NotSupported) and "status -1" in str(raised.value), what
        assert (w.cpu().numpy() == 9.0).all(), what + ": w_v was written before the refusal"
    for k in range(6):
        args = a + pattern + [w]
        args[k] = None
        with pytest.raises(g.GkoError):
            call(entry, st, n, C.c_int(0), *args)
    assert (w.cpu().numpy() == 9.0).all()
    # nothing of the above reached the values or the device: valid calls on the same arrays are right
    call(entry, st, n, C.c_int(0), *a, *pattern, w)
    assert np.array_equal(w.cpu().numpy(), w_want)
    w_low = gexec.to_device(np.full(len(l_ci), 9.0))
    call(entry, st, n, C.c_int(1), *a, *lower, w_low)
    assert np.array_equal(w_low.cpu().numpy(), l_want)
    # a lower pattern is a pattern: the general solve on it, without the scaling
    call(entry, st, n, C.c_int(0), *a, *lower, w_low)
    assert np.array_equal(w_low.cpu().numpy(), gr.general_inverse(rp, ci, v, l_rp, l_ci, False))
    w_own = gexec.to_device(np.full(len(ci), 9.0))
    call(entry, st, n, C.c_int(0), *a, a[0], a[1], w_own)
    assert np.array_equal(w_own.cpu().numpy(), reference("small", "general", np.float64, 1)[2])
    call(entry, st, 0, C.c_int(0), None, None, None, None, None, None)


# ------------------------------------------------------------------ apply and transpose
def transposed(rp, ci, v):
    n = len(rp) - 1
    t = sp.csr_matrix((v, ci, rp), shape=(n, n)).T.tocsr()
    t.sort_indices()
    return t.indptr.astype(rp.dtype), t.indices.astype(ci.dtype), t.data


def applied(gexec, op, b, x0, alpha, beta):
    """(op b, alpha op b + beta x0) through strided vectors whose padding must stay untouched"""
    nrhs = b.shape[1]
    bd, _ = strided(gexec, b, nrhs + 3, fill=7.0)
    xd, store = strided(gexec, np.full_like(b, np.nan), nrhs + 2, fill=np.nan)
    op.apply(bd, xd)
    full = store.cpu().numpy()
    assert np.isnan(full[:, nrhs:]).all(), "the apply wrote into the padding of x"
    yd, ystore = strided(gexec, x0, nrhs + 2, fill=np.nan)
    op.apply(alpha, bd, beta, yd)
    yfull = ystore.cpu().numpy()
    assert np.isnan(yfull[:, nrhs:]).all()
    assert np.isfinite(full[:, :nrhs]).all() and np.isfinite(yfull[:, :nrhs]).all()
    return full[:, :nrhs], yfull[:, :nrhs]


class ByHand:
    """x = W^T (W b) with Csr.apply and Csr.transpose()"""

    def __init__(self, gexec, w):
        self.gexec, self.w, self.wt = gexec, w, w.transpose()

    def apply(self, *args):
        b, x = args[-3] if len(args) == 4 else args[0], args[-1]
        t = g.Dense.create(self.gexec, b.size, b.dtype)
        self.w.apply(b, t)
        if len(args) == 4:
            self.wt.apply(args[0], t, args[2], x)
        else:
            self.wt.apply(t, x)


@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_apply_is_the_csr_apply_of_the_reference_inverse(gexec, kind, dtype, itype):
    m = check_case(gexec, "small", kind, dtype, itype, 2)
    w_rp, w_ci, w_v = reference("small", kind, dtype, 2)
    n = len(w_rp) - 1
    inv = m.get_approximate_inverse()
    alpha = g.Dense.from_numpy(gexec, np.array([[-1.5]], dtype))
    beta = g.Dense.from_numpy(gexec, np.array([[0.75]], dtype))
    t = m.transpose()
    assert isinstance(t, g.base.LinOp) and t.get_size() == m.get_size()
    w64 = sp.csr_matrix((w_v.astype(np.float64), w_ci, w_rp), shape=(n, n))
    if kind == "spd":
        assert t is m and m.conj_transpose() is m
        ops = [(m, ByHand(gexec, inv), w64.T @ w64)]
    else:
        assert type(t) is g.GeneralIsai and t is not m and t.sparsity_power == 2
        for got, want in zip(csr_arrays(t.get_approximate_inverse()), transposed(w_rp, w_ci, w_v)):
            assert np.array_equal(got, want)
        ops = [(m, inv, w64), (t, t.get_approximate_inverse(), w64.T)]
    for op, by_hand, host in ops:
        for nrhs in (1, 3):
            b = np.random.default_rng(nrhs).uniform(-1, 1, (n, nrhs)).astype(dtype)
            x0 = np.random.default_rng(5).uniform(-1, 1, (n, nrhs)).astype(dtype)
            got, want = applied(gexec, op, b, x0, alpha, beta), applied(gexec, by_hand, b, x0, alpha, beta)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            # and the product is the product: against scipy, to the SpMV's rounding (two products for spd)
            exact = host @ b.astype(np.float64)
            bound = (abs(host) @ np.abs(b).astype(np.float64)).max()
            assert np.abs(got[0] - exact).max() <= 64 * np.finfo(dtype).eps * bound
            # apply_advanced agrees with alpha apply + beta x to the same tolerance
            combined = -1.5 * got[0].astype(np.float64) + 0.75 * x0.astype(np.float64)
            assert np.abs(got[1] - combined).max() <= 64 * np.finfo(dtype).eps * (1.5 * bound + 0.75)


def test_an_spd_application_neither_copies_to_the_host_nor_synchronises(gexec):
    rp, ci, v = case_arrays("small", None, np.float64)
    m = generate(gexec, "spd", device_csr(gexec, rp, ci, v), sparsity_power=2)
    alpha, beta = g.Dense.from_numpy(gexec, np.array([[2.0]])), g.Dense.from_numpy(gexec, np.array([[0.5]]))
    for nrhs in (1, 3):
        b = g.Dense.from_numpy(gexec, np.ones((64, nrhs)))
        x = g.Dense.from_numpy(gexec, np.zeros((64, nrhs)))
        m.apply(b, x)                   # the intermediate vector of this column count is allocated here
        before = gexec.arena_info()["num_allocations"]
        with _lib.record() as tape:
            m.apply(b, x)
            m.apply(alpha, b, beta, x)
        names = [name for _, _, name in tape.calls]
        assert names == ["gkoc_csr_spmv_f64_i32"] * 3 + ["gkoc_csr_advanced_spmv_f64_i32"], names
        assert gexec.arena_info()["num_allocations"] == before


# ------------------------------------------------------------------ the preconditioners
def smallest_symmetric_eigenvalue(a_host):
    """of (A + A^T) / 2: where it is positive, ||A^-1|| <= 1 / that, so ||x - x*|| <= ||b - A x|| / that"""
    sym = ((a_host + a_host.T) * 0.5).tocsc()
    lam = float(spla.eigsh(sym, k=1, sigma=0, which="LM", return_eigenvectors=False)[0])
    assert lam > 0
    return lam


def check_solution(a_host, b, x, reduction):
    """the residual at the tolerance of the existing preconditioner tests, and x against scipy's direct solve
    within what that residual allows"""
    assert np.linalg.norm(b - a_host @ x) <= reduction * np.linalg.norm(b)
    direct = spla.spsolve(a_host.tocsc(), b)
    allowed = 2 * reduction * np.linalg.norm(b) / smallest_symmetric_eigenvalue(a_host)
    assert np.linalg.norm(x - direct) <= allowed


def test_cg_with_spd_isai_beats_scalar_jacobi(gexec, model_problem):
    a, a_host, b = model_problem
    jacobi, _ = solve_with(gexec, g.Cg, a, b, g.Jacobi.build().with_max_block_size(1))
    assert jacobi.has_converged
    its = {}
    for power in (1, 2):
        s, x = solve_with(gexec, g.Cg, a, b, g.SpdIsai.build().with_sparsity_power(power))
        assert s.has_converged and isinstance(s.get_preconditioner(), g.SpdIsai), power
        check_solution(a_host, b, x, 1e-9)
        its[power] = s.num_iterations
    print("CG iterations: scalar Jacobi %d, SpdIsai %s" % (jacobi.num_iterations, its))
    assert its[2] <= its[1] < jacobi.num_iterations
    # a generated operator instead of a factory: the same solve
    op = g.SpdIsai.build().on(gexec).generate(a)
    f = g.Cg.build().with_criteria(*criteria()).with_generated_preconditioner(op).on(gexec).generate(a)
    x = g.Dense.from_numpy(gexec, np.zeros_like(b))
    f.apply(g.Dense.from_numpy(gexec, b), x)
    assert f.get_preconditioner() is op and f.has_converged and f.num_iterations == its[1]
    # and for the other solver classes
    for cls in (g.Fcg, g.Bicgstab, g.Gmres):
        s, x = solve_with(gexec, cls, a, b, g.SpdIsai.build())
        assert s.has_converged and s.num_iterations < 1000, cls.__name__
        check_solution(a_host, b, x, 1e-8)


def test_bicgstab_and_gmres_with_general_isai_on_the_convection_matrix(gexec, model_problem):
    _, _, b = model_problem
    rp, ci, v = gr.convection(12)
    n = len(rp) - 1
    a, a_host = g.Csr.from_arrays(gexec, (n, n), rp, ci, v), sp.csr_matrix((v, ci, rp), shape=(n, n))
    assert abs(a_host - a_host.T).max() > 0.1
    for cls in (g.Bicgstab, g.Gmres, g.Cgs):
        f = cls.build().with_criteria(*criteria()).on(gexec).generate(a)
        x = g.Dense.from_numpy(gexec, np.zeros_like(b))
        f.apply(g.Dense.from_numpy(gexec, b), x)
        assert f.has_converged
        for power in (1, 2):
            s, x = solve_with(gexec, cls, a, b, g.GeneralIsai.build().with_sparsity_power(power))
            assert s.has_converged and isinstance(s.get_preconditioner(), g.GeneralIsai), cls.__name__
            print("%s: %d iterations without, %d with GeneralIsai power %d"
                  % (cls.__name__, f.num_iterations, s.num_iterations, power))
            assert s.num_iterations <= f.num_iterations, cls.__name__
            check_solution(a_host, b, x, 1e-8)


def test_multigrid_with_ir_general_isai_smoothers(gexec, model_problem):
    a, a_host, b = model_problem

    def smoother():
        return (g.Ir.build().with_preconditioner(g.GeneralIsai.build()).with_relaxation_factor(0.9)
                .with_criteria(g.stop.Iteration.build().with_max_iters(1)))
    solver = (g.Multigrid.build().with_pre_smoother(smoother()).with_post_smoother(smoother())
              .with_criteria(g.stop.Iteration.build().with_max_iters(100),
                             g.stop.ResidualNorm.build().with_reduction_factor(1e-8))
              .on(gexec).generate(a))
    assert all(isinstance(s, g.Ir) and isinstance(s.get_preconditioner(), g.GeneralIsai)
               for s in solver.pre + solver.post)
    x = g.Dense.from_numpy(gexec, np.full_like(b, 1e30))       # default_initial_guess is zero
    solver.apply(g.Dense.from_numpy(gexec, b), x)
    print("Multigrid with Ir(GeneralIsai) smoothers: %d cycles" % solver.num_iterations)
    assert solver.has_converged and solver.num_iterations < 100
    check_solution(a_host, b, x.to_numpy()[:, 0], 1e-8)
    assert float(solver.residual_norm[0]) <= 1e-8 * np.linalg.norm(b)
    # SpdIsai as the smoother of a preconditioning cycle
    f = g.Multigrid.build().with_criteria(g.stop.Iteration.build().with_max_iters(1)) \
        .with_pre_smoother(g.SpdIsai.build())
    s, x = solve_with(gexec, g.Cg, a, b, f)
    assert s.has_converged
    check_solution(a_host, b, x, 1e-9)
