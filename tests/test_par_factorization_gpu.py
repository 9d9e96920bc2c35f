"""ParIlu / ParIc on the device (factorization.ParIlu / ParIc, Ilu / Ic with_factorization) against the numpy
sweeps of tests/par_factorization_refs.py.  Factors are compared with np.array_equal: the sweeps are specified
bit for bit.  At few sweeps the restatement differs from the exact factorization
(tests/test_par_factorization_refs_cpu.py), so no comparison here can pass by way of the exact kernel."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import ginkgo_amd as g
import factorization_refs as fr
import isai_refs as ir
import par_factorization_refs as pr
from test_factorization_gpu import (KINDS, TYPES, TYPE_IDS, criteria, csr_arrays, device_csr, factors_of, same,
                                    shuffled, solve_with, transposed)
from test_factorization_gpu import generate as generate_exact

pytestmark = pytest.mark.gpu

NAMES = ["one", "diagonal", "chain", "stencil", "random"]


# ------------------------------------------------------------------ helpers
def generate(gexec, kind, a, iterations=None, **params):
    f = (g.factorization.ParIlu if kind == "ilu" else g.factorization.ParIc).build()
    if iterations is not None:
        f = f.with_iterations(iterations)
    for k, val in params.items():
        f = getattr(f, "with_" + k)(val)
    return f.on(gexec).generate(a)


@functools.lru_cache(maxsize=None)
def case_matrix(name, spd):
    """a few hundred rows each; symmetric patterns, strictly diagonally dominant values"""
    rng = np.random.default_rng(len(name) * 13 + 5)
    if name == "one":
        return sp.csr_matrix(np.array([[2.0]]))
    if name == "diagonal":
        return sp.diags(rng.uniform(1, 2, 300)).tocsr()
    if name == "chain":
        return fr.from_lower_pattern(fr.chain_pattern(40), rng, spd)
    if name == "stencil":
        return fr.stencil27(6)              # 216 rows of up to 27 entries: several workgroups
    if name == "random":
        return fr.from_lower_pattern(fr.random_pattern(300, rng, 3), rng, spd)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case_levels(name):
    rp, ci, _ = fr.arrays(case_matrix(name, True))
    return pr.num_levels(rp, ci)


_REFS = {}      # {(case, kind, value type): {iterations: (factors, changes)}}, computed once, read-only


def reference(key, kind, a, dtype, counts):
    """{iterations: (the factors as the classes return them, int32 indices; the changes of the last sweep)}"""
    have = _REFS.setdefault((key, kind, dtype), {})
    todo = sorted(set(counts) - set(have))
    if todo:
        rp, ci, v = fr.arrays(a, np.int32, dtype)
        if kind == "ilu":
            for k, (swept, changes) in pr.ilu_sweeps_at(rp, ci, v, todo).items():
                have[k] = (fr.split_l_u(rp, ci, swept), changes)
        else:
            l_rp, l_ci, l_v = fr.split_l(rp, ci, v)
            for k, (swept, changes) in pr.ic_sweeps_at(l_rp, l_ci, l_v, todo).items():
                have[k] = ((l_rp, l_ci, swept), changes)
        for k in todo:
            for arr in have[k][0]:
                arr.setflags(write=False)
    return have


def check_case(gexec, kind, key, a, dtype, itype, counts):
    rp, ci, v = fr.arrays(a, itype, dtype)
    dev = device_csr(gexec, rp, ci, v)
    refs = reference(key, kind, a, dtype, counts)
    for iterations in counts:
        fact = generate(gexec, kind, dev, iterations)
        want, changes = refs[iterations]
        assert all(np.isfinite(x).all() for x in want)
        assert fact.iterations == iterations and fact.get_size() == dev.size
        same(factors_of(kind, fact), want, itype)
        assert fact.last_sweep_changes() == changes, iterations
        assert fact.last_sweep_changes() == changes        # cached
    for got, kept in zip(csr_arrays(dev), (rp, ci, v)):
        assert np.array_equal(got, kept), "generate changed the caller's matrix"
    return dev, refs


# ------------------------------------------------------------------ factors, bit for bit
@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("kind", KINDS)
def test_factors_match_the_sweeps(gexec, kind, name, dtype, itype):
    """1, 2, 3 sweeps (both parities of the ping-pong; no work buffer at 1), as many as the lower solve has
    levels, and one more.  With `levels` sweeps the factors are the exact ones of factorization.Ilu / Ic.

    The last sweep of `levels + 1` changes nothing, ever.  The one of `levels` changes nothing either, with one
    exception the contract itself makes: a row of the first level of ParIc still takes the root of its
    diagonal in sweep 1, so for a matrix of ONE level (the 1 x 1 and the diagonal case) sweep 1 = `levels`
    changes every entry - there the count must be the restatement's, which is the number of entries."""
    a = case_matrix(name, kind == "ic")
    levels = case_levels(name)
    assert levels == {"one": 1, "diagonal": 1, "chain": 40, "stencil": 36}.get(name, levels)
    counts = sorted({1, 2, 3, levels, levels + 1})
    dev, refs = check_case(gexec, kind, name, a, dtype, itype, counts)
    exact = generate_exact(gexec, kind, dev)
    same(factors_of(kind, exact), refs[levels][0], itype)
    same(factors_of(kind, exact), refs[levels + 1][0], itype)
    assert refs[levels + 1][1] == 0
    if kind == "ic" and levels == 1:
        assert refs[levels][1] == a.shape[0]
    else:
        assert refs[levels][1] == 0
    if levels > 3:
        assert refs[1][1] > 0 and refs[3][1] > 0
        assert not np.array_equal(refs[3][0][2], refs[levels][0][2])


def boundary_lengths():
    limits = g.factorization.row_limits()
    assert 1 <= len(limits) <= 4 and limits == sorted(set(limits)) and limits[0] >= 8
    # the first and the last length of every path, and a row that is streamed in three rounds
    return sorted({x for limit in limits for x in (limit, limit + 1)} | {2 * limits[-1] + 22})


@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_hub_rows_at_every_path_boundary(gexec, kind, dtype, itype):
    """the kernel picks its path from the LONGEST row, so every length gets a matrix of its own in which one
    hub row has exactly that many entries (ic: in its lower triangle) and no other more than 4"""
    lengths = boundary_lengths()
    assert max(lengths) > 2 * 64 and len(lengths) >= 3
    for length in lengths:
        if kind == "ilu":
            n_lower = (length - 1) // 2
            n_upper = length - 1 - n_lower
        else:
            n_lower, n_upper = length - 1, 2
        n, hub = n_lower + n_upper + 60, n_lower + 20
        a = fr.from_lower_pattern(fr.hub_pattern(n, hub, n_lower, n_upper), np.random.default_rng(length), kind == "ic")
        stored = np.diff((sp.tril(a, format="csr") if kind == "ic" else a).indptr)
        assert stored.max() == stored[hub] == length and np.sort(stored)[-2] <= 4
        _, refs = check_case(gexec, kind, "hub%d" % length, a, dtype, itype, (3,))
        assert refs[3][1] > 0


# ------------------------------------------------------------------ preparation
@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
def test_missing_diagonals_become_explicit_zeros(gexec, dtype, itype):
    """rows 5, 57 and 199 lose their diagonal entry (as in test_factorization_gpu).  ILU: sweep 1 divides by the
    explicit zeros, so after 3 sweeps inf / NaN sit where the restatement has them - and because an entry is a
    function of the input and the previous sweep alone (no "write only if finite"), they are gone once the
    sweeps reach the number of levels: the exact factors, which are finite.  IC: the pivot is the root of a
    negative number and the NaNs are where the restatement has them."""
    a = case_matrix("random", True)
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
    ref, _ = pr.par_ilu_factors(rp, ci, zeroed, 3)
    assert not np.isfinite(ref[2]).all() and not np.isfinite(ref[5]).all()
    same(factors_of("ilu", generate(gexec, "ilu", dev, 3)), ref, itype, equal_nan=True)
    exact = fr.ilu_factors(rp, ci, zeroed)
    assert all(np.isfinite(x).all() for x in exact)
    healed = generate(gexec, "ilu", dev, pr.num_levels(rp, ci))
    same(factors_of("ilu", healed), exact, itype)
    assert healed.last_sweep_changes() == 0
    ref, _ = pr.par_ic_factor(rp, ci, zeroed, 3)
    assert np.isnan(ref[2]).any()
    same(factors_of("ic", generate(gexec, "ic", dev, 3)), ref, itype, equal_nan=True)
    assert np.array_equal(dev.values.cpu().numpy(), v[~gone]), "generate changed the caller's matrix"


@pytest.mark.parametrize("kind", KINDS)
def test_unsorted_input_is_sorted_unless_told_not_to(gexec, kind):
    a = case_matrix("random", kind == "ic")
    rp, ci, v = fr.arrays(a)
    ref = reference("random", kind, a, np.float64, (2,))[2][0]
    ci_u, v_u = shuffled(rp, ci, v, np.random.default_rng(8))
    assert not np.array_equal(ci_u, ci)
    dev = device_csr(gexec, rp, ci_u, v_u)
    same(factors_of(kind, generate(gexec, kind, dev, 2)), ref, np.int32)
    assert np.array_equal(dev.col_idxs.cpu().numpy(), ci_u) and np.array_equal(dev.values.cpu().numpy(), v_u), \
        "generate changed the caller's matrix"
    # sorted input and skip_sorting: the same factors
    same(factors_of(kind, generate(gexec, kind, device_csr(gexec, rp, ci, v), 2, skip_sorting=True)), ref, np.int32)
    if kind == "ilu":
        # skip_sorting on rows whose UPPER entries are out of order: U keeps the storage order, so nothing
        # was sorted
        ci_u, v_u = shuffled(rp, ci, v, np.random.default_rng(9), upper_only=True)
        got = factors_of(kind, generate(gexec, kind, device_csr(gexec, rp, ci_u, v_u), 2, skip_sorting=True))
        assert np.array_equal(got[4], fr.split_l_u(rp, ci_u, v_u)[4]) and not np.array_equal(got[4], ref[4])


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
        f1, f2 = generate(gexec, kind, fb, 2), generate(gexec, kind, csr, 2)
        want = (pr.par_ilu_factors if kind == "ilu" else pr.par_ic_factor)(*fr.arrays(a), 2)[0]
        for p, q, r in zip(factors_of(kind, f1), factors_of(kind, f2), want):
            assert p.size and np.array_equal(p, q) and np.array_equal(p, r) and np.isfinite(p).all()
        factory = (g.factorization.ParIlu if kind == "ilu" else g.factorization.ParIc).build().with_iterations(2)
        m = (g.Ilu if kind == "ilu" else g.Ic).build().with_factorization(factory).on(gexec).generate(fb)
        for p, q in zip(factors_of(kind, m.factorization), factors_of(kind, f2)):
            assert np.array_equal(p, q)


@pytest.mark.parametrize("kind", KINDS)
def test_zero_iterations_mean_the_default_and_negative_ones_are_refused(gexec, kind):
    sweeps = g.factorization.DEFAULT_SWEEPS
    assert sweeps == 5
    a = case_matrix("random", kind == "ic")
    dev = device_csr(gexec, *fr.arrays(a))
    want, changes = reference("random", kind, a, np.float64, (sweeps,))[sweeps]
    for fact in (generate(gexec, kind, dev, 0), generate(gexec, kind, dev)):
        assert fact.iterations == sweeps
        same(factors_of(kind, fact), want, np.int32)
        assert fact.last_sweep_changes() == changes
    cls = g.factorization.ParIlu if kind == "ilu" else g.factorization.ParIc
    with pytest.raises(g.GkoError):
        cls.build().with_iterations(-1)
    if kind == "ic":
        both = generate(gexec, kind, dev, 2, both_factors=True)
        same(csr_arrays(both.get_lt_factor()), transposed(*csr_arrays(both.get_l_factor())), np.int32)
        assert generate(gexec, kind, dev, 2, both_factors=False).get_lt_factor() is None


def test_the_classes_refuse_what_ilu_and_ic_refuse(gexec):
    dev = device_csr(gexec, *fr.arrays(case_matrix("chain", True)))
    for cls in (g.factorization.ParIlu, g.factorization.ParIc):
        with pytest.raises(g.NotSupported):
            cls.build().on(gexec).generate(g.Dense.create(gexec, (4, 4)))
        with pytest.raises(g.NotSupported):
            cls.build().on(gexec).generate(dev.convert_to_ell())
        wide = g.Csr.from_arrays(gexec, (2, 3), np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32), np.ones(2))
        with pytest.raises(g.DimensionMismatch):
            cls.build().on(gexec).generate(wide)
        cplx = g.Csr.from_arrays(gexec, (2, 2), np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32),
                                 np.ones(2, np.complex128))
        with pytest.raises(g.NotSupported):
            cls.build().on(gexec).generate(cplx)
    # a preconditioner does not take the other kind's factorization
    with pytest.raises(g.NotSupported):
        g.Ic.build().with_factorization(g.factorization.ParIlu.build()).on(gexec).generate(dev)


# ------------------------------------------------------------------ the raw entries
def test_invalid_arguments_are_refused_before_a_value_is_touched(gexec):
    from ginkgo_amd._lib import call
    st = gexec.stream
    a = case_matrix("random", False)
    rp, ci, v = fr.arrays(a)
    low = fr.arrays(sp.tril(a, format="csr"))
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))

    def dev(*arrays):
        return [gexec.to_device(np.array(x)) for x in arrays]

    def without_diagonal(rp_, ci_, v_, row):
        rows_ = np.repeat(np.arange(n), np.diff(rp_))
        keep = ~((rows_ == row) & (ci_ == row))
        out = np.zeros_like(rp_)
        out[1:] = np.cumsum(np.bincount(rows_[keep], minlength=n))
        return out, ci_[keep], v_[keep]

    ci_out, ci_neg = ci.copy(), ci.copy()
    ci_out[rp[100]], ci_neg[rp[100]] = n, -1
    rp_bad, rp_first = rp.copy(), rp.copy()
    assert rp[11] > rp[10]
    rp_bad[10], rp_bad[11] = rp[11], rp[10]
    rp_first[0] = 1
    extra = sp.tril(a, format="lil")
    extra[57, 58] = 0.25
    full, tri = dev(rp, ci, v), dev(*low)
    nnz, nnz_low = len(ci), len(low[1])
    out = gexec.to_device(np.full(nnz + 1, 9.0))
    work = gexec.to_device(np.full(nnz + 1, 9.0))
    changed = gexec.to_device(np.array([77], np.int64))
    ilu, ic = "gkoc_par_ilu_sweeps_f64_i32", "gkoc_par_ic_sweeps_f64_i32"
    missing, missing_low = dev(*without_diagonal(rp, ci, v, 57)), dev(*without_diagonal(*low, 57))
    bad = [("no sweep", ilu, n, nnz, full, 0, work, out),
           ("a negative number of sweeps", ic, n, nnz_low, tri, -1, work, out),
           ("a negative size", ilu, -1, nnz, full, 2, work, out),
           ("no row pointers", ilu, n, nnz, [None] + full[1:], 2, work, out),
           ("no columns", ic, n, nnz_low, [tri[0], None, tri[2]], 2, work, out),
           ("no values", ilu, n, nnz, full[:2] + [None], 2, work, out),
           ("no output", ilu, n, nnz, full, 2, work, None),
           ("no work buffer for two sweeps", ilu, n, nnz, full, 2, None, out),
           ("no work buffer for three sweeps", ic, n, nnz_low, tri, 3, None, out),
           ("work is the output", ilu, n, nnz, full, 2, out, out),
           ("work is the input", ilu, n, nnz, full, 2, full[2], out),
           ("the output is the input", ic, n, nnz_low, tri, 1, None, tri[2]),
           ("work overlaps the output", ilu, n, nnz, full, 2, out[1:], out),
           ("row pointers that descend", ilu, n, nnz, dev(rp_bad, ci, v), 2, work, out),
           ("row pointers that start at 1", ilu, n, nnz, dev(rp_first, ci, v), 2, work, out),
           ("row pointers that do not end at nnz", ilu, n, nnz - 1, full, 2, work, out),
           ("a column out of range", ilu, n, nnz, dev(rp, ci_out, v), 2, work, out),
           ("a negative column", ilu, n, nnz, dev(rp, ci_neg, v), 2, work, out),
           ("a row without its diagonal", ilu, n, nnz - 1, missing, 2, work, out),
           ("a row without its diagonal", ic, n, nnz_low - 1, missing_low, 2, work, out),
           ("a diagonal that is not last", ic, n, nnz_low + 1, dev(*fr.arrays(extra.tocsr())), 2, work, out),
           ("a full matrix for ic", ic, n, nnz, full, 2, work, out)]
    for what, name, n_, nnz_, m, iterations, work_, out_ in bad:
        kept = m[2].cpu().numpy().copy() if m[2] is not None else None
        with pytest.raises(g.GkoError):
            call(name, st, n_, nnz_, *m, iterations, work_, out_, changed)
        if kept is not None:
            assert np.array_equal(m[2].cpu().numpy(), kept), what + ": the input was written"
        if out_ is out:
            assert (out.cpu().numpy() == 9.0).all(), what + ": out_vals was written before the refusal"
        if work_ is work:
            assert (work.cpu().numpy() == 9.0).all(), what + ": work was written before the refusal"
    # nothing of the above reached the device: valid calls on the same arrays are right; the counter and the
    # work buffer are optional
    want, count = pr.ilu_sweeps(rp, ci, v, 2)
    call(ilu, st, n, nnz, *full, 2, work, out, changed)
    assert np.array_equal(out.cpu().numpy()[:nnz], want) and int(changed.item()) == count > 0
    assert out.cpu().numpy()[nnz] == 9.0 and work.cpu().numpy()[nnz] == 9.0
    assert np.array_equal(work.cpu().numpy()[:nnz], pr.ilu_sweeps(rp, ci, v, 1)[0])
    assert np.array_equal(full[2].cpu().numpy(), v)
    want, count = pr.ic_sweeps(*low, 1)
    changed.fill_(77)
    call(ic, st, n, nnz_low, *tri, 1, None, out, None)
    assert np.array_equal(out.cpu().numpy()[:nnz_low], want) and int(changed.item()) == 77
    call(ic, st, n, nnz_low, *tri, 1, None, out, changed)
    assert int(changed.item()) == count > 0
    # no rows: nothing to do
    call(ilu, st, 0, 0, None, None, None, 1, None, None, None)
    call(ic, st, 0, 0, None, None, None, 3, None, None, changed)
    assert int(changed.item()) == 0


@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_a_zero_pivot_gives_the_restatement_s_non_finite_entries(gexec, kind, dtype, itype):
    from ginkgo_amd._lib import IT, VT, call
    a = case_matrix("random", kind == "ic")
    rp, ci, v = fr.arrays(sp.tril(a, format="csr") if kind == "ic" else a, itype, dtype)
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    v[(rows == ci) & np.isin(rows, (0, 3))] = 0
    want, _ = (pr.ilu_sweeps if kind == "ilu" else pr.ic_sweeps)(rp, ci, v, 3)
    assert np.isinf(want).any() or np.isnan(want).any()
    assert np.isfinite(want).any()
    m = device_csr(gexec, rp, ci, v)
    out, work = gexec.to_device(np.zeros_like(v)), gexec.to_device(np.zeros_like(v))
    call("gkoc_par_%s_sweeps_%s_%s" % (kind, VT[m.dtype], IT[m.col_idxs.dtype]), gexec.stream, n, len(ci),
         m.row_ptrs, m.col_idxs, m.values, 3, work, out, None)
    assert np.array_equal(out.cpu().numpy(), want, equal_nan=True)
    # the call succeeded; the next one on this executor is right
    check_case(gexec, kind, "random", a, dtype, itype, (2,))


# ------------------------------------------------------------------ no schedule
def entries_of(fn):
    """the names of the library's entries that fn() calls"""
    from ginkgo_amd._lib import record
    with record() as tape:
        fn()
    return [name for _, _, name in tape.calls]


def test_no_level_schedule_is_built(gexec):
    dev = device_csr(gexec, *fr.arrays(case_matrix("stencil", True)))
    par_ilu = lambda: g.factorization.ParIlu.build().with_iterations(3)     # noqa: E731
    par_ic = lambda: g.factorization.ParIc.build().with_iterations(3)       # noqa: E731
    runs = {
        "ParIlu": lambda: par_ilu().on(gexec).generate(dev),
        "ParIc": lambda: par_ic().on(gexec).generate(dev),
        "Ilu": lambda: g.Ilu.build().with_factorization(par_ilu()).with_l_solver(g.LowerIsai.build())
        .with_u_solver(g.UpperIsai.build()).on(gexec).generate(dev),
        "Ic": lambda: g.Ic.build().with_factorization(par_ic()).with_l_solver(g.LowerIsai.build())
        .on(gexec).generate(dev),
    }
    for what, fn in runs.items():
        names = entries_of(fn)
        stem = "gkoc_par_ilu_sweeps_" if "Ilu" in what else "gkoc_par_ic_sweeps_"
        assert sum(name.startswith(stem) for name in names) == 1, what
        assert not [name for name in names if "trs_generate" in name or "_factorize_" in name], what
    # the defaults are untouched: without with_factorization the exact factorization, on its schedule
    for cls, stem in ((g.Ilu, "gkoc_ilu_factorize_"), (g.Ic, "gkoc_ic_factorize_")):
        names = entries_of(lambda: cls.build().with_l_solver(g.LowerIsai.build()).on(gexec).generate(dev))
        assert any(name.startswith(stem) for name in names) and any("trs_generate" in name for name in names)
        assert not [name for name in names if "_sweeps_" in name]
        m = cls.build().on(gexec).generate(dev)
        assert type(m.factorization) is (g.factorization.Ilu if cls is g.Ilu else g.factorization.Ic)
    # skip_sorting of the preconditioner is not passed on to a given factory
    rp, ci, v = fr.arrays(case_matrix("stencil", True))
    ci_u, v_u = shuffled(rp, ci, v, np.random.default_rng(8))
    m = g.Ilu.build().with_skip_sorting(True).with_factorization(par_ilu()).on(gexec) \
        .generate(device_csr(gexec, rp, ci_u, v_u))
    same(factors_of("ilu", m.factorization), reference("stencil", "ilu", case_matrix("stencil", True), np.float64,
                                                         (3,))[3][0], np.int32)


# ------------------------------------------------------------------ the solvers
GRID = 12
# A = 27 I - T x T x T with T = tridiag(1, 1, 1): the smallest eigenvalue is 27 - (1 + 2 cos(pi / (GRID + 1)))^3
LAMBDA_MIN = 27.0 - (1.0 + 2.0 * np.cos(np.pi / (GRID + 1))) ** 3
REDUCTION = 1e-10


def host_pcg(a, b, precond):
    """preconditioned CG, x_0 = 0; stops, like the device solver, before the iteration in which
    ||r|| <= REDUCTION * ||r_0|| is seen.  Returns (x, iterations)."""
    x = np.zeros_like(b)
    r = b.copy()
    z = precond(r)
    p = z.copy()
    rho = r @ z
    stop = REDUCTION * np.linalg.norm(r)
    its = 0
    while np.linalg.norm(r) > stop and its < 1000:
        q = a @ p
        alpha = rho / (p @ q)
        x += alpha * p
        r -= alpha * q
        its += 1
        z = precond(r)
        rho, rho_old = r @ z, rho
        p = z + (rho / rho_old) * p
    return x, its


def host_bicgstab(a, b, precond):
    """the loop of ginkgo_amd.krylov.Bicgstab (core/solver/bicgstab.cpp), x_0 = 0: the criterion is checked
    on r at the head of an iteration and on s in its middle; a stop in the middle does not count the iteration"""
    x = np.zeros_like(b)
    r = b.copy()
    rr = r.copy()
    p, v = np.zeros_like(b), np.zeros_like(b)
    prev_rho = alpha = omega = 1.0
    stop = REDUCTION * np.linalg.norm(r)
    it = -1
    while it < 1000:
        it += 1
        rho = rr @ r
        if np.linalg.norm(r) <= stop:
            break
        p = r + (rho / prev_rho * alpha / omega) * (p - omega * v)
        y = precond(p)
        v = a @ y
        alpha = rho / (rr @ v)
        s = r - alpha * v
        if np.linalg.norm(s) <= stop:
            x += alpha * y
            break
        z = precond(s)
        t = a @ z
        omega = (s @ t) / (t @ t)
        x += alpha * y + omega * z
        r = s - omega * t
        prev_rho = rho
    return x, it


@pytest.fixture(scope="module")
def stencil_problem(gexec):
    a_host = fr.stencil27(GRID)
    rp, ci, v = fr.arrays(a_host)
    return device_csr(gexec, rp, ci, v), a_host, (rp, ci, v), np.ones(GRID ** 3)


def csr_of(rp, ci, v):
    n = len(rp) - 1
    return sp.csr_matrix((v, ci, rp), shape=(n, n))


def host_preconditioners(kind, arrays):
    """{inner solver: r -> M^-1 r on the host} with the restatement's 3-sweep factors: exact triangular
    solves for the default pair, the reference W of tests/isai_refs.py for the ISAI solvers"""
    if kind == "ic":
        (l_rp, l_ci, l_v), _ = pr.par_ic_factor(*arrays, 3)
        lower = csr_of(l_rp, l_ci, l_v)
        upper = lower.T.tocsr()
        w = csr_of(l_rp, l_ci, ir.tri_inverse(l_rp, l_ci, l_v, l_rp, l_ci, True))
        wt = w.T.tocsr()
        return {"trs": lambda r: spla.spsolve_triangular(upper, spla.spsolve_triangular(lower, r, lower=True),
                                                         lower=False),
                "isai": lambda r: wt @ (w @ r)}
    (l_rp, l_ci, l_v, u_rp, u_ci, u_v), _ = pr.par_ilu_factors(*arrays, 3)
    lower, upper = csr_of(l_rp, l_ci, l_v), csr_of(u_rp, u_ci, u_v)
    w_l = csr_of(l_rp, l_ci, ir.tri_inverse(l_rp, l_ci, l_v, l_rp, l_ci, True))
    w_u = csr_of(u_rp, u_ci, ir.tri_inverse(u_rp, u_ci, u_v, u_rp, u_ci, False))
    return {"trs": lambda r: spla.spsolve_triangular(upper, spla.spsolve_triangular(lower, r, lower=True),
                                                     lower=False),
            "isai": lambda r: w_u @ (w_l @ r)}


def device_preconditioner(kind, inner):
    if kind == "ic":
        f = g.Ic.build().with_factorization(g.factorization.ParIc.build().with_iterations(3))
        return f.with_l_solver(g.LowerIsai.build()) if inner == "isai" else f
    f = g.Ilu.build().with_factorization(g.factorization.ParIlu.build().with_iterations(3))
    return f.with_l_solver(g.LowerIsai.build()).with_u_solver(g.UpperIsai.build()) if inner == "isai" else f


@pytest.mark.parametrize("inner", ["trs", "isai"])
@pytest.mark.parametrize("kind", ["ic", "ilu"])
def test_solvers_with_three_sweeps_match_the_host(gexec, stencil_problem, kind, inner):
    """Cg with Ic + ParIc(3), Bicgstab with Ilu + ParIlu(3), with the level-scheduled solvers and with ISAI,
    against the same iteration on the host with the restatement's factors.

    Both sides stop at ||r|| <= 1e-10 ||b||, so x_dev - x_host = A^-1 (r_host - r_dev) is at most
    2e-10 ||b|| / lambda_min(A) long (plus rounding far below that: 2.1e-10 is asserted).  The iteration
    counts agree within one: tests/test_isai_gpu.py pins no count for this matrix by equality."""
    a, a_host, arrays, b = stencil_problem
    solver_cls, host = (g.Cg, host_pcg) if kind == "ic" else (g.Bicgstab, host_bicgstab)
    x_host, its_host = host(a_host, b, host_preconditioners(kind, arrays)[inner])
    s, x = solve_with(gexec, solver_cls, a, b, device_preconditioner(kind, inner))
    m = s.get_preconditioner()
    assert isinstance(m.factorization, g.factorization.ParIc if kind == "ic" else g.factorization.ParIlu)
    assert m.factorization.iterations == 3
    assert isinstance(m.get_l_solver(), g.LowerIsai if inner == "isai" else g.LowerTrs)
    print("%s + Par%s(3) + %s: device %d iterations, host %d" % (solver_cls.__name__, kind.capitalize(), inner,
                                                               s.num_iterations, its_host))
    assert s.has_converged and abs(s.num_iterations - its_host) <= 1
    assert np.linalg.norm(b - a_host @ x) <= 1.01 * REDUCTION * np.linalg.norm(b)
    assert np.linalg.norm(x - x_host) <= 2.1 * REDUCTION * np.linalg.norm(b) / LAMBDA_MIN
    if kind == "ic":
        # a ready ParIc object gives the same x as the factory route
        fact = g.factorization.ParIc.build().with_iterations(3).on(gexec).generate(a)
        f = g.Ic.build().with_l_solver(g.LowerIsai.build()) if inner == "isai" else g.Ic.build()
        ready = f.on(gexec).generate(fact)
        assert ready.factorization is fact
        solver = g.Cg.build().with_criteria(*criteria()).with_generated_preconditioner(ready).on(gexec).generate(a)
        x2 = g.Dense.from_numpy(gexec, np.zeros_like(b))
        solver.apply(g.Dense.from_numpy(gexec, b), x2)
        assert solver.num_iterations == s.num_iterations and np.array_equal(x2.to_numpy()[:, 0], x)
