"""matrix.Permutation, Csr.permute and reorder.ScaledReordered on the device.  Permutations only move values, so
everything is compared bit for bit: against numpy indexing, and for ScaledReordered(Direct) against the chain of
restatements - the permutation of tests/reorder_refs.py, the factors of tests/factorization_refs.py on the pattern
of tests/symbolic_refs.py of the permuted matrix, the two host solves of tests/trs_refs.py and the inverse
permutation.  Multigrid with the reordered direct coarsest solve is measured like
tests/test_multigrid_direct_gpu.py measures the natural one."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import ginkgo_amd as g
import factorization_refs as fr
import pgm_refs as pr
import reorder_refs as rr
import symbolic_refs as sr
import trs_refs as tr
from test_direct_gpu import device_csr, dtype_of, reference_solve
from test_multigrid_direct_gpu import COARSEST_ROWS, MIN_COARSE_ROWS, coarse_factor, direct_factory
from test_pgm_gpu import device_matrix, matrix

pytestmark = pytest.mark.gpu

TYPES = [(np.float64, np.int32), (np.float64, np.int64), (np.float32, np.int32), (np.float32, np.int64)]
TYPE_IDS = ["f64-i32", "f64-i64", "f32-i32", "f32-i64"]
LEAF = 8


def some_permutation(n, seed=11):
    return np.random.default_rng(seed).permutation(n)


# ------------------------------------------------------------------ Permutation
@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
def test_permutation_apply_inverse_compose(gexec, dtype, itype):
    n = 300
    p, q = some_permutation(n), some_permutation(n, 12)
    perm, other = g.Permutation.create(gexec, p, itype), g.Permutation.create(gexec, q, itype)
    assert perm.get_size() == (n, n) and perm.get_permutation_size() == n
    assert perm.get_permutation().cpu().numpy().dtype == itype
    assert np.array_equal(perm.get_permutation().cpu().numpy(), p)
    b = np.random.default_rng(2).uniform(-1, 1, (n, 3)).astype(dtype)
    x = g.Dense.from_numpy(gexec, np.full((n, 3), np.nan, dtype))
    perm.apply(g.Dense.from_numpy(gexec, b), x)
    assert np.array_equal(x.to_numpy(), b[p])
    inv = perm.compute_inverse()
    want_inv = np.empty(n, np.int64)
    want_inv[p] = np.arange(n)
    assert np.array_equal(inv.get_permutation().cpu().numpy(), want_inv)
    back = g.Dense.from_numpy(gexec, np.full((n, 3), np.nan, dtype))
    inv.apply(x, back)
    assert np.array_equal(back.to_numpy(), b)
    # first this, then other
    both = perm.compose(other)
    assert np.array_equal(both.get_permutation().cpu().numpy(), p[q])
    both.apply(g.Dense.from_numpy(gexec, b), x)
    assert np.array_equal(x.to_numpy(), b[p][q])
    # x = alpha P b + beta x: each product and the sum rounded
    x0 = np.random.default_rng(3).uniform(-1, 1, (n, 3)).astype(dtype)
    alpha, beta = dtype(0.75), dtype(-1.5)
    x = g.Dense.from_numpy(gexec, x0)
    perm.apply(g.scalar(gexec, float(alpha), dtype_of(dtype)), g.Dense.from_numpy(gexec, b),
               g.scalar(gexec, float(beta), dtype_of(dtype)), x)
    assert np.array_equal(x.to_numpy(), (alpha * b[p]).astype(dtype) + (beta * x0).astype(dtype))


def test_permutation_create_checks_its_array(gexec):
    for bad in ([0, 1, 1], [0, 1, 3], [-1, 0, 1], [[0, 1]], [0.0, 1.0]):
        with pytest.raises(g.GkoError):
            g.Permutation.create(gexec, np.array(bad))
    with pytest.raises(g.DimensionMismatch):
        g.Permutation.create(gexec, np.arange(3)).compose(g.Permutation.create(gexec, np.arange(4)))


# ------------------------------------------------------------------ Csr.permute
def permuted_by_numpy(a, p, mode):
    a = sp.csr_matrix(a)
    n = len(p)
    inv = np.empty(n, np.int64)
    inv[p] = np.arange(n)
    rows = {"symmetric": p, "rows": p, "columns": None, "inverse_symmetric": inv, "inverse_rows": inv,
            "inverse_columns": None}[mode]
    cols = {"symmetric": p, "rows": None, "columns": p, "inverse_symmetric": inv, "inverse_rows": None,
            "inverse_columns": inv}[mode]
    m = a if rows is None else a[rows]
    m = sp.csr_matrix(m if cols is None else m[:, cols])
    m.sort_indices()
    return m


VALUE_TYPES = TYPES + [(np.complex128, np.int32)]


@pytest.mark.parametrize("dtype,itype", VALUE_TYPES, ids=TYPE_IDS + ["c128-i32"])
def test_csr_permute_every_mode(gexec, dtype, itype):
    a = sr.unsymmetric(120, 0.05, 3).astype(dtype)
    if dtype == np.complex128:
        a = a + 1j * sp.csr_matrix((np.arange(1, a.nnz + 1, dtype=np.float64), a.indices, a.indptr), shape=a.shape)
    a.sort_indices()
    n = a.shape[0]
    p = some_permutation(n)
    dev = g.Csr.from_arrays(gexec, a.shape, a.indptr.astype(itype), a.indices.astype(itype), a.data)
    perm = g.Permutation.create(gexec, p, itype)
    for mode in g.matrix.PERMUTE_MODES:
        got = dev.permute(perm, mode)
        want = permuted_by_numpy(a, p, mode)
        assert got.size == (n, n) and got.row_ptrs.cpu().numpy().dtype == itype
        assert np.array_equal(got.row_ptrs.cpu().numpy(), want.indptr), mode
        assert np.array_equal(got.col_idxs.cpu().numpy(), want.indices), mode
        assert np.array_equal(got.values.cpu().numpy(), want.data), mode
    assert np.array_equal(dev.col_idxs.cpu().numpy(), a.indices) and np.array_equal(dev.values.cpu().numpy(), a.data)
    with pytest.raises(g.GkoError):
        dev.permute(perm, "diagonal")
    with pytest.raises(g.DimensionMismatch):
        dev.permute(g.Permutation.create(gexec, np.arange(n - 1), itype))
    other = np.int64 if itype == np.int32 else np.int32
    with pytest.raises(g.NotSupported):
        dev.permute(g.Permutation.create(gexec, p, other))


# ------------------------------------------------------------------ ScaledReordered(Direct)
@functools.lru_cache(maxsize=None)
def grid(name):
    return {"27p_5": fr.stencil27(5), "5p_20": rr.stencil5(20)}[name]


@functools.lru_cache(maxsize=None)
def chain_of_restatements(name, kind, dtype_name):
    """(perm, the permuted sorted matrix, the reference factors on it, its level count, natural order's)"""
    dtype = np.dtype(dtype_name).type
    a = sp.csr_matrix(grid(name)).astype(dtype)
    perm = rr.nested_dissection(a, LEAF)
    ap = rr.permuted(a, perm)
    rp, ci = sr.lu_pattern(ap, np.int32)
    v = sr.on_filled_pattern(ap, rp, ci, dtype)
    ref = fr.ilu_factors(rp, ci, v) if kind == "lu" else fr.ic_factor(rp, ci, v)
    assert all(np.isfinite(x).all() for x in ref)
    for arr in (perm,) + tuple(ref):
        arr.setflags(write=False)
    return perm, ap, ref, rr.factor_shape(ap)[1], rr.factor_shape(a)[1]


def reordered(inner, leaf=LEAF):
    return g.ScaledReordered.build().with_inner_operator(inner) \
        .with_reordering(g.NestedDissection.build().with_leaf_size(leaf))


@pytest.mark.parametrize("dtype,itype", [(np.float64, np.int32), (np.float32, np.int64)], ids=["f64-i32", "f32-i64"])
@pytest.mark.parametrize("name", ["27p_5", "5p_20"])
@pytest.mark.parametrize("kind", ["cholesky", "lu"])
def test_scaled_reordered_direct_is_the_chain_of_restatements(gexec, kind, name, dtype, itype):
    perm, ap, ref, levels, natural_levels = chain_of_restatements(name, kind, np.dtype(dtype).name)
    a = sp.csr_matrix(grid(name)).astype(dtype)
    n = a.shape[0]
    dev, _ = device_csr(gexec, a, dtype, itype)
    fact = (g.factorization.Lu if kind == "lu" else g.factorization.Cholesky).build()
    solver = reordered(g.Direct.build().with_factorization(fact)).on(gexec).generate(dev)
    # P and the permuted, sorted matrix
    assert np.array_equal(solver.get_permutation().get_permutation().cpu().numpy(), perm)
    pm = solver.get_system_matrix()
    assert np.array_equal(pm.row_ptrs.cpu().numpy(), ap.indptr) and np.array_equal(pm.col_idxs.cpu().numpy(), ap.indices)
    assert np.array_equal(pm.values.cpu().numpy(), ap.data)
    # the factors
    inner = solver.get_inner_operator()
    f = inner.get_factorization()
    got = [t.cpu().numpy() for t in (f.get_l_factor().row_ptrs, f.get_l_factor().col_idxs, f.get_l_factor().values)]
    for x, y in zip(got, ref[:3]):
        assert np.array_equal(x, y)
    # the levels of the lower solve: the restatement's, and fewer than natural order's
    assert inner.get_lower_solver().num_levels == levels < natural_levels
    natural = g.Direct.build().with_factorization(fact).on(gexec).generate(dev)
    assert natural.get_lower_solver().num_levels == natural_levels
    # x, from the two host solves and the inverse permutation
    b = np.random.default_rng(17).uniform(-1, 1, (n, 2)).astype(dtype)
    x = g.Dense.from_numpy(gexec, np.full((n, 2), np.nan, dtype))
    solver.apply(g.Dense.from_numpy(gexec, b), x)
    want = np.empty_like(b)
    want[perm] = reference_solve(kind, ref, b[perm])
    assert np.array_equal(x.to_numpy(), want)
    a64 = a.astype(np.float64)
    assert np.abs(a64 @ want.astype(np.float64) - b).max() <= 64 * n * np.finfo(dtype).eps * np.abs(b).max()
    # x = beta x + alpha solve(b), composed as in Direct
    x0 = np.random.default_rng(5).uniform(-1, 1, (n, 2)).astype(dtype)
    alpha, beta = dtype(0.75), dtype(-1.5)
    x = g.Dense.from_numpy(gexec, x0)
    solver.apply(g.scalar(gexec, float(alpha), dtype_of(dtype)), g.Dense.from_numpy(gexec, b),
                 g.scalar(gexec, float(beta), dtype_of(dtype)), x)
    assert np.array_equal(x.to_numpy(), (beta * x0).astype(dtype) + (alpha * want).astype(dtype))


def test_scalings_are_refused_and_the_parts_are_optional(gexec):
    f = g.ScaledReordered.build().with_row_scaling(None).with_col_scaling(None)
    for setter in (f.with_row_scaling, f.with_col_scaling):
        with pytest.raises(g.NotSupported):
            setter(object())
    a = rr.stencil5(6)
    dev, _ = device_csr(gexec, a, np.float64, np.int32)
    b = np.random.default_rng(1).uniform(-1, 1, (36, 1))
    # no reordering: the identity; no inner operator: x = b
    plain = g.ScaledReordered.build().on(gexec).generate(dev)
    x = g.Dense.from_numpy(gexec, np.zeros((36, 1)))
    plain.apply(g.Dense.from_numpy(gexec, b), x)
    assert np.array_equal(x.to_numpy(), b)
    only_reordered = g.ScaledReordered.build().with_reordering(g.NestedDissection.build().with_leaf_size(4)) \
        .on(gexec).generate(dev)
    only_reordered.apply(g.Dense.from_numpy(gexec, b), x)
    assert np.array_equal(x.to_numpy(), b)
    with pytest.raises(g.NotSupported):
        g.ScaledReordered.build().on(gexec).generate(g.Dense.from_numpy(gexec, np.eye(3)))


def test_an_inner_iterative_solver_starts_from_x(gexec):
    """x' = P x reaches the inner solver: from the exact solution Cg has nothing to do"""
    a = rr.stencil5(12)
    n = a.shape[0]
    dev, _ = device_csr(gexec, a, np.float64, np.int32)
    exact = np.random.default_rng(4).integers(-3, 4, (n, 1)).astype(np.float64)
    b = a @ exact           # small integers: the product is exact, so the residual at `exact` is 0
    cg = g.Cg.build().with_criteria(g.stop.Iteration.build().with_max_iters(100),
                                    g.stop.ResidualNorm.build().with_reduction_factor(1e-8))
    solver = reordered(cg).on(gexec).generate(dev)
    x = g.Dense.from_numpy(gexec, exact)
    solver.apply(g.Dense.from_numpy(gexec, b), x)
    assert solver.get_inner_operator().num_iterations == 0
    assert np.array_equal(x.to_numpy(), exact)
    x = g.Dense.from_numpy(gexec, np.zeros((n, 1)))
    solver.apply(g.Dense.from_numpy(gexec, b), x)
    assert solver.get_inner_operator().num_iterations > 0
    assert np.abs(x.to_numpy() - exact).max() < 1e-6


# ------------------------------------------------------------------ Multigrid with the reordered direct solve
def reordered_factory():
    return reordered(direct_factory())


def permuted_level(level, perm, dtype):
    """the level's operator permuted symmetrically; the values are moved by position, so they keep their type
    (np.longdouble too)"""
    n = len(level["rp"]) - 1
    where = sp.csr_matrix((np.arange(1.0, len(level["ci"]) + 1), level["ci"], level["rp"]), shape=(n, n))
    ap = rr.permuted(where, perm)
    return {"rp": ap.indptr, "ci": ap.indices, "v": np.asarray(level["v"], dtype)[ap.data.astype(np.int64) - 1]}


def v_cycle(levels, perm, factor, b, relax, l=0):
    """the V-cycle of tests/test_multigrid_direct_gpu.py with x = P^T solve(P b) at the bottom"""
    level = levels[l]
    if l == len(levels) - 1:
        lower, upper = factor
        out = np.empty_like(b)
        out[perm] = tr.trs_solve(*upper, tr.trs_solve(*lower, b[perm]), upper=True)
        return out
    x = pr._sweeps(level, b, None, 1, relax)
    r = b - pr.spmv(level["rp"], level["ci"], level["v"], x)
    xc = v_cycle(levels, perm, factor, pr.restrict(level["agg"], level["n_coarse"], r), relax, l + 1)
    x = pr.prolong_add(level["agg"], xc, x)
    return pr._sweeps(level, b, x, 1, relax)


@pytest.mark.parametrize("vt", [np.float64, np.float32], ids=["f64", "f32"])
def test_one_v_cycle_with_the_reordered_direct_coarsest_solve(gexec, vt):
    """the criterion and the bound of tests/test_multigrid_direct_gpu.py: e_ref is the max-norm error of the
    restatement in T against the same cycle in np.longdouble, the device must lie within 4 e_ref of the latter"""
    levels = pr.hierarchy(*pr.triple(matrix("stencil"), vt), vt, min_coarse_rows=MIN_COARSE_ROWS)
    assert [len(lv["rp"]) - 1 for lv in levels] == [1728, 826, COARSEST_ROWS]
    n = 1728
    coarse = levels[-1]
    perm = rr.nested_dissection(sp.csr_matrix((np.ones(len(coarse["ci"])), coarse["ci"], coarse["rp"]),
                                              shape=(COARSEST_ROWS,) * 2), LEAF)
    b = np.random.default_rng(31).uniform(-1, 1, (n, 1)).astype(vt)
    relax = float(np.asarray(0.9, vt))
    x_t = v_cycle(levels, perm, coarse_factor(permuted_level(coarse, perm, vt), vt), b, relax)
    exact = pr.hierarchy(*pr.triple(matrix("stencil"), vt), np.longdouble, min_coarse_rows=MIN_COARSE_ROWS,
                         aggs=[(lv["agg"], lv["n_coarse"]) for lv in levels[:-1]])
    x_l = v_cycle(exact, perm, coarse_factor(permuted_level(exact[-1], perm, np.longdouble), np.longdouble),
                  b.astype(np.longdouble), relax)
    e_ref = float(np.abs(x_t - x_l).max())
    assert e_ref > 0
    mg = (g.Multigrid.build().with_min_coarse_rows(MIN_COARSE_ROWS).with_coarsest_solver(reordered_factory())
          .on(gexec).generate(device_matrix(gexec, "stencil", vt, np.int32)))
    coarsest = mg.get_coarsest_solver()
    assert isinstance(coarsest, g.ScaledReordered) and coarsest.size == (COARSEST_ROWS,) * 2
    assert isinstance(coarsest.get_inner_operator(), g.Direct)
    assert np.array_equal(coarsest.get_permutation().get_permutation().cpu().numpy(), perm)
    assert mg.capturable
    x = g.Dense.from_numpy(gexec, np.full((n, 1), np.nan, vt))
    mg.apply(g.Dense.from_numpy(gexec, b), x)
    e_dev = float(np.abs(x.to_numpy().astype(np.longdouble) - x_l).max())
    print(f"v-cycle, reordered direct coarsest solve, {np.dtype(vt).name}: e_ref {e_ref:.3e} e_dev {e_dev:.3e} "
          f"ratio {e_dev / e_ref:.3f}")
    assert e_dev <= 4 * e_ref, (e_dev, e_ref)


def test_cg_counts_with_and_without_the_reordering(gexec):
    """the coarsest solve is exact up to rounding either way, so CG preconditioned by one V-cycle needs the same
    iterations with the natural-order Direct and with the reordered one"""
    a = device_matrix(gexec, "stencil", np.float64, np.int32)
    a_host = matrix("stencil")
    b = np.random.default_rng(3).uniform(-1, 1, a_host.shape[0])
    counts = {}
    for name, coarsest in (("natural", direct_factory()), ("reordered", reordered_factory())):
        mg = g.Multigrid.build().with_criteria(g.stop.Iteration.build().with_max_iters(1)) \
            .with_min_coarse_rows(MIN_COARSE_ROWS).with_coarsest_solver(coarsest)
        solver = (g.Cg.build().with_criteria(g.stop.Iteration.build().with_max_iters(200),
                                             g.stop.ResidualNorm.build().with_reduction_factor(1e-10))
                  .with_preconditioner(mg).on(gexec).generate(a))
        x = g.Dense.from_numpy(gexec, np.zeros_like(b))
        solver.apply(g.Dense.from_numpy(gexec, b), x)
        assert solver.has_converged, name
        assert np.linalg.norm(a_host @ x.to_numpy()[:, 0] - b) <= 2e-10 * np.linalg.norm(b), name
        counts[name] = solver.num_iterations
    print(f"CG iterations with one V-cycle, coarsest level {COARSEST_ROWS} rows: {counts}")
    assert counts["natural"] == counts["reordered"], counts
