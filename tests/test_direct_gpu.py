"""The direct factorizations and the direct solver on the device (factorization.Lu / Cholesky, solver Direct)
against the numpy loops of tests/factorization_refs.py and tests/trs_refs.py run on the filled pattern of
tests/symbolic_refs.py.  Factors and solves are compared with np.array_equal; that the factorization is EXACT -
what separates it from ILU(0) / IC(0) - is the standard componentwise backward-error bound."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import ginkgo_amd as g
import factorization_refs as fr
import symbolic_refs as sr
import trs_refs as tr

pytestmark = pytest.mark.gpu

TYPES = [(np.float64, np.int32), (np.float64, np.int64), (np.float32, np.int32), (np.float32, np.int64)]
TYPE_IDS = ["f64-i32", "f64-i64", "f32-i32", "f32-i64"]
KINDS = ["lu", "cholesky"]
SHAPES = ["one", "blocks", "chain200", "arrow_first70", "arrow_last70", "stencil5", "random300"]


def csr_arrays(m):
    return [t.cpu().numpy() for t in (m.row_ptrs, m.col_idxs, m.values)]


@functools.lru_cache(maxsize=None)
def case_matrix(name, spd):
    """strictly diagonally dominant matrices on the shapes of tests/test_symbolic_gpu.py: symmetric values with
    spd, independent ones in the two triangles without"""
    rng = np.random.default_rng(len(name) * 7 + 1)
    lower = {
        "one": lambda: [[]],
        "blocks": lambda: sr.blocks(sr.arrow_first(6), fr.chain_pattern(5)),
        "chain200": lambda: fr.chain_pattern(200),
        "arrow_first70": lambda: sr.arrow_first(70),
        "arrow_last70": lambda: sr.arrow_last(70),
        "stencil5": lambda: sr.lower_rows(sr.symmetrized(fr.stencil27(5))),
        "random300": lambda: fr.random_pattern(300, rng, deps=3),
    }[name]()
    return fr.from_lower_pattern(lower, rng, spd)


_REFS = {}      # reference factors, computed once per (case, kind, value type) and left unchanged


def reference(kind, name, a, dtype):
    """lu: (l_rp, l_ci, l_v, u_rp, u_ci, u_v); cholesky: (l_rp, l_ci, l_v) - index arrays in int32"""
    key = (kind, name, np.dtype(dtype).name)
    if key not in _REFS:
        rp, ci = sr.lu_pattern(a, np.int32)
        v = sr.on_filled_pattern(a, rp, ci, dtype)
        _REFS[key] = fr.ilu_factors(rp, ci, v) if kind == "lu" else fr.ic_factor(rp, ci, v)
        for arr in _REFS[key]:
            arr.setflags(write=False)
        assert all(np.isfinite(x).all() for x in _REFS[key])
    return _REFS[key]


def factory(kind):
    return (g.factorization.Lu if kind == "lu" else g.factorization.Cholesky).build()


def device_csr(gexec, a, dtype, itype):
    rp, ci, v = fr.arrays(a, itype, dtype)
    return g.Csr.from_arrays(gexec, a.shape, rp, ci, v), (rp, ci, v)


def factors_of(kind, fact):
    if kind == "lu":
        return csr_arrays(fact.get_l_factor()) + csr_arrays(fact.get_u_factor())
    return csr_arrays(fact.get_l_factor())


def same(got, want, itype):
    assert len(got) == len(want)
    for p, q in zip(got, want):
        q = q.astype(itype) if q.dtype.kind == "i" else q
        assert p.dtype == q.dtype and p.shape == q.shape
        assert np.array_equal(p, q)


# ------------------------------------------------------------------ factors, bit for bit
@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_factors_match_reference(gexec, kind, name, dtype, itype):
    a = case_matrix(name, kind == "cholesky")
    dev, kept = device_csr(gexec, a, dtype, itype)
    fact = factory(kind).on(gexec).generate(dev)
    for got, was in zip(csr_arrays(dev), kept):
        assert np.array_equal(got, was), "generate changed the caller's matrix"
    same(factors_of(kind, fact), reference(kind, name, a, dtype), itype)
    if kind == "cholesky":
        lt = fact.get_lt_factor()
        l_rp, l_ci, l_v = reference(kind, name, a, dtype)
        want = sp.csr_matrix((l_v, l_ci, l_rp), shape=a.shape).T.tocsr()
        want.sort_indices()
        same(csr_arrays(lt), [want.indptr, want.indices, want.data], itype)
    else:
        l_rp, l_ci, l_v, u_rp, u_ci, u_v = reference(kind, name, a, dtype)
        combined = fact.get_combined()
        want_rp, want_ci = sr.lu_pattern(a, itype)
        assert np.array_equal(combined.row_ptrs.cpu().numpy(), want_rp)
        assert np.array_equal(combined.col_idxs.cpu().numpy(), want_ci)


def test_unsorted_input_and_the_algorithm_names(gexec):
    a = case_matrix("stencil5", False)
    rp, ci, v = fr.arrays(a, np.int32, np.float64)
    for i in range(len(rp) - 1):            # reverse every row
        ci[rp[i]:rp[i + 1]] = ci[rp[i]:rp[i + 1]][::-1].copy()
        v[rp[i]:rp[i + 1]] = v[rp[i]:rp[i + 1]][::-1].copy()
    want = reference("lu", "stencil5", a, np.float64)
    for algorithm in ("general", "near_symmetric", "symmetric"):
        dev = g.Csr.from_arrays(gexec, a.shape, rp, ci, v)
        fact = g.factorization.Lu.build().with_symbolic_algorithm(algorithm).on(gexec).generate(dev)
        same(factors_of("lu", fact), want, np.int32)
        assert np.array_equal(dev.col_idxs.cpu().numpy(), ci)
    with pytest.raises(g.GkoError):
        g.factorization.Lu.build().with_symbolic_algorithm("nested_dissection")
    fb = g.Csr.from_arrays(gexec, a.shape, *fr.arrays(a, np.int32, np.float64)).convert_to_fbcsr(1)
    same(factors_of("lu", g.factorization.Lu.build().on(gexec).generate(fb)), want, np.int32)


def test_an_unsymmetric_pattern_gets_exact_zeros(gexec):
    """the symmetrised pattern is a superset of the true LU fill: what it adds comes out as exact zeros, and the
    product is A"""
    rng = np.random.default_rng(9)
    lower = fr.random_pattern(60, rng, deps=2)
    a = fr.from_lower_pattern(lower, rng, False).tolil()
    for i in range(10, 60, 3):              # drop upper entries: the pattern is unsymmetric now
        for j in lower[i][:1]:
            a[j, i] = 0
    a = a.tocsr()
    a.eliminate_zeros()
    assert (abs(a) > 0).astype(int).T.tocsr().toarray().tolist() != (abs(a) > 0).astype(int).toarray().tolist()
    dev, _ = device_csr(gexec, a, np.float64, np.int32)
    fact = g.factorization.Lu.build().on(gexec).generate(dev)
    rp, ci = sr.lu_pattern(a, np.int32)
    same(factors_of("lu", fact), fr.ilu_factors(rp, ci, sr.on_filled_pattern(a, rp, ci, np.float64)), np.int32)
    l, u = (fr.dense_of(*csr_arrays(m)) for m in (fact.get_l_factor(), fact.get_u_factor()))
    n = a.shape[0]
    gamma = n * 2.0 ** -53 / (1 - n * 2.0 ** -53)
    assert (np.abs(a.toarray() - l @ u) <= gamma * (np.abs(l) @ np.abs(u))).all()
    # the true fill of the unsymmetric pattern by boolean elimination; what the combined pattern adds is zero
    fill = a.toarray() != 0
    for k in range(n):
        below = np.nonzero(fill[k + 1:, k])[0] + k + 1
        fill[np.ix_(below, np.nonzero(fill[k, k + 1:])[0] + k + 1)] = True
    added = (fr.dense_of(rp, ci, np.ones(len(ci))) != 0) & ~fill
    assert added.any() and ((l + u)[added] == 0).all()


# ------------------------------------------------------------------ exactness
def backward_error_holds(a_dense, left, right, dtype):
    """|A - L R| <= gamma_n |L| |R| componentwise, gamma_n = n u / (1 - n u): the LU / Cholesky backward-error
    bound (Higham, Accuracy and Stability of Numerical Algorithms, Theorems 9.3 and 10.3); products in float64"""
    n = a_dense.shape[0]
    u = float(np.finfo(dtype).eps) / 2
    gamma = n * u / (1 - n * u)
    left, right = left.astype(np.float64), right.astype(np.float64)
    err = np.abs(a_dense.astype(np.float64) - left @ right)
    bound = gamma * (np.abs(left) @ np.abs(right))
    worst = float((err / np.where(bound > 0, bound, 1.0))[bound > 0].max())
    return bool((err <= bound).all()), worst


@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("name", ["stencil5", "random300"])
@pytest.mark.parametrize("kind", KINDS)
def test_the_factorization_is_exact_where_the_incomplete_one_is_not(gexec, kind, name, dtype, itype):
    a = fr.stencil27(5) if name == "stencil5" else case_matrix(name, kind == "cholesky")
    dev, (rp, ci, v) = device_csr(gexec, a, dtype, itype)
    a_dense = fr.dense_of(rp, ci, v)                # A as the value type holds it
    if kind == "lu":
        direct = g.factorization.Lu.build().on(gexec).generate(dev)
        incomplete = g.factorization.Ilu.build().on(gexec).generate(dev)
        pairs = [(fr.dense_of(*csr_arrays(f.get_l_factor())), fr.dense_of(*csr_arrays(f.get_u_factor())))
                 for f in (direct, incomplete)]
    else:
        direct = g.factorization.Cholesky.build().on(gexec).generate(dev)
        incomplete = g.factorization.Ic.build().on(gexec).generate(dev)
        pairs = [(fr.dense_of(*csr_arrays(f.get_l_factor())), fr.dense_of(*csr_arrays(f.get_lt_factor())))
                 for f in (direct, incomplete)]
    holds, worst = backward_error_holds(a_dense, *pairs[0], dtype)
    fails, worst_incomplete = backward_error_holds(a_dense, *pairs[1], dtype)
    print(f"{kind} {name} {np.dtype(dtype).name}: |A - L R| / (gamma_n |L||R|) max {worst:.3e} direct, "
          f"{worst_incomplete:.3e} incomplete")
    assert holds, worst
    assert not fails, "the incomplete factorization satisfies the bound too: the test cannot fail"


# ------------------------------------------------------------------ the given pattern
@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
def test_the_matrix_own_pattern_gives_the_incomplete_factors(gexec, dtype, itype):
    for kind, incomplete in (("lu", g.factorization.Ilu), ("cholesky", g.factorization.Ic)):
        a = case_matrix("stencil5", kind == "cholesky")
        dev, _ = device_csr(gexec, a, dtype, itype)
        given = factory(kind).with_symbolic_factorization(dev).on(gexec).generate(dev)
        same(factors_of(kind, given), factors_of(kind, incomplete.build().on(gexec).generate(dev)), itype)
        rp, ci, v = fr.arrays(a, np.int32, dtype)
        same(factors_of(kind, given), fr.ilu_factors(rp, ci, v) if kind == "lu" else fr.ic_factor(rp, ci, v), itype)


def test_a_given_pattern_is_checked(gexec):
    a = case_matrix("blocks", False)
    dev, (rp, ci, v) = device_csr(gexec, a, np.float64, np.int32)
    other, _ = device_csr(gexec, case_matrix("arrow_first70", False), np.float64, np.int32)
    with pytest.raises(g.DimensionMismatch):
        g.factorization.Lu.build().with_symbolic_factorization(other).on(gexec).generate(dev)
    no_diag = sp.csr_matrix(a - sp.diags(a.diagonal()))
    no_diag.eliminate_zeros()
    with pytest.raises(g.GkoError):
        g.factorization.Lu.build().with_symbolic_factorization(device_csr(gexec, no_diag, np.float64, np.int32)[0]) \
            .on(gexec).generate(dev)
    unsorted = g.Csr.from_arrays(gexec, a.shape, rp, ci[::-1].copy(), v)
    with pytest.raises(g.GkoError):
        g.factorization.Cholesky.build().with_symbolic_factorization(unsorted).on(gexec).generate(dev)
    with pytest.raises(g.NotSupported):
        g.factorization.Lu.build().with_symbolic_factorization("symmetric")


# ------------------------------------------------------------------ Direct
def reference_solve(kind, ref, b):
    if kind == "lu":
        l_rp, l_ci, l_v, u_rp, u_ci, u_v = ref
        return tr.trs_solve(u_rp, u_ci, u_v, tr.trs_solve(l_rp, l_ci, l_v, b, unit_diag=True), upper=True)
    l_rp, l_ci, l_v = ref
    lt = sp.csr_matrix((l_v, l_ci, l_rp), shape=(len(l_rp) - 1,) * 2).T.tocsr()
    lt.sort_indices()
    return tr.trs_solve(lt.indptr, lt.indices, lt.data, tr.trs_solve(l_rp, l_ci, l_v, b), upper=True)


@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("name", ["arrow_first70", "stencil5"])
@pytest.mark.parametrize("kind", KINDS)
def test_direct_apply_is_the_two_sequential_solves(gexec, kind, name, dtype, itype):
    a = case_matrix(name, kind == "cholesky")
    n = a.shape[0]
    dev, _ = device_csr(gexec, a, dtype, itype)
    ref = reference(kind, name, a, dtype)
    rng = np.random.default_rng(17)
    for cols in (1, 3):
        solver = g.Direct.build().with_factorization(factory(kind)).with_num_rhs(cols).on(gexec).generate(dev)
        assert isinstance(solver.get_factorization(),
                          g.factorization.Lu if kind == "lu" else g.factorization.Cholesky)
        b = rng.uniform(-1, 1, (n, cols)).astype(dtype)
        x = g.Dense.from_numpy(gexec, np.full((n, cols), np.nan, dtype))
        solver.apply(g.Dense.from_numpy(gexec, b), x)
        want = reference_solve(kind, ref, b)
        assert np.array_equal(x.to_numpy(), want)
        # it solves: the residual is at rounding level
        a_t = fr.dense_of(*fr.arrays(a, np.int32, dtype)).astype(np.float64)
        assert np.abs(a_t @ want.astype(np.float64) - b).max() <= 64 * n * np.finfo(dtype).eps * np.abs(b).max()
        # x = beta x + alpha solve(b): scale, then add_scaled, each product and the sum rounded
        x0 = rng.uniform(-1, 1, (n, cols)).astype(dtype)
        alpha, beta = dtype(0.75), dtype(-1.5)
        x = g.Dense.from_numpy(gexec, x0)
        solver.apply(g.scalar(gexec, float(alpha), dtype_of(dtype)), g.Dense.from_numpy(gexec, b),
                     g.scalar(gexec, float(beta), dtype_of(dtype)), x)
        assert np.array_equal(x.to_numpy(), (beta * x0).astype(dtype) + (alpha * want).astype(dtype))


def dtype_of(dtype):
    import torch
    return torch.float64 if dtype == np.float64 else torch.float32


def test_direct_takes_a_generated_factorization_and_defaults_to_lu(gexec):
    a = case_matrix("blocks", True)
    dev, _ = device_csr(gexec, a, np.float64, np.int32)
    fact = g.factorization.Cholesky.build().with_both_factors(False).on(gexec).generate(dev)
    solver = g.Direct.build().on(gexec).generate(fact)
    assert solver.get_factorization() is fact
    b = np.random.default_rng(3).uniform(-1, 1, (a.shape[0], 1))
    x = g.Dense.from_numpy(gexec, np.zeros_like(b))
    solver.apply(g.Dense.from_numpy(gexec, b), x)
    assert np.array_equal(x.to_numpy(), reference_solve("cholesky", reference("cholesky", "blocks", a, np.float64), b))
    default = g.Direct.build().on(gexec).generate(dev)
    assert isinstance(default.get_factorization(), g.factorization.Lu)
    with pytest.raises(g.NotSupported):
        g.Direct.build().with_factorization(g.factorization.Ilu.build()).on(gexec).generate(dev)


# ------------------------------------------------------------------ as a preconditioner
def cg_iterations(gexec, a, b, precond):
    f = g.Cg.build().with_criteria(g.stop.Iteration.build().with_max_iters(1000),
                                   g.stop.ResidualNorm.build().with_reduction_factor(1e-10))
    f = f.with_generated_preconditioner(precond) if isinstance(precond, g.base.LinOp) else f.with_preconditioner(precond)
    solver = f.on(gexec).generate(a)
    x = g.Dense.from_numpy(gexec, np.zeros_like(b))
    solver.apply(g.Dense.from_numpy(gexec, b), x)
    assert solver.has_converged
    return solver.num_iterations, x.to_numpy()[:, 0]


def test_cg_with_the_exact_factors_stops_after_one_iteration(gexec):
    a_host = fr.stencil27(5)
    a, _ = device_csr(gexec, a_host, np.float64, np.int32)
    b = np.random.default_rng(3).uniform(-1, 1, a_host.shape[0])
    jacobi, _ = cg_iterations(gexec, a, b, g.Jacobi.build().with_max_block_size(1))
    assert jacobi > 1
    for precond in (g.Ilu.build().with_factorization(g.factorization.Lu.build()),
                    g.Ic.build().with_factorization(g.factorization.Cholesky.build()),
                    g.Ilu.build().on(gexec).generate(g.factorization.Lu.build().on(gexec).generate(a))):
        count, x = cg_iterations(gexec, a, b, precond)
        assert count == 1, count
        assert np.linalg.norm(a_host @ x - b) <= 1e-10 * np.linalg.norm(b)
