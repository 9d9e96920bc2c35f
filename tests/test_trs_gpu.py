"""Level-scheduled triangular solves (LowerTrs / UpperTrs) and the Sor / GaussSeidel preconditioner on
the device, against the numpy loops of tests/trs_refs.py.  Results are compared with np.array_equal:
the kernels promise the reference's rounding."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import ginkgo_amd as g
import trs_refs as tr

pytestmark = pytest.mark.gpu

TYPES = [(np.float64, np.int32), (np.float64, np.int64), (np.float32, np.int32), (np.float32, np.int64)]
TYPE_IDS = ["f64-i32", "f64-i64", "f32-i32", "f32-i64"]
SIDES = [False, True]
SIDE_IDS = ["lower", "upper"]


# ------------------------------------------------------------------ helpers
def trs(gexec, rp, ci, v, upper, unit=False):
    n = len(rp) - 1
    a = g.Csr.from_arrays(gexec, (n, n), rp, ci, v)
    cls = g.UpperTrs if upper else g.LowerTrs
    return cls.build().with_unit_diagonal(unit).with_num_rhs(1).on(gexec).generate(a)


def strided(gexec, array, ld, fill=0.0):
    """(Dense view of `array` inside a store with row stride ld, the store)"""
    n, k = array.shape
    full = np.full((n, ld), fill, array.dtype)
    full[:, :k] = array
    store = gexec.to_device(full)
    return g.Dense(gexec, store[:, :k]), store


def run(gexec, solver, b):
    """solve with ldb = nrhs + 3 and ldx = nrhs + 2, x's padding NaN before and after"""
    n, nrhs = b.shape
    bd, _ = strided(gexec, b, nrhs + 3, fill=7.0)
    xd, store = strided(gexec, np.full_like(b, np.nan), nrhs + 2, fill=np.nan)
    solver.apply(bd, xd)
    full = store.cpu().numpy()
    assert np.isnan(full[:, nrhs:]).all(), "the solve wrote into the padding of x"
    return full[:, :nrhs]


def expected_launches(level_ptrs, w):
    wide = np.diff(level_ptrs) > w
    narrow_runs = int(np.sum(~wide & np.r_[True, wide[:-1]]))
    return int(wide.sum()) + narrow_runs


def check_schedule(solver, rp, ci, upper):
    n = len(rp) - 1
    ptrs, rows = solver.levels()
    ref_ptrs, ref_rows, _ = tr.levels(rp, ci, upper)
    assert solver.num_levels == len(ptrs) - 1 == len(ref_ptrs) - 1
    assert np.array_equal(np.sort(rows), np.arange(n)), "levels() is not a permutation of the rows"
    assert ptrs[0] == 0 and ptrs[-1] == n and (np.diff(ptrs) > 0).all()
    level_of = np.empty(n, np.int64)
    level_of[rows] = np.repeat(np.arange(solver.num_levels), np.diff(ptrs))
    row_of = np.repeat(np.arange(n), np.diff(rp))
    dep = ci > row_of if upper else ci < row_of
    assert (level_of[ci[dep]] < level_of[row_of[dep]]).all(), "a dependency is not in an earlier level"
    inner = np.ones(max(n - 1, 0), bool)
    inner[ptrs[1:-1] - 1] = False
    assert (np.diff(rows)[inner] > 0).all(), "rows do not ascend inside a level"
    assert np.array_equal(ptrs, ref_ptrs) and np.array_equal(rows, ref_rows)
    assert 1 <= solver.wide_threshold <= 4096
    assert solver.num_launches == expected_launches(ptrs, solver.wide_threshold)


_REFS = {}      # reference solutions, shared by the index types and by the tests that use one case


def check_case(gexec, rows_or_csr, upper, dtype, itype, nrhs=1, unit=False, seed=0, key=None):
    if isinstance(rows_or_csr, list):
        rp, ci, v = tr.from_rows(tr.mirror(rows_or_csr) if upper else rows_or_csr, itype, dtype)
    else:
        rp, ci, v = (a.astype(t) for a, t in zip(rows_or_csr, (itype, itype, dtype)))
    n = len(rp) - 1
    solver = trs(gexec, rp, ci, v, upper, unit)
    check_schedule(solver, rp, ci, upper)
    b = np.random.default_rng(seed).uniform(-1, 1, (n, nrhs)).astype(dtype)
    got = run(gexec, solver, b)
    key = key and (key, upper, dtype, nrhs, unit, seed)
    ref = _REFS.get(key)
    if ref is None:
        ref = tr.trs_solve(rp, ci, v, b, upper=upper, unit_diag=unit)
        ref.setflags(write=False)
        if key:
            _REFS[key] = ref
    assert np.isfinite(ref).all()
    assert np.array_equal(got, ref)
    return solver, got


def general_rows(n, rng, deps, shuffle=True):
    """row i: min(i, deps) distinct dependencies, a diagonal in [1, 2]; storage order shuffled"""
    rows = []
    for i in range(n):
        cols = rng.choice(i, min(i, deps), replace=False) if i else []
        r = [(int(c), float(rng.uniform(-0.5, 0.5))) for c in cols] + [(i, float(rng.uniform(1, 2)))]
        if shuffle:
            rng.shuffle(r)
        rows.append([tuple(e) for e in r])
    return rows


@functools.lru_cache(maxsize=None)
def wide_threshold(gexec):
    rp, ci, v = tr.from_rows([[(0, 1.0)]])
    return trs(gexec, rp, ci, v, False).wide_threshold


@functools.lru_cache(maxsize=None)
def case_rows(name, w=None):
    rng = np.random.default_rng(len(name) * 7 + 1)
    if name == "one":
        return [[(0, 2.0)]]
    if name == "diagonal":
        return [[(i, float(rng.uniform(1, 2)))] for i in range(300)]
    if name == "chain":
        # 2500 levels of one row in one narrow launch; consecutive levels write neighbouring words
        return [([(i - 1, float(rng.uniform(-0.9, 0.9)))] if i else []) + [(i, float(rng.uniform(1, 2)))]
                for i in range(2500)]
    if name == "tiers":
        rows = tr.tiers_rows(w, rng)
        return [[(c, v * 0.25 if c != i else v) for c, v in r] for i, r in enumerate(rows)]
    if name == "random":
        return general_rows(4000, rng, 4)
    if name == "hub":
        # row 350 has 300 entries, row 0 has 1, the others 2
        rows = general_rows(400, rng, 1)
        cols = rng.permutation(350)[:299]
        hub = [(int(c), float(rng.uniform(-0.1, 0.1))) for c in cols] + [(350, 1.5)]
        rng.shuffle(hub)
        rows[350] = [tuple(e) for e in hub]
        return rows
    if name == "no_diagonal":
        rows = general_rows(200, rng, 3)
        for i in (0, 57, 199):
            rows[i] = [e for e in rows[i] if e[0] != i]
        return rows
    raise KeyError(name)


# ------------------------------------------------------------------ solves
@pytest.mark.parametrize("upper", SIDES, ids=SIDE_IDS)
@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("name", ["one", "diagonal", "chain", "random", "hub", "no_diagonal"])
def test_solve_matches_reference(gexec, name, dtype, itype, upper):
    solver, _ = check_case(gexec, case_rows(name), upper, dtype, itype, key=name)
    if name in ("one", "diagonal"):
        assert solver.num_levels == 1 and solver.num_launches == 1
    if name == "chain":
        assert solver.num_levels == 2500 and solver.num_launches == 1


@pytest.mark.parametrize("upper", SIDES, ids=SIDE_IDS)
@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
def test_empty_system(gexec, dtype, itype, upper):
    rp, ci, v = np.zeros(1, itype), np.zeros(0, itype), np.zeros(0, dtype)
    solver = trs(gexec, rp, ci, v, upper)
    assert (solver.num_levels, solver.num_launches) == (0, 0)
    ptrs, rows = solver.levels()
    assert np.array_equal(ptrs, [0]) and rows.size == 0
    x = g.Dense.create(gexec, (0, 1), g.Dense.from_numpy(gexec, np.zeros((1, 1), dtype)).dtype)
    solver.apply(x, x)
    # no right-hand side at all
    one = trs(gexec, *tr.from_rows([[(0, 2.0)]], itype, dtype), upper)
    e = g.Dense(gexec, gexec.to_device(np.zeros((1, 2), dtype))[:, :0])
    one.apply(e, e)


@pytest.mark.parametrize("upper", SIDES, ids=SIDE_IDS)
@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
def test_tiers_wide_wide_narrow(gexec, dtype, itype, upper):
    w = wide_threshold(gexec)
    rows = case_rows("tiers", w)
    assert len(rows) < 13000
    solver, _ = check_case(gexec, rows, upper, dtype, itype, key="tiers")
    assert solver.num_levels == 42 and solver.num_launches == 3


@pytest.mark.parametrize("upper", SIDES, ids=SIDE_IDS)
@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
def test_stencil_full_matrix_and_triangle(gexec, oracle, dtype, itype, upper):
    rp, ci, v = oracle.stencil_csr(3, 12)
    a = sp.csr_matrix((v, ci, rp), shape=(1728, 1728))
    tri = sp.triu(a, format="csr") if upper else sp.tril(a, format="csr")
    _, full = check_case(gexec, (rp, ci, v), upper, dtype, itype, key="stencil")
    solver, part = check_case(gexec, (tri.indptr, tri.indices, tri.data), upper, dtype, itype)
    assert solver.num_levels == 78
    assert np.array_equal(full, part)


@pytest.mark.parametrize("upper", SIDES, ids=SIDE_IDS)
@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("name", ["random", "tiers", "chain"])
def test_three_right_hand_sides(gexec, name, dtype, itype, upper):
    rows = case_rows(name, wide_threshold(gexec) if name == "tiers" else None)
    check_case(gexec, rows, upper, dtype, itype, nrhs=3, seed=4, key=name)


@pytest.mark.parametrize("upper", SIDES, ids=SIDE_IDS)
@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
def test_unit_diagonal_ignores_the_stored_one(gexec, dtype, itype, upper):
    rng = np.random.default_rng(9)
    rows = [[(c, v if c != i else float(rng.choice([0.0, 1e30, -3.0]))) for c, v in r]
            for i, r in enumerate(general_rows(500, rng, 3))]
    check_case(gexec, rows, upper, dtype, itype, nrhs=3, unit=True)
    # without a stored diagonal at all: the same answer as with unit_diagonal
    bare = [[e for e in r if e[0] != i] for i, r in enumerate(rows)]
    _, x_unit = check_case(gexec, rows, upper, dtype, itype, unit=True)
    _, x_bare = check_case(gexec, bare, upper, dtype, itype, unit=False)
    assert np.array_equal(x_unit, x_bare)


@pytest.mark.parametrize("upper", SIDES, ids=SIDE_IDS)
@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("name", ["tiers", "chain"])
def test_planted_answers(gexec, name, dtype, itype, upper):
    """dyadic entries, integer x, b = T x exactly: x comes back exactly, whatever the reference says"""
    rng = np.random.default_rng(21)
    rows = tr.tiers_rows(wide_threshold(gexec), rng) if name == "tiers" else tr.chain_rows(2500, rng)
    if upper:
        rows = tr.mirror(rows)
    x, b = tr.planted(rows, rng, nrhs=3)
    rp, ci, v = tr.from_rows(rows, itype, dtype)
    got = run(gexec, trs(gexec, rp, ci, v, upper), b.astype(dtype))
    assert np.array_equal(got, x)


@pytest.mark.parametrize("upper", SIDES, ids=SIDE_IDS)
@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("alpha,beta", [(-1.0, 2.0), (0.75, 0.0)])
def test_advanced_apply(gexec, alpha, beta, dtype, itype, upper):
    rows = case_rows("random")
    rp, ci, v = tr.from_rows(tr.mirror(rows) if upper else rows, itype, dtype)
    n = len(rows)
    solver = trs(gexec, rp, ci, v, upper)
    rng = np.random.default_rng(2)
    b, x0 = (rng.uniform(-1, 1, (n, 3)).astype(dtype) for _ in range(2))
    bd, _ = strided(gexec, b, 6)
    xd, store = strided(gexec, x0, 5, fill=np.nan)
    solver.apply(g.Dense.from_numpy(gexec, np.array([[alpha]], dtype)), bd,
                 g.Dense.from_numpy(gexec, np.array([[beta]], dtype)), xd)
    ref = dtype(beta) * x0 + dtype(alpha) * tr.trs_solve(rp, ci, v, b, upper=upper)
    full = store.cpu().numpy()
    assert ref.dtype == dtype and np.array_equal(full[:, :3], ref) and np.isnan(full[:, 3:]).all()


def test_linop_interface(gexec):
    rp, ci, v = tr.from_rows(case_rows("hub"))
    a = g.Csr.from_arrays(gexec, (400, 400), rp, ci, v)
    solver = g.LowerTrs.build().on(gexec).generate(a)
    assert solver.get_system_matrix() is a and solver.get_size() == (400, 400)
    with pytest.raises(g.NotSupported):
        g.LowerTrs.build().on(gexec).generate(g.Dense.create(gexec, (4, 4)))
    with pytest.raises(g.NotSupported):
        g.UpperTrs.build().on(gexec).generate(a.convert_to_ell())
    wide = g.Csr.from_arrays(gexec, (2, 3), np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32),
                             np.ones(2))
    with pytest.raises(g.DimensionMismatch):
        g.UpperTrs.build().on(gexec).generate(wide)
    with pytest.raises(g.DimensionMismatch):
        solver.apply(g.Dense.create(gexec, (399, 1)), g.Dense.create(gexec, (400, 1)))


# ------------------------------------------------------------------ argument checks of the C ABI
def test_invalid_arguments_are_refused_and_the_device_stays_usable(gexec):
    from ginkgo_amd._lib import call
    rows = case_rows("hub")
    rp, ci, v = tr.from_rows(rows)
    n = len(rows)
    lower = trs(gexec, rp, ci, v, False)
    upper = trs(gexec, rp, ci, v, True)
    a = lower.get_system_matrix()
    b = g.Dense.from_numpy(gexec, np.ones((n, 2)))
    x = g.Dense.create(gexec, (n, 2))
    st = gexec.stream

    def solve(name="gkoc_lower_trs_solve_f64_i32", t=None, n_=n, nrhs=2, rp_=a.row_ptrs, ci_=a.col_idxs,
              v_=a.values, b_=b.values, ldb=2, x_=x.values, ldx=2):
        call(name, st, lower._struct if t is None else t, C.c_int(0), n_, nrhs, rp_, ci_, v_, b_, ldb, x_, ldx)

    bad = [dict(n_=-1), dict(nrhs=-1), dict(ldb=1), dict(ldx=1), dict(rp_=None), dict(ci_=None),
           dict(v_=None), dict(b_=None), dict(x_=None), dict(t=upper._struct), dict(n_=n - 1),
           dict(t=C.c_void_p(0)), dict(name="gkoc_upper_trs_solve_f64_i32")]
    for kw in bad:
        with pytest.raises(g.GkoError):
            solve(**kw)
    out = C.c_void_p()
    for name in ("gkoc_lower_trs_generate_i32", "gkoc_upper_trs_generate_i32"):
        with pytest.raises(g.GkoError):
            call(name, st, -1, a.row_ptrs, a.col_idxs, C.byref(out))
        with pytest.raises(g.GkoError):
            call(name, st, n, None, a.col_idxs, C.byref(out))
        with pytest.raises(g.GkoError):
            call(name, st, n, a.row_ptrs, None, C.byref(out))
        assert not out.value
    with pytest.raises(g.GkoError):
        call("gkoc_trs_struct_info", C.c_void_p(0), None, None, None, None, None)
    l_rp = gexec.alloc((n + 1,), a.row_ptrs.dtype)
    with pytest.raises(g.GkoError):
        call("gkoc_factorization_initialize_row_ptrs_l_u_i32", st, -1, a.row_ptrs, a.col_idxs, l_rp, None)
    with pytest.raises(g.GkoError):
        call("gkoc_factorization_initialize_row_ptrs_l_u_i32", st, n, None, a.col_idxs, l_rp, None)
    for w in (0.0, 2.0, -0.5, 2.5, float("nan")):
        with pytest.raises(g.GkoError):
            g.Sor.build().with_relaxation_factor(w).on(gexec).generate(a)
        with pytest.raises(g.GkoError):
            g.Sor.build().with_relaxation_factor(w).with_symmetric(True).on(gexec).generate(a)
    with pytest.raises(g.GkoError):
        call("gkoc_sor_initialize_weighted_l_f64_i32", st, -1, a.row_ptrs, a.col_idxs, a.values,
             C.c_double(1.0), l_rp, None, None)
    with pytest.raises(g.GkoError):
        call("gkoc_sor_initialize_weighted_l_u_f64_i32", st, n, a.row_ptrs, a.col_idxs, a.values,
             C.c_double(1.0), l_rp, None, None, None, None, None)
    # nothing of the above reached the device: a valid solve is still right
    ref = tr.trs_solve(rp, ci, v, np.ones((n, 2)))
    solve()
    assert np.array_equal(x.to_numpy(), ref)


# ------------------------------------------------------------------ Sor / GaussSeidel
def sor_matrix(dtype, itype, seed=6, n=300):
    """diagonally dominant, unsymmetric pattern, a few rows without entries on one side"""
    rng = np.random.default_rng(seed)
    a = sp.random(n, n, 0.03, random_state=rng, format="lil", data_rvs=lambda k: rng.uniform(-1, 1, k))
    a.setdiag(rng.uniform(4, 5, n))
    a = a.tocsr()
    a.sort_indices()
    return a.indptr.astype(itype), a.indices.astype(itype), a.data.astype(dtype)


def csr_arrays(m):
    return [t.cpu().numpy() for t in (m.row_ptrs, m.col_idxs, m.values)]


@pytest.mark.parametrize("symmetric", [False, True], ids=["sor", "ssor"])
@pytest.mark.parametrize("weight", [1.0, 1.2])
@pytest.mark.parametrize("dtype,itype", TYPES, ids=TYPE_IDS)
def test_sor_factors_and_apply(gexec, dtype, itype, weight, symmetric):
    rp, ci, v = sor_matrix(dtype, itype)
    n = len(rp) - 1
    a = g.Csr.from_arrays(gexec, (n, n), rp, ci, v)
    m = (g.Sor.build().with_relaxation_factor(weight).with_symmetric(symmetric).with_skip_sorting(False)
         .on(gexec).generate(a))
    ref = tr.weighted_l_u(rp, ci, v, weight)
    got_l = csr_arrays(m.l)
    assert all(p.dtype == q.dtype and np.array_equal(p, q) for p, q in zip(got_l, ref[:3]))
    b = np.random.default_rng(1).uniform(-1, 1, (n, 1)).astype(dtype)
    z = tr.trs_solve(*ref[:3], b)
    if symmetric:
        got_u = csr_arrays(m.u)
        assert all(p.dtype == q.dtype and np.array_equal(p, q) for p, q in zip(got_u, ref[3:]))
        z = tr.trs_solve(*ref[3:], z, upper=True)
    else:
        assert m.u is None
    x = g.Dense.from_numpy(gexec, np.full((n, 1), np.nan, dtype))
    m.apply(g.Dense.from_numpy(gexec, b), x)
    assert np.array_equal(x.to_numpy(), z)
    # advanced apply, and three right-hand sides through the same object
    b3 = np.random.default_rng(2).uniform(-1, 1, (n, 3)).astype(dtype)
    x0 = np.random.default_rng(3).uniform(-1, 1, (n, 3)).astype(dtype)
    z3 = tr.trs_solve(*ref[:3], b3)
    if symmetric:
        z3 = tr.trs_solve(*ref[3:], z3, upper=True)
    x = g.Dense.from_numpy(gexec, x0)
    m.apply(g.Dense.from_numpy(gexec, np.array([[-1.0]], dtype)), g.Dense.from_numpy(gexec, b3),
            g.Dense.from_numpy(gexec, np.array([[2.0]], dtype)), x)
    assert np.array_equal(x.to_numpy(), dtype(2) * x0 + dtype(-1) * z3)


def test_sor_sorts_unsorted_input_unless_told_not_to(gexec):
    rp, ci, v = sor_matrix(np.float64, np.int32)
    n = len(rp) - 1
    rng = np.random.default_rng(8)
    ci_u, v_u = ci.copy(), v.copy()
    for r in range(n):
        p = rng.permutation(rp[r + 1] - rp[r])
        ci_u[rp[r]:rp[r + 1]], v_u[rp[r]:rp[r + 1]] = ci[rp[r]:rp[r + 1]][p], v[rp[r]:rp[r + 1]][p]
    a = g.Csr.from_arrays(gexec, (n, n), rp, ci_u, v_u)
    f = g.Sor.build().with_relaxation_factor(1.2).with_symmetric(True).on(gexec)
    m = f.generate(a)
    assert np.array_equal(a.col_idxs.cpu().numpy(), ci_u), "generate changed the caller's matrix"
    for got, ref in zip(csr_arrays(m.l) + csr_arrays(m.u), tr.weighted_l_u(rp, ci, v, 1.2)):
        assert np.array_equal(got, ref)
    m = f.with_skip_sorting(True).generate(a)
    for got, ref in zip(csr_arrays(m.l) + csr_arrays(m.u), tr.weighted_l_u(rp, ci_u, v_u, 1.2)):
        assert np.array_equal(got, ref)


def test_gauss_seidel_is_sor_with_weight_one(gexec):
    rp, ci, v = sor_matrix(np.float64, np.int32)
    n = len(rp) - 1
    a = g.Csr.from_arrays(gexec, (n, n), rp, ci, v)
    b = g.Dense.from_numpy(gexec, np.random.default_rng(1).uniform(-1, 1, (n, 1)))
    for symmetric in (False, True):
        gs = g.GaussSeidel.build().with_symmetric(symmetric).on(gexec).generate(a)
        so = g.Sor.build().with_relaxation_factor(1.0).with_symmetric(symmetric).on(gexec).generate(a)
        assert isinstance(gs, g.GaussSeidel) and gs.relaxation_factor == 1.0
        for p, q in zip(csr_arrays(gs.l), csr_arrays(so.l)):
            assert np.array_equal(p, q)
        x1, x2 = g.Dense.create(gexec, (n, 1)), g.Dense.create(gexec, (n, 1))
        gs.apply(b, x1)
        so.apply(b, x2)
        assert np.array_equal(x1.to_numpy(), x2.to_numpy()) and np.isfinite(x1.to_numpy()).all()


def test_sor_of_an_fbcsr_matrix(gexec):
    rng = np.random.default_rng(12)
    blocks = sp.random(40, 40, 0.1, random_state=rng, format="csr") + sp.eye(40)
    a = sp.kron(blocks, np.ones((3, 3)), format="csr")
    a.data = rng.uniform(-1, 1, a.nnz)
    a = (a + sp.diags(np.full(120, 9.0))).tocsr()
    fb = g.Fbcsr.from_scipy(gexec, sp.bsr_matrix(a, blocksize=(3, 3)))
    csr = fb.convert_to_csr()
    f = g.Sor.build().with_relaxation_factor(1.2).with_symmetric(True).on(gexec)
    m1, m2 = f.generate(fb), f.generate(csr)
    for p, q in zip(csr_arrays(m1.l) + csr_arrays(m1.u), csr_arrays(m2.l) + csr_arrays(m2.u)):
        assert p.size and np.array_equal(p, q)


# ------------------------------------------------------------------ end to end
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


def test_cg_with_ssor_beats_scalar_jacobi(gexec, model_problem):
    a, a_host, b = model_problem
    ssor = lambda: g.Sor.build().with_relaxation_factor(1.0).with_symmetric(True)
    jacobi = lambda: g.Jacobi.build().with_max_block_size(1)
    s_ssor, x_ssor = solve_with(gexec, g.Cg, a, b, ssor())
    s_jac, x_jac = solve_with(gexec, g.Cg, a, b, jacobi())
    print("iterations: SSOR(1)", s_ssor.num_iterations, "scalar Jacobi", s_jac.num_iterations)
    for s, x in ((s_ssor, x_ssor), (s_jac, x_jac)):
        assert s.has_converged and s.num_iterations < 1000
        assert np.linalg.norm(b - a_host @ x) <= 1e-9 * np.linalg.norm(b)
    assert s_ssor.num_iterations < s_jac.num_iterations
    # captured iterations (the default at this size) against plain launches
    e_ssor, y_ssor = solve_with(gexec, g.Cg, a, b, ssor(), hip_graph=False)
    e_jac, y_jac = solve_with(gexec, g.Cg, a, b, jacobi(), hip_graph=False)
    assert e_ssor.has_converged and e_jac.has_converged
    assert e_jac.num_iterations == s_jac.num_iterations
    assert e_ssor.num_iterations == s_ssor.num_iterations
    control = np.array_equal(x_jac, y_jac)
    print("scalar Jacobi bit-equal between graph and plain launches:", control)
    if control:
        assert np.array_equal(x_ssor, y_ssor)


def test_generated_preconditioner_and_other_solvers(gexec, model_problem):
    a, a_host, b = model_problem
    for cls, precond in ((g.Gmres, g.Sor.build().with_relaxation_factor(1.2).with_symmetric(False)),
                         (g.Bicgstab, g.GaussSeidel.build())):
        s, x = solve_with(gexec, cls, a, b, precond)
        assert s.has_converged and s.num_iterations < 1000, cls.__name__
        assert np.linalg.norm(b - a_host @ x) <= 1e-8 * np.linalg.norm(b), cls.__name__
    m = g.Sor.build().with_relaxation_factor(1.2).with_symmetric(True).on(gexec).generate(a)
    f = g.Cg.build().with_criteria(*criteria()).with_generated_preconditioner(m).on(gexec)
    s = f.generate(a)
    x = g.Dense.from_numpy(gexec, np.zeros_like(b))
    s.apply(g.Dense.from_numpy(gexec, b), x)
    assert s.get_preconditioner() is m and s.has_converged
    assert np.linalg.norm(b - a_host @ x.to_numpy()[:, 0]) <= 1e-9 * np.linalg.norm(b)
