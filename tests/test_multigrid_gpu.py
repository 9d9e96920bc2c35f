"""Multigrid on the device: one cycle against the numpy restatement (tests/pgm_refs.py) with a tolerance taken
from the restatement's own error, the level list, Multigrid as a preconditioner of CG and as a solver."""
import numpy as np
import pytest

import ginkgo_amd as g
import pgm_refs as pr
from ginkgo_amd import _lib
from test_factorization_gpu import criteria, model_problem, solve_with  # noqa: F401
from test_pgm_gpu import device_matrix, matrix

pytestmark = pytest.mark.gpu

LEVEL_ROWS = [1728, 826, 391, 184, 88, 41]
_LEVELS = {}


def levels_of(name, vt):
    """the restatement's hierarchy of a case of test_pgm_gpu in the value type vt, computed once"""
    if (name, vt) not in _LEVELS:
        _LEVELS[(name, vt)] = pr.hierarchy(*pr.triple(matrix(name), vt), vt)
    return _LEVELS[(name, vt)]


def iteration(k):
    return g.stop.Iteration.build().with_max_iters(k)


def level_rows(mg):
    levels = mg.get_mg_level_list()
    return [lv.get_fine_op().size[0] for lv in levels] + [(levels[-1].get_coarse_op() if levels
                                                          else mg.get_system_matrix()).size[0]]


# ------------------------------------------------------------------ one cycle
@pytest.mark.parametrize("vt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["stencil", "scaled"])
@pytest.mark.parametrize("kind", ["v", "w"])
def test_one_cycle_lies_within_the_restatements_own_error(gexec, kind, name, vt):
    """The yardstick is the same cycle on the same aggregates evaluated in np.longdouble; e_ref is the max-norm
    error of the restatement in T against it, and the device result must lie within 4 e_ref of the yardstick
    (4: the SpMV's fused alpha / beta rounding may differ from numpy's order).
    Measured e_dev / e_ref on the MI355X (one run): f64 0.63 (v, scaled) to 1.05 (w, scaled), f32 0.88 (w, scaled)
    to 1.41 (v, scaled); the plain stencil lies between (Multigrid item)."""
    levels = levels_of(name, vt)
    n = len(levels[0]["rp"]) - 1
    b = np.random.default_rng(31).uniform(-1, 1, (n, 1)).astype(vt)
    relax = float(np.asarray(0.9, vt))          # the relaxation factor as T holds it, for the yardstick too
    x_t = pr.cycle(levels, b, kind=kind, relax=relax)
    exact = pr.hierarchy(*pr.triple(matrix(name), vt), np.longdouble,
                         aggs=[(lv["agg"], lv["n_coarse"]) for lv in levels[:-1]])
    assert [len(lv["rp"]) for lv in exact] == [len(lv["rp"]) for lv in levels]
    x_l = pr.cycle(exact, b.astype(np.longdouble), kind=kind, relax=relax)
    e_ref = float(np.abs(x_t - x_l).max())
    assert e_ref > 0
    mg = g.Multigrid.build().with_cycle(kind).on(gexec).generate(device_matrix(gexec, name, vt, np.int32))
    x = g.Dense.from_numpy(gexec, np.full((n, 1), np.nan, vt))      # the zero guess ignores what x holds
    mg.apply(g.Dense.from_numpy(gexec, b), x)
    e_dev = float(np.abs(x.to_numpy().astype(np.longdouble) - x_l).max())
    print(f"cycle {kind} {name} {np.dtype(vt).name}: e_ref {e_ref:.3e} e_dev {e_dev:.3e} ratio {e_dev / e_ref:.3f}")
    assert e_dev <= 4 * e_ref, (e_dev, e_ref)


def test_several_columns_with_a_stride(gexec):
    a = device_matrix(gexec, "stencil", np.float64, np.int32)
    mg = g.Multigrid.build().on(gexec).generate(a)
    n = a.size[0]
    b = np.random.default_rng(37).uniform(-1, 1, (n, 3))
    store = gexec.to_device(np.full((n, 5), 7.0))
    x = g.Dense(gexec, store[:, :3])
    mg.apply(g.Dense.from_numpy(gexec, b), x)
    want = pr.cycle(levels_of("stencil", np.float64), b)
    np.testing.assert_allclose(x.to_numpy(), want, rtol=0, atol=1e-14)
    assert np.all(store.cpu().numpy()[:, 3:] == 7.0)


# ------------------------------------------------------------------ levels
def test_level_list(gexec):
    a = device_matrix(gexec, "stencil", np.float64, np.int32)
    mg = g.Multigrid.build().on(gexec).generate(a)
    assert level_rows(mg) == LEVEL_ROWS
    assert all(isinstance(lv, g.Pgm) for lv in mg.get_mg_level_list())
    assert mg.get_coarsest_solver().size == (41, 41)
    nnz = [lv.get_fine_op().get_num_stored_elements() for lv in mg.get_mg_level_list()]
    nnz.append(mg.get_mg_level_list()[-1].get_coarse_op().get_num_stored_elements())
    assert nnz == [len(lv["v"]) for lv in levels_of("stencil", np.float64)]
    assert level_rows(g.Multigrid.build().with_max_levels(2).on(gexec).generate(a)) == LEVEL_ROWS[:2]
    assert level_rows(g.Multigrid.build().with_min_coarse_rows(10 ** 6).on(gexec).generate(a)) == LEVEL_ROWS[:1]
    assert level_rows(g.Multigrid.build().with_min_coarse_rows(200).on(gexec).generate(a)) == LEVEL_ROWS[:4]
    # the level factory is the caller's
    one_round = g.Multigrid.build().with_mg_level(g.Pgm.build().with_max_iterations(1)).on(gexec).generate(a)
    assert all(lv.rounds == 1 for lv in one_round.get_mg_level_list()) and level_rows(one_round) != LEVEL_ROWS
    # a level that does not get smaller ends the list
    eye = g.Csr.from_arrays(gexec, (300, 300), np.arange(301, dtype=np.int32), np.arange(300, dtype=np.int32),
                            np.ones(300))
    assert level_rows(g.Multigrid.build().on(gexec).generate(eye)) == [300]
    with pytest.raises(g.GkoError):
        g.Multigrid.build().with_cycle("f").on(gexec).generate(a)


# ------------------------------------------------------------------ as a preconditioner
def multigrid(**params):
    f = g.Multigrid.build().with_criteria(iteration(1))
    for k, v in params.items():
        f = getattr(f, "with_" + k)(v)
    return f


def test_cg_with_one_cycle_needs_the_host_count(gexec, model_problem):
    a, a_host, b = model_problem
    jacobi, _ = solve_with(gexec, g.Cg, a, b, g.Jacobi.build().with_max_block_size(1))
    v, x = solve_with(gexec, g.Cg, a, b, multigrid())
    print(f"CG iterations: Multigrid(v) {v.num_iterations}, scalar Jacobi {jacobi.num_iterations}")
    assert v.has_converged and v.num_iterations <= 13           # the host count of 12, plus 1 for rounding
    assert v.num_iterations < jacobi.num_iterations
    assert np.linalg.norm(a_host @ x - b) <= 2e-10 * np.linalg.norm(b)
    w, x = solve_with(gexec, g.Cg, a, b, multigrid(cycle="w"))
    assert w.has_converged and w.num_iterations <= v.num_iterations
    assert np.linalg.norm(a_host @ x - b) <= 2e-10 * np.linalg.norm(b)
    # no criteria at all is one cycle as well
    none, _ = solve_with(gexec, g.Cg, a, b, g.Multigrid.build())
    assert none.num_iterations == v.num_iterations


def test_user_smoothers_and_coarsest_solver(gexec, model_problem):
    a, a_host, b = model_problem
    jac = g.Jacobi.build().with_max_block_size(1)
    inner = g.Cg.build().with_criteria(iteration(30), g.stop.ResidualNorm.build().with_reduction_factor(1e-6))
    for params in ({"pre_smoother": jac}, {"pre_smoother": jac, "post_smoother": jac, "smoother_iters": 2},
                   {"coarsest_solver": inner}, {"pre_smoother": jac, "coarsest_solver": inner}):
        solver, x = solve_with(gexec, g.Cg, a, b, multigrid(**params))
        assert solver.has_converged, params
        assert np.linalg.norm(a_host @ x - b) <= 2e-10 * np.linalg.norm(b), params
    # a Jacobi operator as smoother with the built-in relaxation is the built-in smoother up to rounding
    builtin, _ = solve_with(gexec, g.Cg, a, b, multigrid())
    user, _ = solve_with(gexec, g.Cg, a, b, multigrid(pre_smoother=jac))
    assert abs(user.num_iterations - builtin.num_iterations) <= 1
    mg = multigrid(coarsest_solver=inner).on(gexec).generate(a)
    assert isinstance(mg.get_coarsest_solver(), g.Cg) and isinstance(mg.get_preconditioner(), g.Identity)


def test_for_other_solver_classes(gexec, model_problem):
    a, a_host, b = model_problem
    jacobi, _ = solve_with(gexec, g.Cg, a, b, g.Jacobi.build().with_max_block_size(1))
    for cls in (g.Bicgstab, g.Gmres, g.Fcg):
        solver, x = solve_with(gexec, cls, a, b, multigrid())
        # Gmres minimises the residual over CG's Krylov space and Fcg is CG in exact arithmetic: CG's bound;
        # Bicgstab has no such bound, it only has to beat CG with scalar Jacobi
        bound = jacobi.num_iterations - 1 if cls is g.Bicgstab else 13
        assert solver.has_converged and solver.num_iterations <= bound, cls
        assert np.linalg.norm(a_host @ x - b) <= 2e-10 * np.linalg.norm(b), cls


def test_an_application_neither_copies_to_the_host_nor_synchronises(gexec, model_problem):
    a, _, b = model_problem
    mg = multigrid().on(gexec).generate(a)
    db, x = g.Dense.from_numpy(gexec, b), g.Dense.from_numpy(gexec, np.zeros_like(b))
    mg.apply(db, x)                 # warm-up: the level vectors are allocated here
    before = gexec.arena_info()["num_allocations"]
    with _lib.record() as tape:
        mg.apply(db, x)
    names = [name for _, _, name in tape.calls]
    assert "gkoc_pgm_restrict_f64_i32" in names and "gkoc_pgm_prolong_add_f64_i32" in names
    assert names.count("gkoc_pgm_restrict_f64_i32") == len(LEVEL_ROWS) - 1
    forbidden = [nm for nm in names if "memcpy" in nm or "synchronize" in nm or "malloc" in nm or "pgm_check" in nm]
    assert not forbidden, forbidden
    assert gexec.arena_info()["num_allocations"] == before
    # two products per level and cycle above the coarsest (residual, post-smoother), three more sweeps there
    products = [nm for nm in names if nm.startswith("gkoc_csr_advanced_spmv")]
    assert len(products) == 2 * (len(LEVEL_ROWS) - 1) + 3 and not [nm for nm in names if nm == "gkoc_csr_spmv_f64_i32"]


# ------------------------------------------------------------------ as a solver
def test_as_a_solver_with_a_residual_criterion(gexec, model_problem):
    a, a_host, b = model_problem
    host = pr.stationary_iterations(a_host, b, levels_of("stencil", np.float64), 1e-8)
    solver = (g.Multigrid.build()
              .with_criteria(iteration(100), g.stop.ResidualNorm.build().with_reduction_factor(1e-8))
              .on(gexec).generate(a))
    x = g.Dense.from_numpy(gexec, np.full_like(b, 1e30))       # default_initial_guess is zero
    solver.apply(g.Dense.from_numpy(gexec, b), x)
    print(f"Multigrid as a solver: {solver.num_iterations} cycles, host {host}")
    assert solver.has_converged and abs(solver.num_iterations - host) <= 1
    assert np.linalg.norm(a_host @ x.to_numpy()[:, 0] - b) <= 1e-8 * np.linalg.norm(b)
    assert float(solver.residual_norm[0]) <= 1e-8 * np.linalg.norm(b)


def test_provided_initial_guess_continues_from_x(gexec, model_problem):
    a, _, b = model_problem
    db = g.Dense.from_numpy(gexec, b)
    two = g.Multigrid.build().with_criteria(iteration(2)).on(gexec).generate(a)
    x2 = g.Dense.from_numpy(gexec, np.zeros_like(b))
    two.apply(db, x2)
    assert two.num_iterations == 2
    x = g.Dense.from_numpy(gexec, np.full_like(b, 3.0))
    g.Multigrid.build().with_criteria(iteration(1)).on(gexec).generate(a).apply(db, x)
    first = x.to_numpy()
    (g.Multigrid.build().with_criteria(iteration(1)).with_default_initial_guess("provided")
     .on(gexec).generate(a).apply(db, x))
    assert np.array_equal(x.to_numpy(), x2.to_numpy()) and not np.array_equal(first, x2.to_numpy())
    with pytest.raises(g.GkoError):
        g.Multigrid.build().with_default_initial_guess("ones").on(gexec).generate(a)
