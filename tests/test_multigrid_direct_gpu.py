"""Multigrid with a direct coarsest solver: Direct over factorization.Cholesky on a coarsest level of a few
hundred rows.  One V-cycle against a host restatement composed from tests/pgm_refs.py with the reference factors'
triangular loops at the bottom, by the criterion of tests/test_multigrid_gpu.py: the ratio to the restatement's
own rounding error, measured against the restatement."""
import numpy as np
import pytest
import scipy.sparse as sp

import ginkgo_amd as g
import factorization_refs as fr
import pgm_refs as pr
import symbolic_refs as sr
import trs_refs as tr
from test_pgm_gpu import device_matrix, matrix

pytestmark = pytest.mark.gpu

MIN_COARSE_ROWS = 400       # the hierarchy of the 12^3 stencil is 1728, 826, 391, ...: the cut leaves 391 rows
COARSEST_ROWS = 391


def direct_factory():
    return g.Direct.build().with_factorization(g.factorization.Cholesky.build())


def coarse_factor(level, dtype):
    """the reference Cholesky factor of a level's operator in `dtype` as (L arrays, L^T arrays)"""
    n = len(level["rp"]) - 1
    a = sp.csr_matrix((np.asarray(level["v"], np.float64), level["ci"], level["rp"]), shape=(n, n))
    rp, ci = sr.lu_pattern(a, np.int64)
    vals = np.zeros(len(ci), dtype)
    at = {(i, int(c)): k for i in range(n) for k, c in zip(range(rp[i], rp[i + 1]), ci[rp[i]:rp[i + 1]])}
    for i in range(n):
        for k in range(level["rp"][i], level["rp"][i + 1]):
            vals[at[(i, int(level["ci"][k]))]] = level["v"][k]
    l_rp, l_ci, l_v = fr.ic_factor(rp, ci, vals)
    # the transpose by positions, so that the values keep their type (longdouble too)
    order = np.lexsort((np.repeat(np.arange(n), np.diff(l_rp)), l_ci))
    t_rp = np.zeros(n + 1, l_rp.dtype)
    np.cumsum(np.bincount(l_ci, minlength=n), out=t_rp[1:])
    return (l_rp, l_ci, l_v), (t_rp, np.repeat(np.arange(n), np.diff(l_rp))[order].astype(l_ci.dtype), l_v[order])


def v_cycle(levels, factor, b, relax, l=0):
    """pr.cycle's V-cycle from a zero guess with the two triangular loops as coarsest solver"""
    level = levels[l]
    if l == len(levels) - 1:
        lower, upper = factor
        return tr.trs_solve(*upper, tr.trs_solve(*lower, b), upper=True)
    x = pr._sweeps(level, b, None, 1, relax)
    r = b - pr.spmv(level["rp"], level["ci"], level["v"], x)
    xc = v_cycle(levels, factor, pr.restrict(level["agg"], level["n_coarse"], r), relax, l + 1)
    x = pr.prolong_add(level["agg"], xc, x)
    return pr._sweeps(level, b, x, 1, relax)


@pytest.mark.parametrize("vt", [np.float64, np.float32], ids=["f64", "f32"])
def test_one_v_cycle_with_a_direct_coarsest_solve(gexec, vt):
    """e_ref is the max-norm error of the restatement in T against the same cycle, on the same aggregates, in
    np.longdouble; the device result must lie within 4 e_ref of that yardstick, the factor test_multigrid_gpu.py
    allows a cycle (the SpMV's fused alpha / beta rounding may differ from numpy's order)."""
    levels = pr.hierarchy(*pr.triple(matrix("stencil"), vt), vt, min_coarse_rows=MIN_COARSE_ROWS)
    assert [len(lv["rp"]) - 1 for lv in levels] == [1728, 826, COARSEST_ROWS]
    n = 1728
    b = np.random.default_rng(31).uniform(-1, 1, (n, 1)).astype(vt)
    relax = float(np.asarray(0.9, vt))
    x_t = v_cycle(levels, coarse_factor(levels[-1], vt), b, relax)
    exact = pr.hierarchy(*pr.triple(matrix("stencil"), vt), np.longdouble, min_coarse_rows=MIN_COARSE_ROWS,
                         aggs=[(lv["agg"], lv["n_coarse"]) for lv in levels[:-1]])
    x_l = v_cycle(exact, coarse_factor(exact[-1], np.longdouble), b.astype(np.longdouble), relax)
    e_ref = float(np.abs(x_t - x_l).max())
    assert e_ref > 0
    mg = (g.Multigrid.build().with_min_coarse_rows(MIN_COARSE_ROWS).with_coarsest_solver(direct_factory())
          .on(gexec).generate(device_matrix(gexec, "stencil", vt, np.int32)))
    assert isinstance(mg.get_coarsest_solver(), g.Direct) and mg.get_coarsest_solver().size == (COARSEST_ROWS,) * 2
    assert isinstance(mg.get_coarsest_solver().get_factorization(), g.factorization.Cholesky)
    assert mg.capturable
    x = g.Dense.from_numpy(gexec, np.full((n, 1), np.nan, vt))
    mg.apply(g.Dense.from_numpy(gexec, b), x)
    e_dev = float(np.abs(x.to_numpy().astype(np.longdouble) - x_l).max())
    print(f"v-cycle, direct coarsest solve, {np.dtype(vt).name}: e_ref {e_ref:.3e} e_dev {e_dev:.3e} "
          f"ratio {e_dev / e_ref:.3f}")
    assert e_dev <= 4 * e_ref, (e_dev, e_ref)


def test_cg_with_the_direct_coarsest_solver(gexec):
    """CG preconditioned by one V-cycle converges with either coarsest solver at the same cut-off; the counts
    are printed, no order between them is asserted"""
    a = device_matrix(gexec, "stencil", np.float64, np.int32)
    a_host = matrix("stencil")
    b = np.random.default_rng(3).uniform(-1, 1, a_host.shape[0])
    counts = {}
    for name, coarsest in (("direct", direct_factory()), ("sweeps", None)):
        mg = g.Multigrid.build().with_criteria(g.stop.Iteration.build().with_max_iters(1)) \
            .with_min_coarse_rows(MIN_COARSE_ROWS)
        if coarsest is not None:
            mg = mg.with_coarsest_solver(coarsest)
        solver = (g.Cg.build().with_criteria(g.stop.Iteration.build().with_max_iters(200),
                                             g.stop.ResidualNorm.build().with_reduction_factor(1e-10))
                  .with_preconditioner(mg).on(gexec).generate(a))
        x = g.Dense.from_numpy(gexec, np.zeros_like(b))
        solver.apply(g.Dense.from_numpy(gexec, b), x)
        assert solver.has_converged, name
        assert np.linalg.norm(a_host @ x.to_numpy()[:, 0] - b) <= 2e-10 * np.linalg.norm(b), name
        counts[name] = solver.num_iterations
    print(f"CG iterations with one V-cycle, coarsest level {COARSEST_ROWS} rows: {counts}")
