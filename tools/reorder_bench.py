"""reorder.NestedDissection in front of factorization.Cholesky and the Direct coarsest solver of Multigrid, on the
Pgm coarse operators of the 27-point Laplacian (tools/direct_bench.py measures the natural order alone): per
operator, in one call and alternating, natural order and the dissection at every leaf size - nnz(L), the levels
of the lower solve, the reordering time with its rounds and the launches the host waits for, Cholesky.generate
and its numeric phase (the pattern given), and one V-cycle with Direct / ScaledReordered(Direct) at the bottom
against the built-in four sweeps.  f64 / int32.  (development / measurement tool)

    python tools/reorder_bench.py [grid:cut ...] [--leaf-size=8,32,64,128]
                                  default: 64:500 64:1000 64:2000 128:2000   (339, 712, 1485 and 2687 rows)

Timing as in tools/direct_bench.py: a host clock around a second, synchronised call; an application over `reps`
plain launches between two synchronisations."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

import ginkgo_amd as g

cases = [a for a in sys.argv[1:] if not a.startswith("--")] or ["64:500", "64:1000", "64:2000", "128:2000"]
leaf_sizes = [8, 32, 64, 128]
for arg in sys.argv[1:]:
    if arg.startswith("--leaf-size="):
        leaf_sizes = [int(c) for c in arg.split("=")[1].split(",")]
ex = g.Cdna4Executor.create(0)
REPS = 5


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t


def apply_us(op):
    b = g.Dense.from_numpy(ex, np.ones(op.size[0]))
    x = g.Dense.create(ex, (op.size[0], 1))
    op.apply(b, x)
    _, t = wall(lambda: [op.apply(b, x) for _ in range(REPS)])
    return t * 1e6 / REPS


def multigrid(a, cut, coarsest):
    f = g.Multigrid.build().with_criteria(g.stop.Iteration.build().with_max_iters(1)).with_min_coarse_rows(cut)
    if coarsest is not None:
        f = f.with_coarsest_solver(coarsest)
    return f.on(ex).generate(a)


def direct():
    return g.Direct.build().with_factorization(g.factorization.Cholesky.build())


def cholesky(m):
    """(nnz(L), levels, generate, numeric alone) of Cholesky on m, each the second of two calls"""
    chol = g.factorization.Cholesky.build()
    chol.on(ex).generate(m)
    fact, t_all = wall(lambda: chol.on(ex).generate(m))
    given = g.factorization.Cholesky.build().with_symbolic_factorization(fact.get_symbolic())
    given.on(ex).generate(m)
    _, t_numeric = wall(lambda: given.on(ex).generate(m))
    lower = g.LowerTrs.build().on(ex).generate(fact.get_l_factor())
    return fact.get_l_factor().get_num_stored_elements(), lower.num_levels, t_all, t_numeric


matrices = {}
for case in cases:
    grid, cut = (int(v) for v in case.split(":"))
    if grid not in matrices:
        matrices[grid] = g.stencil_csr(ex, 3, grid)
    a = matrices[grid]
    sweeps = multigrid(a, cut, None)
    coarse = sweeps.get_mg_level_list()[-1].get_coarse_op()
    n = coarse.size[0]
    print(f"L27({grid}^3), cut {cut}: coarsest {n} rows, nnz {coarse.get_num_stored_elements()};  one V-cycle with "
          f"four sweeps {apply_us(sweeps):9.1f} us", flush=True)
    nnz_l, levels, t_all, t_num = cholesky(coarse)
    t_cycle = apply_us(multigrid(a, cut, direct()))
    print(f"  natural      : nnz(L) {nnz_l:8d}, {levels:5d} levels;  Cholesky.generate {t_all*1e3:9.2f} ms, numeric alone "
          f"{t_num*1e3:9.2f} ms;  V-cycle with Direct {t_cycle:10.1f} us", flush=True)
    for leaf in leaf_sizes:
        nd = g.NestedDissection.build().with_leaf_size(leaf).on(ex)
        g.reorder.NestedDissection(nd, coarse)
        run, t_nd = wall(lambda: g.reorder.NestedDissection(nd, coarse))
        permuted = coarse.permute(run.permutation, "symmetric")
        nnz_l, levels, t_all, t_num = cholesky(permuted)
        wrapped = g.ScaledReordered.build().with_inner_operator(direct()) \
            .with_reordering(g.NestedDissection.build().with_leaf_size(leaf))
        t_cycle = apply_us(multigrid(a, cut, wrapped))
        print(f"  nd, leaf {leaf:4d}: nnz(L) {nnz_l:8d}, {levels:5d} levels;  Cholesky.generate {t_all*1e3:9.2f} ms, numeric "
              f"alone {t_num*1e3:9.2f} ms;  V-cycle with ScaledReordered(Direct) {t_cycle:10.1f} us;  reordering "
              f"{t_nd*1e3:8.2f} ms in {run.rounds} rounds, {run.launches} waited launches "
              f"({t_nd*1e6/max(run.launches, 1):6.1f} us each, regroup and split included)", flush=True)
    del sweeps, coarse
    torch.cuda.synchronize()
