"""factorization.Cholesky and the Direct solver as coarsest solver of Multigrid on the 27-point Laplacian: per
cut-off (with_min_coarse_rows) the coarsest operator, the generate time of Cholesky on it - as a whole, with the
pattern given, which leaves the numeric phase (gather, level schedule, factorization, transpose), and the symbolic
phase alone (the class's own two steps: the symmetrised lower triangle, then forest, walks and the triplet
pipeline) - the fill, the levels of the lower solve, and one V-cycle and CG to 1e-10 with Direct against the
built-in four sweeps at the same cut-off.  f64 / int32.  (development / measurement tool)

    python tools/direct_bench.py [grid ...] [--cut=rows,rows,...]       default: 64 128, --cut=500,1000,2000

Timing as in tools/multigrid_bench.py: a host clock around a second, synchronised call; an application over
`reps` plain launches between two synchronisations."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

import ginkgo_amd as g

grids = [int(a) for a in sys.argv[1:] if not a.startswith("--")] or [64, 128]
cuts = [500, 1000, 2000]
for arg in sys.argv[1:]:
    if arg.startswith("--cut="):
        cuts = [int(c) for c in arg[6:].split(",")]
ex = g.Cdna4Executor.create(0)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t


def apply_us(op, reps):
    b = g.Dense.from_numpy(ex, np.ones(op.size[0]))
    x = g.Dense.create(ex, (op.size[0], 1))
    for _ in range(2):
        op.apply(b, x)
    _, t = wall(lambda: [op.apply(b, x) for _ in range(reps)])
    return t * 1e6 / reps


def cg(a, precond):
    s = (g.Cg.build()
         .with_criteria(g.stop.Iteration.build().with_max_iters(5000),
                        g.stop.ResidualNorm.build().with_reduction_factor(1e-10))
         .with_generated_preconditioner(precond).on(ex).generate(a))
    rhs = g.Dense.from_numpy(ex, np.ones(a.size[0]))
    x = g.Dense.from_numpy(ex, np.zeros(a.size[0]))
    s.apply(rhs, x)
    x.fill(0.0)
    _, t = wall(lambda: s.apply(rhs, x))
    assert s.has_converged
    return s.num_iterations, t


def multigrid(a, cut, direct):
    f = g.Multigrid.build().with_criteria(g.stop.Iteration.build().with_max_iters(1)).with_min_coarse_rows(cut)
    if direct:
        f = f.with_coarsest_solver(g.Direct.build().with_factorization(g.factorization.Cholesky.build()))
    return f.on(ex).generate(a)


for grid in grids:
    a = g.stencil_csr(ex, 3, grid)
    print(f"L27({grid}^3): n={a.size[0]} nnz={a.get_num_stored_elements()}", flush=True)
    for cut in cuts:
        sweeps = multigrid(a, cut, False)
        levels = sweeps.get_mg_level_list()
        coarse = levels[-1].get_coarse_op()
        chol = g.factorization.Cholesky.build()
        chol.on(ex).generate(coarse)                    # warm-up: code objects, arena
        fact, t_all = wall(lambda: chol.on(ex).generate(coarse))
        given = g.factorization.Cholesky.build().with_symbolic_factorization(fact.get_symbolic())
        given.on(ex).generate(coarse)
        _, t_numeric = wall(lambda: given.on(ex).generate(coarse))
        # the coarse operator is sorted and stores every diagonal, so it is its own prepared copy
        _, t_symbolic = wall(lambda: fact._symbolic_cholesky(*fact._symmetrized_lower(coarse)))
        lower = g.LowerTrs.build().on(ex).generate(fact.get_l_factor())
        nnz_l, nnz_a = fact.get_l_factor().get_num_stored_elements(), coarse.get_num_stored_elements()
        print(f"  cut {cut:5d}: {len(levels) + 1} levels, coarsest {coarse.size[0]} rows, nnz {nnz_a}, nnz(L) {nnz_l} "
              f"({nnz_l / nnz_a:.1f} x), {lower.num_levels} levels in {lower.num_launches} launches;  Cholesky.generate "
              f"{t_all*1e3:8.2f} ms, numeric alone {t_numeric*1e3:8.2f} ms, symbolic alone {t_symbolic*1e3:8.2f} ms",
              flush=True)
        del fact, given, lower
        direct = multigrid(a, cut, True)
        t_sweeps, t_direct = apply_us(sweeps, 20), apply_us(direct, 20)
        its_s, cg_s = cg(a, sweeps)
        its_d, cg_d = cg(a, direct)
        print(f"             one V-cycle: sweeps {t_sweeps:9.1f} us, Direct {t_direct:9.1f} us;  CG to 1e-10: sweeps "
              f"{its_s} iterations {cg_s*1e3:8.2f} ms, Direct {its_d} iterations {cg_d*1e3:8.2f} ms", flush=True)
        del sweeps, direct, levels, coarse
    del a
    torch.cuda.synchronize()
