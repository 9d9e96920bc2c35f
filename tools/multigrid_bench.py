"""Multigrid over Pgm levels on the 27-point Laplacian: the generate time, the levels and their fill, one
V-cycle next to the CSR SpMV of A, and CG to 1e-10 (right-hand side of ones) with Multigrid (one V-cycle,
defaults), with scalar Jacobi and with Ic + LowerIsai power 1, as iterations and as time.  f64 / int32.
(development / measurement tool)

    python tools/multigrid_bench.py [grid ...]       default: 64 128

generate() is timed as a whole with a host clock around a second, synchronised call.  An application is timed
over `reps` plain launches between two synchronisations, a solve with a host clock around a second,
synchronised apply."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

import ginkgo_amd as g

grids = [int(a) for a in sys.argv[1:] if not a.startswith("--")] or [64, 128]
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


def cg(a, precond, reduction=1e-10):
    s = (g.Cg.build()
         .with_criteria(g.stop.Iteration.build().with_max_iters(5000),
                        g.stop.ResidualNorm.build().with_reduction_factor(reduction))
         .with_generated_preconditioner(precond).on(ex).generate(a))
    rhs = g.Dense.from_numpy(ex, np.ones(a.size[0]))
    x = g.Dense.from_numpy(ex, np.zeros(a.size[0]))
    s.apply(rhs, x)
    x.fill(0.0)
    _, t = wall(lambda: s.apply(rhs, x))
    assert s.has_converged
    return s.num_iterations, t


def multigrid(a):
    return g.Multigrid.build().with_criteria(g.stop.Iteration.build().with_max_iters(1)).on(ex).generate(a)


for grid in grids:
    a = g.stencil_csr(ex, 3, grid)
    nnz = a.get_num_stored_elements()
    print(f"L27({grid}^3): n={a.size[0]} nnz={nnz}  CSR SpMV {apply_us(a, 50):.1f} us", flush=True)
    multigrid(a)                                        # warm-up: code objects, arena
    mg, t_gen = wall(lambda: multigrid(a))
    levels = mg.get_mg_level_list()
    ops = [lv.get_fine_op() for lv in levels] + [levels[-1].get_coarse_op()]
    fill = sum(op.get_num_stored_elements() for op in ops) / nnz
    print(f"  Multigrid.generate {t_gen*1e3:9.1f} ms;  levels (rows) {' -> '.join(str(op.size[0]) for op in ops)};  "
          f"rounds {[lv.rounds for lv in levels]};  sum nnz / nnz(A) = {fill:.3f}", flush=True)
    t_cycle = apply_us(mg, 20)
    its, t_cg = cg(a, mg)
    print(f"  one V-cycle {t_cycle:10.1f} us;  CG + Multigrid(v): {its:4d} iterations, {t_cg*1e3:9.2f} ms to 1e-10",
          flush=True)
    del mg, levels, ops
    jac = g.Jacobi.build().with_max_block_size(1).on(ex).generate(a)
    its, t_cg = cg(a, jac)
    print(f"  CG + scalar Jacobi: {its:4d} iterations, {t_cg*1e3:9.2f} ms to 1e-10", flush=True)
    del jac
    fact = g.factorization.Ic.build().on(ex).generate(a)
    m = g.Ic.build().with_l_solver(g.LowerIsai.build().with_sparsity_power(1)).on(ex).generate(fact)
    its, t_cg = cg(a, m)
    print(f"  CG + Ic + LowerIsai power 1: {its:4d} iterations, {t_cg*1e3:9.2f} ms to 1e-10", flush=True)
    del a, m, fact
    torch.cuda.synchronize()
