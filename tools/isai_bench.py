"""Triangular ISAI on the IC(0) factor of the 27-point Laplacian (natural ordering: 7 (g - 1) + 1 levels): the
generate time for the sparsity powers 1 and 2, one application of Ic with the level-scheduled solvers
(LowerTrs / UpperTrs) against Ic with the ISAI solvers (two CSR SpMVs), and CG with both as iterations and as
time to the same reduction; and SpdIsai (powers 1 and 2) and GeneralIsai (power 1) of the system matrix itself,
which need no factorization: generate, nnz(W), one application, CG.  f64 / int32.  (development / measurement
tool)

    python tools/isai_bench.py [grid ...]       default: 64 128

generate() is timed as a whole with a host clock around a second, synchronised call (power 2: the pattern
through the triplet pipeline included).  An application is timed over `reps` plain launches between two
synchronisations."""
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


def cg(a, precond, reduction=1e-10, must_converge=True):
    s = (g.Cg.build()
         .with_criteria(g.stop.Iteration.build().with_max_iters(5000),
                        g.stop.ResidualNorm.build().with_reduction_factor(reduction))
         .with_generated_preconditioner(precond).on(ex).generate(a))
    rhs = g.Dense.from_numpy(ex, np.ones(a.size[0]))
    x = g.Dense.from_numpy(ex, np.zeros(a.size[0]))
    s.apply(rhs, x)
    x.fill(0.0)
    _, t = wall(lambda: s.apply(rhs, x))
    assert s.has_converged or not must_converge
    return s.num_iterations if s.has_converged else -1, t


for grid in grids:
    a = g.stencil_csr(ex, 3, grid)
    print(f"L27({grid}^3): n={a.size[0]} nnz={a.get_num_stored_elements()}  CSR SpMV {apply_us(a, 50):.1f} us",
          flush=True)
    fact = g.factorization.Ic.build().on(ex).generate(a)
    lower = fact.get_l_factor()
    trs = g.Ic.build().on(ex).generate(fact)
    t_apply = apply_us(trs, 5)
    its, t_cg = cg(a, trs)
    print(f"  Ic + LowerTrs / UpperTrs ({trs.get_l_solver().num_levels} levels, "
          f"{trs.get_l_solver().num_launches} launches per solve): apply {t_apply:10.1f} us;  "
          f"CG {its:4d} iterations, {t_cg*1e3:9.2f} ms to 1e-10", flush=True)
    del trs
    for power in (1, 2):
        def isai():
            return g.LowerIsai.build().with_sparsity_power(power).on(ex).generate(lower)
        isai()                                          # warm-up: code objects, arena
        w, t_gen = wall(isai)
        nnz = w.get_approximate_inverse().get_num_stored_elements()
        del w
        m = g.Ic.build().with_l_solver(g.LowerIsai.build().with_sparsity_power(power)).on(ex).generate(fact)
        t_apply = apply_us(m, 50)
        its, t_cg = cg(a, m)
        print(f"  LowerIsai power {power}: generate {t_gen*1e3:9.1f} ms, nnz(W) = {nnz};  Ic + ISAI: apply "
              f"{t_apply:10.1f} us;  CG {its:4d} iterations, {t_cg*1e3:9.2f} ms to 1e-10", flush=True)
        del m
    for cls, power in ((g.SpdIsai, 1), (g.SpdIsai, 2), (g.GeneralIsai, 1)):
        def dense_solve_isai():
            return cls.build().with_sparsity_power(power).on(ex).generate(a)
        dense_solve_isai()                              # warm-up: code objects, arena
        m, t_gen = wall(dense_solve_isai)
        nnz = m.get_approximate_inverse().get_num_stored_elements()
        t_apply = apply_us(m, 50)
        # W of GeneralIsai is not symmetric: CG with it is shown for comparison, -1 = not converged
        its, t_cg = cg(a, m, must_converge=cls is g.SpdIsai)
        print(f"  {cls.__name__} power {power}: generate {t_gen*1e3:9.1f} ms, nnz(W) = {nnz};  apply "
              f"{t_apply:10.1f} us;  CG {its:4d} iterations, {t_cg*1e3:9.2f} ms to 1e-10", flush=True)
        del m
    jac = g.Jacobi.build().with_max_block_size(1).on(ex).generate(a)
    its, t_cg = cg(a, jac)
    print(f"  CG + scalar Jacobi: {its:4d} iterations, {t_cg*1e3:9.2f} ms to 1e-10", flush=True)
    del a, jac, fact, lower
    torch.cuda.synchronize()
