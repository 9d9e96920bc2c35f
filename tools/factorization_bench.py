"""ILU(0) / IC(0) factorize times on the 27-point Laplacian (natural ordering: 7 (g - 1) + 1 levels) next to
one CSR SpMV of the same matrix, and CG + Ic / Ilu against CG + block-Jacobi(8) as iterations and as time to
the same reduction.  (development / measurement tool)

    python tools/factorization_bench.py [grid ...]       default: 128 256

generate() is timed as a whole with a host clock around a second, synchronised call: the sorted copy, the
host-side level analysis, the factorization kernels and the split (Ic: and the transpose)."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

import ginkgo_amd as g

grids = [int(a) for a in sys.argv[1:] if not a.startswith("--")] or [128, 256]
ex = g.Cdna4Executor.create(0)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t


def spmv_us(a, reps=50):
    b = g.Dense.from_numpy(ex, np.ones(a.size[0]))
    x = g.Dense.create(ex, (a.size[0], 1))
    for _ in range(3):
        a.apply(b, x)
    _, t = wall(lambda: [a.apply(b, x) for _ in range(reps)])
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


for grid in grids:
    a = g.stencil_csr(ex, 3, grid)
    print(f"L27({grid}^3): n={a.size[0]} nnz={a.get_num_stored_elements()}  CSR SpMV {spmv_us(a):.1f} us",
          flush=True)
    for name, fact, prec in (("Ilu", g.factorization.Ilu, g.Ilu), ("Ic", g.factorization.Ic, g.Ic)):
        fact.build().on(ex).generate(a)                 # warm-up: code objects, arena
        f, t = wall(lambda: fact.build().on(ex).generate(a))
        m = prec.build().on(ex).generate(f)
        its, t_cg = cg(a, m)
        print(f"  factorization.{name}.generate {t*1e3:9.1f} ms;  CG + {name}: {its:4d} iterations, "
              f"{t_cg*1e3:9.2f} ms to 1e-10", flush=True)
        del f, m
    jac = g.Jacobi.build().with_max_block_size(8).on(ex).generate(a)
    its, t_cg = cg(a, jac)
    print(f"  CG + block-Jacobi(8): {its:4d} iterations, {t_cg*1e3:9.2f} ms to 1e-10", flush=True)
    del a, jac
    torch.cuda.synchronize()
