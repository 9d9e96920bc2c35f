"""Level-scheduled triangular solves and the Sor / SSOR preconditioner on the 27-point Laplacian
(natural ordering: 7 (g - 1) + 1 levels).  Per grid size: levels, launches, W and the set-up time
of the analysis; us per lower and upper solve next to the CSR SpMV of the SAME triangle in the same
run and next to launches x the time of a minimal launch; CG + SSOR(1) against CG + block-Jacobi(8)
as iterations and as time to the same reduction.  (development / measurement tool)

    python tools/trs_bench.py [grid ...]       default: 128 256

The triangles are the factors of Sor(1, symmetric): L = D + L_A, U = D^-1 (D + U_A) - the
pattern of A's triangles with the diagonal.  Times are device events around `reps` calls after a
warm-up; the CG times are a host clock around a second, synchronised solve."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

import ginkgo_amd as g
from ginkgo_amd import _lib

grids = [int(a) for a in sys.argv[1:] if not a.startswith("--")] or [128, 256]
ex = g.Cdna4Executor.create(0)


def timeit(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps      # us


def minimal_launch_us(count=2000):
    """back-to-back launches of a one-element fill, replayed from a call tape (no Python work per call)"""
    one = g.Dense.create(ex, (1, 1))
    with _lib.record() as tape:
        for _ in range(count):
            one.fill(0.0)
    return timeit(tape.replay, 5) / count


def cg(a, precond, reduction=1e-10):
    s = (g.Cg.build()
         .with_criteria(g.stop.Iteration.build().with_max_iters(5000),
                        g.stop.ResidualNorm.build().with_reduction_factor(reduction))
         .with_generated_preconditioner(precond).on(ex).generate(a))
    n = a.size[0]
    rhs = g.Dense.from_numpy(ex, np.ones(n))
    x = g.Dense.from_numpy(ex, np.zeros(n))
    s.apply(rhs, x)
    torch.cuda.synchronize()
    x.fill(0.0)
    torch.cuda.synchronize()
    t = time.perf_counter()
    s.apply(rhs, x)
    torch.cuda.synchronize()
    t = time.perf_counter() - t
    assert s.has_converged
    return s.num_iterations, t


launch_us = minimal_launch_us()
print(f"minimal launch, back to back: {launch_us:.2f} us", flush=True)
for grid in grids:
    a = g.stencil_csr(ex, 3, grid)
    n = a.size[0]
    torch.cuda.synchronize()
    t = time.perf_counter()
    m = g.Sor.build().with_relaxation_factor(1.0).with_symmetric(True).on(ex).generate(a)
    torch.cuda.synchronize()
    t_sor = time.perf_counter() - t
    print(f"L27({grid}^3): n={n} nnz={a.get_num_stored_elements()}  Sor(1, symmetric).generate "
          f"{t_sor*1e3:.0f} ms (factors + both analyses)", flush=True)
    b = g.Dense.from_numpy(ex, np.random.default_rng(3).uniform(-1, 1, n))
    x = g.Dense.create(ex, (n, 1))
    for name, tri, cls in (("lower", m.l, g.LowerTrs), ("upper", m.u, g.UpperTrs)):
        torch.cuda.synchronize()
        t = time.perf_counter()
        s = cls.build().on(ex).generate(tri)
        torch.cuda.synchronize()
        t_gen = time.perf_counter() - t
        reps = 20 if grid <= 128 else 5
        t_solve = timeit(lambda: s.apply(b, x), reps)
        t_spmv = timeit(lambda: tri.apply(b, x), 50)
        print(f"  {name}: {s.num_levels} levels, {s.num_launches} launches, W={s.wide_threshold}, "
              f"generate {t_gen*1e3:.0f} ms (host analysis); solve {t_solve:.1f} us, CSR SpMV of the same "
              f"triangle {t_spmv:.1f} us, launches x minimal launch {s.num_launches*launch_us:.1f} us",
              flush=True)
    del b, x
    it_s, t_s = cg(a, m)
    print(f"  CG + SSOR(1):          {it_s:4d} iterations, {t_s*1e3:9.2f} ms to 1e-10", flush=True)
    del m
    jac = g.Jacobi.build().with_max_block_size(8).on(ex).generate(a)
    it_j, t_j = cg(a, jac)
    print(f"  CG + block-Jacobi(8):  {it_j:4d} iterations, {t_j*1e3:9.2f} ms to 1e-10", flush=True)
    print(f"  faster: {'SSOR' if t_s < t_j else 'block-Jacobi(8)'} ({max(t_s, t_j)/min(t_s, t_j):.2f} x)",
          flush=True)
    del a, jac
    torch.cuda.synchronize()
