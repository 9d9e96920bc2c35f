"""ParIc / ParIlu against the level-scheduled Ic / Ilu on the 27-point Laplacian (natural ordering:
7 (g - 1) + 1 levels): the generate time of factorization.Ic / Ilu (the baseline of the same run), the generate
time of ParIc / ParIlu at 1, 3 and 5 sweeps, one sweep next to one CSR SpMV of the same matrix, and the CG
iterations to 1e-10 with LowerIsai on each IC factor.  f64 / int32.  (development / measurement tool)

    python tools/par_factorization_bench.py [grid ...]       default: 64 128
    python tools/par_factorization_bench.py --threshold [grid ...]      default: 64

--threshold prints four rows instead: ParIc / ParIlu (5 sweeps) and ParIct / ParIlut (5 iterations,
fill_in_limit 2.0) with the generate time, the stored entries of the factors, and the iterations to 1e-10 of
CG with Ic + LowerIsai resp. Gmres with Ilu + LowerIsai / UpperIsai ("no convergence" where the solver does not
get there, e.g. with a factor that holds NaN).

generate() is timed as a whole with a host clock around a second, synchronised call: preparation (copy,
diagonal check), factorization and split.  One sweep is the difference of the raw entry at 11 sweeps and at 1
over 10 - the entry's checking pass and its synchronisation drop out - and, next to it, the algorithmic bytes
of a sweep over that time."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import scipy.sparse as sp
import torch

import ginkgo_amd as g
from ginkgo_amd._lib import call

THRESHOLD = "--threshold" in sys.argv
grids = [int(a) for a in sys.argv[1:] if not a.startswith("--")] or ([64] if THRESHOLD else [64, 128])
ex = g.Cdna4Executor.create(0)
REPS = 5


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t


def best(fn, reps=REPS):
    """(last result, the shortest of `reps` timed calls after one warm-up)"""
    fn()
    out, times = None, []
    for _ in range(reps):
        out, t = wall(fn)
        times.append(t)
    return out, min(times)


def apply_us(op, reps):
    b = g.Dense.from_numpy(ex, np.ones(op.size[0]))
    x = g.Dense.create(ex, (op.size[0], 1))
    for _ in range(2):
        op.apply(b, x)
    _, t = wall(lambda: [op.apply(b, x) for _ in range(reps)])
    return t * 1e6 / reps


def cg_iterations(a, fact):
    m = g.Ic.build().with_l_solver(g.LowerIsai.build()).on(ex).generate(fact)
    s = (g.Cg.build()
         .with_criteria(g.stop.Iteration.build().with_max_iters(5000),
                        g.stop.ResidualNorm.build().with_reduction_factor(1e-10))
         .with_generated_preconditioner(m).on(ex).generate(a))
    x = g.Dense.from_numpy(ex, np.zeros(a.size[0]))
    s.apply(g.Dense.from_numpy(ex, np.ones(a.size[0])), x)
    assert s.has_converged
    return s.num_iterations


def sweep_us(entry, m):
    """one sweep of the raw entry on the Csr `m`: (11 sweeps - 1 sweep) / 10"""
    nnz = m.values.numel()
    out, work = ex.alloc((nnz,), m.dtype), ex.alloc((nnz,), m.dtype)

    def run(k):
        return lambda: call(entry, ex.stream, m.size[0], nnz, m.row_ptrs, m.col_idxs, m.values, k, work, out, None)
    return (best(run(11))[1] - best(run(1))[1]) * 1e6 / 10


def lower_triangle(a):
    """the lower triangle of `a` with its diagonal - what the ParIc sweeps start from"""
    host = sp.csr_matrix((a.values.cpu().numpy(), a.col_idxs.cpu().numpy(), a.row_ptrs.cpu().numpy()), shape=a.size)
    low = sp.tril(host, format="csr")
    low.sort_indices()
    return g.Csr.from_arrays(ex, a.size, low.indptr.astype(np.int32), low.indices.astype(np.int32), low.data)


def sweep_bytes(m, lower_only):
    """algorithmic bytes of one sweep, every array once: the row's own values in, the previous sweep's values
    in, the new values out (3 x 8 nnz), columns (4 nnz), row pointers and, for ilu, diagonal positions"""
    n, nnz = m.size[0], m.values.numel()
    return 3 * 8 * nnz + 4 * nnz + 4 * (n + 1) + (0 if lower_only else 4 * n)


def solver_iterations(solver_cls, a, m):
    """iterations to 1e-10 with the generated preconditioner m, or None"""
    s = (solver_cls.build()
         .with_criteria(g.stop.Iteration.build().with_max_iters(2000),
                        g.stop.ResidualNorm.build().with_reduction_factor(1e-10))
         .with_generated_preconditioner(m).on(ex).generate(a))
    x = g.Dense.from_numpy(ex, np.zeros(a.size[0]))
    s.apply(g.Dense.from_numpy(ex, np.ones(a.size[0])), x)
    return s.num_iterations if s.has_converged else None


def threshold_rows(a):
    """ParIc / ParIct and ParIlu / ParIlut side by side"""
    fz = g.factorization
    rows = (("ParIc  (5 sweeps)", lambda: fz.ParIc.build().with_iterations(5), True),
            ("ParIct (5 iterations, limit 2.0)", lambda: fz.ParIct.build().with_iterations(5).with_fill_in_limit(2.0),
             True),
            ("ParIlu (5 sweeps)", lambda: fz.ParIlu.build().with_iterations(5), False),
            ("ParIlut (5 iterations, limit 2.0)",
             lambda: fz.ParIlut.build().with_iterations(5).with_fill_in_limit(2.0), False))
    for label, factory, lower_only in rows:
        try:
            fact, t = best(lambda: factory().on(ex).generate(a), reps=2)
        except g.GkoError as err:
            # ParIct on this stencil: NaN pivots rank above every number, are all kept as ties, and the pattern
            # of L L^T outgrows the device
            print(f"  factorization.{label}: generate FAILED ({str(err).splitlines()[-1][-90:]})", flush=True)
            continue
        if lower_only:
            stored = fact.get_l_factor().get_num_stored_elements()
            finite = bool(torch.isfinite(fact.get_l_factor().values).all().item())
            m = g.Ic.build().with_l_solver(g.LowerIsai.build()).on(ex).generate(fact)
            its, solver = solver_iterations(g.Cg, a, m), "CG + Ic + LowerIsai"
        else:
            stored = fact.get_l_factor().get_num_stored_elements() + fact.get_u_factor().get_num_stored_elements()
            finite = bool(torch.isfinite(fact.get_l_factor().values).all().item()
                          and torch.isfinite(fact.get_u_factor().values).all().item())
            m = (g.Ilu.build().with_l_solver(g.LowerIsai.build()).with_u_solver(g.UpperIsai.build())
                 .on(ex).generate(fact))
            its, solver = solver_iterations(g.Gmres, a, m), "Gmres + Ilu + ISAI"
        print(f"  factorization.{label}: generate {t*1e3:9.2f} ms, {stored} stored entries"
              f"{'' if finite else ' (NOT finite)'};  {solver} "
              f"{'no convergence' if its is None else '%d iterations' % its}", flush=True)
        del fact, m


for grid in grids:
    a = g.stencil_csr(ex, 3, grid)
    if THRESHOLD:
        print(f"L27({grid}^3): n={a.size[0]} nnz={a.get_num_stored_elements()}", flush=True)
        threshold_rows(a)
        del a
        torch.cuda.synchronize()
        continue
    n, nnz = a.size[0], a.get_num_stored_elements()
    t_spmv = apply_us(a, 50)
    print(f"L27({grid}^3): n={n} nnz={nnz}  CSR SpMV {t_spmv:.1f} us", flush=True)
    for name, exact_cls, par_cls, entry in (("Ic", g.factorization.Ic, g.factorization.ParIc, "gkoc_par_ic_sweeps_f64_i32"),
                                            ("Ilu", g.factorization.Ilu, g.factorization.ParIlu,
                                             "gkoc_par_ilu_sweeps_f64_i32")):
        exact, t_exact = best(lambda: exact_cls.build().on(ex).generate(a))
        levels = g.LowerTrs.build().on(ex).generate(exact.get_l_factor()).num_levels
        line = f"  factorization.{name} ({levels} levels): generate {t_exact*1e3:9.2f} ms"
        if name == "Ic":
            line += f";  CG + Ic + LowerIsai {cg_iterations(a, exact):4d} iterations"
        print(line, flush=True)
        for sweeps in (1, 3, 5):
            par, t_par = best(lambda: par_cls.build().with_iterations(sweeps).on(ex).generate(a))
            line = (f"  factorization.Par{name} {sweeps} sweeps: generate {t_par*1e3:9.2f} ms "
                    f"({t_exact/t_par:6.1f} x), last sweep changed {par.last_sweep_changes()} entries")
            if name == "Ic":
                line += f";  CG + Ic + LowerIsai {cg_iterations(a, par):4d} iterations"
            print(line, flush=True)
            del par
        m = lower_triangle(a) if name == "Ic" else a
        t_sweep = sweep_us(entry, m)
        print(f"  one Par{name} sweep ({m.values.numel()} entries): {t_sweep:8.1f} us = {t_sweep/t_spmv:5.2f} CSR SpMV "
              f"of A, {sweep_bytes(m, name == 'Ic')/t_sweep*1e-3:7.1f} GB/s of algorithmic bytes", flush=True)
        del exact, m
    del a
    torch.cuda.synchronize()
