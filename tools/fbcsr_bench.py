"""Fbcsr (fixed-block CSR) against CSR and SELL-P on the configs[4] stand-in A = L27(g^3) (x) B,
g = 80 (n = 1 536 000 for 3 x 3 blocks, 13.5 M blocks): one line per format with us per product,
GB/s on the format's own byte model and % of 8 TB/s; CG + block-Jacobi(3) us/it and it/s with
the CSR and the Fbcsr system matrix; the Fbcsr product must be bit-identical to the CSR one.
Also L27 (x) B2, L27 (x) B4 (f64) and the f32 Fbcsr<3>.  (development / measurement tool)

The block matrix is built on the device from L27 (every block = l27(i, j) B), the CSR from it by
Fbcsr.convert_to_csr - the sorted CSR of the Kronecker product, entry for entry.

    python tools/fbcsr_bench.py [grid]              everything above
    python tools/fbcsr_bench.py [grid] --spmv-only  the f64 L27 (x) B3 products alone, 5 each (the
                                                    command of the counter passes, tools/pmc_groups.sh)"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

import ginkgo_amd as g
from ginkgo_amd.executor import MEM_VALUES

args = [a for a in sys.argv[1:] if not a.startswith("--")]
grid = int(args[0]) if args else 80
spmv_only = "--spmv-only" in sys.argv
ex = g.Cdna4Executor.create(0)
l27 = g.stencil_csr(ex, 3, grid)
BLOCKS = {
    2: np.array([[2.0, 0.5], [0.5, 1.5]]),
    3: np.array([[4.0, 1.0, 0.5], [1.0, 3.0, 0.25], [0.5, 0.25, 2.0]]),
    4: np.array([[4.0, 1.0, 0.5, 0.25], [1.0, 3.0, 0.25, 0.5], [0.5, 0.25, 2.0, 0.125],
                 [0.25, 0.5, 0.125, 2.5]]),
}


REPS = 5 if spmv_only else 50


def timeit(fn, reps=REPS):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def line(name, ms, nbytes):
    gbs = nbytes / ms / 1e6
    print(f"{name:40s} {ms*1e3:9.1f} us  {gbs:8.1f} GB/s ({100*gbs/8000:5.1f} % of 8 TB/s)", flush=True)


def block_matrix(bs, dtype):
    b = torch.tensor(BLOCKS[bs].T.reshape(-1), dtype=dtype, device=ex.device)   # column-major block
    vals = ex.alloc((l27.values.numel() * bs * bs,), dtype, MEM_VALUES)
    vals.view(-1, bs * bs).copy_(l27.values.to(dtype)[:, None] * b[None, :])
    n = l27.size[0] * bs
    return g.Fbcsr(ex, (n, n), bs, vals, l27.col_idxs, l27.row_ptrs)


def case(bs, dtype, sellp, cg):
    fb = block_matrix(bs, dtype)
    csr = fb.convert_to_csr()
    n, nnz, nb = fb.size[0], fb.get_num_stored_elements(), fb.get_num_stored_blocks()
    vs = 8 if dtype == torch.float64 else 4
    tag = "f64" if dtype == torch.float64 else "f32"
    print(f"L27({grid}^3) (x) B{bs} {tag}/i32: n={n} nnz={nnz} blocks={nb} ({nnz/n:.1f}/row)", flush=True)
    x = g.Dense.from_numpy(ex, np.random.default_rng(1).uniform(-1, 1, n).astype(
        np.float64 if dtype == torch.float64 else np.float32))
    y1, y2 = g.Dense.create(ex, (n, 1), dtype), g.Dense.create(ex, (n, 1), dtype)
    csr.apply(x, y1)
    fb.apply(x, y2)
    torch.cuda.synchronize()
    assert torch.equal(y1.values, y2.values), "Fbcsr product differs from the CSR product"
    t_csr = timeit(lambda: csr.apply(x, y1))
    line(f"  CSR SpMV", t_csr, (vs + 4) * nnz + 4 * (n + 1) + 2 * vs * n)
    best = t_csr
    if sellp:
        sl = csr.convert_to_sellp()
        stored = sl.values.numel()
        t_sl = timeit(lambda: sl.apply(x, y1))
        line(f"  SELL-P SpMV (stored {stored/nnz:.3f} x nnz)", t_sl, (vs + 4) * stored + 2 * vs * n)
        best = min(best, t_sl)
        del sl
    t_fb = timeit(lambda: fb.apply(x, y2))
    line(f"  Fbcsr<{bs}> SpMV", t_fb, vs * nnz + 4 * nb + 4 * (n // bs + 1) + 2 * vs * n)
    print(f"  Fbcsr<{bs}> / faster of the others: {t_fb/best:.3f}", flush=True)
    if cg:
        prec = g.Jacobi.build().with_max_block_size(bs).on(ex).generate(csr)
        its = {}
        for name, op in (("CSR", csr), (f"Fbcsr<{bs}>", fb)):
            s = (g.Cg.build()
                 .with_criteria(g.stop.Iteration.build().with_max_iters(200),
                                g.stop.ResidualNorm.build().with_reduction_factor(1e-30))
                 .with_generated_preconditioner(prec).on(ex).generate(op))
            rhs = g.Dense.from_numpy(ex, np.ones(n))
            sol = g.Dense.from_numpy(ex, np.zeros(n))
            s.apply(rhs, sol)
            torch.cuda.synchronize()
            sol.fill(0.0)
            t = time.perf_counter()
            s.apply(rhs, sol)
            torch.cuda.synchronize()
            t = time.perf_counter() - t
            its[name] = s.num_iterations / t
            print(f"  CG + block-Jacobi({bs}) on {name:9s}: {s.num_iterations} its, "
                  f"{t*1e6/s.num_iterations:8.1f} us/it, {s.num_iterations/t:8.1f} it/s", flush=True)
        print(f"  CG it/s Fbcsr / CSR: {its[f'Fbcsr<{bs}>'] / its['CSR']:.3f}  (both stop at 200 iterations: "
              f"reduction 1e-30)", flush=True)
        # the iteration counts of a real solve: 1e-8, the Csr without the fused spmv + dot (whose dot
        # sums in another order) - the same iterations and the same x bit for bit
        res = []
        for op, fused in ((csr, False), (fb, True)):
            s = (g.Cg.build()
                 .with_criteria(g.stop.Iteration.build().with_max_iters(5000),
                                g.stop.ResidualNorm.build().with_reduction_factor(1e-8))
                 .with_generated_preconditioner(prec).with_fused_spmv_dot(fused).on(ex).generate(op))
            sol = g.Dense.from_numpy(ex, np.zeros(n))
            s.apply(g.Dense.from_numpy(ex, np.ones(n)), sol)
            torch.cuda.synchronize()
            res.append((s.num_iterations, s.has_converged, sol.values.clone()))
        assert res[0][1] and res[1][1] and res[0][0] == res[1][0], (res[0][:2], res[1][:2])
        assert torch.equal(res[0][2], res[1][2])
        print(f"  CG + block-Jacobi({bs}) to 1e-8: {res[0][0]} iterations on both, x bit-identical", flush=True)
    del fb, csr
    torch.cuda.synchronize()


case(3, torch.float64, sellp=True, cg=not spmv_only)
if not spmv_only:
    case(3, torch.float32, sellp=False, cg=False)
    case(2, torch.float64, sellp=False, cg=False)
    case(4, torch.float64, sellp=False, cg=False)
