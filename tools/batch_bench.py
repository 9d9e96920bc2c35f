"""Batched Bicgstab + scalar Jacobi to a relative residual of 1e-8, f64: time per batch solve and systems per
second for batch.Csr and batch.Ell, against the two routes the single-system classes offer:
  (a) a Python loop of ginkgo_amd.Bicgstab + Jacobi(1) solves over the items - timed on the first `--loop-items`
      items and scaled to the batch;
  (b) ONE ginkgo_amd.Bicgstab + Jacobi(1) solve of the block-diagonal assembly of all items (it runs until the
      norm of the WHOLE residual has dropped by 1e-8, every item as long as the slowest) - up to 2^24 rows.
Workloads: the per-item perturbed 3-point stencil at n = 64, 256, 1024 and the 5-point stencil on 16^2 and 32^2,
2^10 ... 2^16 items.  (development / measurement tool)

    python tools/batch_bench.py [--items 1024,65536] [--workloads tri64,tri256,tri1024,five16,five32]
                                [--reps 5] [--loop-items 16] [--no-baselines] [--json PATH]

The values are made on the device from a seed (base stencil x (1 + 0.2 u), u uniform in [0, 1), which keeps the
items diagonally dominant).  A batch solve is timed with device events around the one library call, x reset
outside the timed window, the median of `reps` after a warm-up; the baselines with a host clock around a
synchronised solve."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import scipy.sparse as sp
import torch

import ginkgo_amd as g
from ginkgo_amd import batch

ap = argparse.ArgumentParser()
ap.add_argument("--items", default=",".join(str(2 ** k) for k in range(10, 17)))
ap.add_argument("--workloads", default="tri64,tri256,tri1024,five16,five32")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--loop-items", type=int, default=16)
ap.add_argument("--no-baselines", action="store_true")
ap.add_argument("--json", default=None)
args = ap.parse_args()
ex = g.Cdna4Executor.create(0)
TOL, MAX_IT = 1e-8, 500
BLOCK_DIAGONAL_ROWS = 2 ** 24


def pattern(name):
    """the base stencil as scipy CSR: dominance 2.5 / 4.5 on the diagonal, -1 beside it"""
    if name.startswith("tri"):
        n = int(name[3:])
        a = sp.diags([-1.0, 2.5, -1.0], [-1, 0, 1], shape=(n, n))
    else:
        m = int(name[4:])
        one = sp.diags([-1.0, 0.0, -1.0], [-1, 0, 1], shape=(m, m))
        a = sp.kron(sp.identity(m), one) + sp.kron(one, sp.identity(m)) + 4.5 * sp.identity(m * m)
    a = a.tocsr()
    a.sort_indices()
    return a


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t


def single_solver(a):
    return (g.Bicgstab.build()
            .with_criteria(g.stop.Iteration.build().with_max_iters(MAX_IT),
                           g.stop.ResidualNorm.build().with_reduction_factor(TOL))
            .with_preconditioner(g.Jacobi.build().with_max_block_size(1)).on(ex).generate(a))


def batch_time(a, b, reps):
    s = (batch.Bicgstab.build().with_max_iterations(MAX_IT).with_tolerance(TOL).with_tolerance_type("relative")
         .with_preconditioner(batch.Jacobi.build()).on(ex).generate(a))
    x = batch.MultiVector.create(ex, a.num_items, (a.size[0], 1))
    times = []
    for rep in range(reps + 1):                         # the first one warms up
        x.values.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        s.apply(b, x)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3)
    it = s.iteration_counts.cpu().numpy()
    assert bool(s.converged.all().item()), "an item did not converge"
    return statistics.median(times[1:]), int(it.min()), int(it.max()), s.plan


def loop_time(a, b, count):
    """(a): one generate and one solve per item, as a user of the single-system classes writes it"""
    n = a.size[0]
    def run():
        for i in range(count):
            s = single_solver(a.create_view_for_item(i))
            x = g.Dense.from_numpy(ex, np.zeros(n))
            s.apply(b.create_view_for_item(i), x)
    run()
    _, t = wall(run)
    return t / count


def block_diagonal_time(a, b):
    """(b): the block-diagonal matrix of all items, assembled on the device from the batch arrays"""
    items, n, nnz = a.num_items, a.size[0], a.get_num_stored_elements_per_item()
    item = torch.arange(items, device=ex.device, dtype=torch.int32)[:, None]
    ptrs = torch.cat([torch.zeros(1, dtype=torch.int32, device=ex.device),
                      (a.row_ptrs[None, 1:] + nnz * item).reshape(-1)])
    cols = (a.col_idxs[None, :] + n * item).reshape(-1)
    big = g.Csr(ex, (items * n, items * n), a.values.reshape(-1), cols.contiguous(), ptrs.contiguous())
    s = single_solver(big)
    rhs = g.Dense(ex, b.values.reshape(items * n, 1))
    x = g.Dense.from_numpy(ex, np.zeros(items * n))
    s.apply(rhs, x)
    x.fill(0.0)
    _, t = wall(lambda: s.apply(rhs, x))
    assert s.has_converged
    return t, s.num_iterations


results = []
for name in args.workloads.split(","):
    base = pattern(name)
    n, nnz = base.shape[0], base.nnz
    for items in (int(v) for v in args.items.split(",")):
        gen = torch.Generator(device=ex.device).manual_seed(1000 + items)
        scale = 1 + 0.2 * torch.rand((items, nnz), generator=gen, device=ex.device, dtype=torch.float64)
        values = scale * torch.from_numpy(base.data).to(ex.device)[None, :]
        csr = batch.Csr(ex, base.shape, values, ex.to_device(base.indices.astype(np.int32)),
                        ex.to_device(base.indptr.astype(np.int32)))
        b = batch.MultiVector(ex, torch.rand((items, n, 1), generator=gen, device=ex.device, dtype=torch.float64))
        row = {"workload": name, "n": n, "nnz": nnz, "items": items}
        for fmt, a in (("csr", csr), ("ell", csr.convert_to_ell())):
            t, lo, hi, p = batch_time(a, b, args.reps)
            row[fmt] = {"seconds": t, "systems_per_second": items / t, "iterations": [lo, hi],
                        "resident_vectors": p.resident_vectors, "values_cached": p.values_cached,
                        "lds_bytes": p.lds_bytes}
            del a
        if not args.no_baselines:
            row["loop_seconds"] = loop_time(csr, b, min(args.loop_items, items)) * items
        if not args.no_baselines and items * n <= BLOCK_DIAGONAL_ROWS:
            row["block_diagonal_seconds"], row["block_diagonal_iterations"] = block_diagonal_time(csr, b)
        results.append(row)
        bd = row.get("block_diagonal_seconds")
        print(f"{name:8s} n={n:5d} items={items:6d}: Csr {row['csr']['seconds']*1e3:9.3f} ms "
              f"({row['csr']['systems_per_second']:.3e} systems/s), Ell {row['ell']['seconds']*1e3:9.3f} ms "
              f"({row['ell']['systems_per_second']:.3e} systems/s), iterations {row['csr']['iterations']}, "
              f"LDS {row['csr']['lds_bytes']} B, {row['csr']['resident_vectors']} vectors resident; (a) loop, scaled "
              + (f"{row['loop_seconds']*1e3:11.1f} ms" if "loop_seconds" in row else "not measured")
              + "; (b) block diagonal "
              + (f"{bd*1e3:9.3f} ms, {row['block_diagonal_iterations']} iterations" if bd else "not measured"),
              flush=True)
        del csr, b, values, scale
        torch.cuda.synchronize()
if args.json:
    with open(args.json, "w") as f:
        json.dump(results, f, indent=1)
