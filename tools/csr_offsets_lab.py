"""The column-offset plan of the CSR SpMV (csrc/csr_offsets.hpp) measured in ONE process on the same buffers,
27-pt stencil of GRID^3 rows (default 256), HIP events, 30 launches per figure:
  * the row-segment kernel (GKOC_TUNE_CSR_OFFSETS = 2) against the offsets kernel, plain product and the fused
    <b, c> entry (gkoc_x_csr_spmv_dot_*; its c and dot must have the same bits either way);
  * the cost of the analysis: the second product from entry to return and to completion;
  * the stencil with every other segment made ineligible (an unsorted row): plan + row-segment kernel in one
    product against the row-segment kernel alone - the "at least half of the segments" rule of csr_structure.hip.
A variant of the kernel that is not in the tree (a step of a change kept apart to be measured, say) is a second
library built from a copy of the sources: --lib PATH loads that one instead of ginkgo_amd/lib, --only-kernels
skips the analysis and the half-eligible matrix.  Two libraries cannot share one process' buffers, so such runs are
taken alternately, a process each, on the same matrix and vectors (same seeds).
usage: python tools/csr_offsets_lab.py [GRID] [--lib PATH] [--only-kernels]      prints one JSON object"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ginkgo_amd as g                      # noqa: E402
from ginkgo_amd import _lib                 # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("grid", nargs="?", type=int, default=256)
ap.add_argument("--lib", default=None, help="libgko_cdna4.so to load instead of the tree's")
ap.add_argument("--only-kernels", action="store_true", help="the four kernel timings and the bit check only")
args = ap.parse_args()
if args.lib:
    _lib.LIB_PATH = os.path.abspath(args.lib)

KEY = 18
ex = g.Cdna4Executor.create(0)


def tune(v):
    _lib.call("gkoc_tune_set", C.c_int(KEY), C.c_int64(v))


def info(a):
    st, el, ns, by, pr = C.c_int(-9), C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
    _lib.call("gkoc_csr_plan_info", C.c_void_p(a.row_ptrs.data_ptr()), C.c_void_p(a.col_idxs.data_ptr()),
              C.byref(st), C.byref(el), C.byref(ns), C.byref(by), C.byref(pr))
    return dict(state=st.value, eligible=el.value, segments=ns.value, bytes=by.value, products=pr.value)


def timed(step, reps=30, warm=5):
    for _ in range(warm):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def wall(step):
    torch.cuda.synchronize()
    t = time.perf_counter()
    step()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t) * 1e3, (time.perf_counter() - t) * 1e3


grid = args.grid
n = grid ** 3
out = {"grid": grid, "lib": _lib.LIB_PATH if args.lib else "tree"}
a = g.stencil_csr(ex, 3, grid)
x = g.Dense.from_numpy(ex, np.random.default_rng(1).uniform(-1, 1, n))
y = g.Dense.create(ex, (n, 1))
dot = g.Dense.create(ex, (1, 1))
nbytes = _lib.lib().gkoc_x_workspace_bytes(C.c_int64(n), C.c_size_t(8))
work = ex.alloc(((nbytes + 7) // 8,), torch.float64)
plain = lambda: a.apply(x, y)                         # noqa: E731
fused = lambda: a.apply_dot(x, y, dot, work)          # noqa: E731

tune(2)
out["row_segment_kernel_ms"] = timed(plain)
out["row_segment_kernel_fused_dot_ms"] = timed(fused)
old_bits = (y.values.clone().view(torch.int64), dot.values.clone().view(torch.int64))
tune(0)
if args.only_kernels:
    plain()
    plain()
else:
    out["first_product_ms(entry_to_return, to_completion)"] = wall(plain)
    out["second_product_with_analysis_ms(entry_to_return, to_completion)"] = wall(plain)
out["plan"] = info(a)
out["offsets_kernel_ms"] = timed(plain)
out["offsets_kernel_fused_dot_ms"] = timed(fused)
out["fused_dot_same_bits"] = bool(torch.equal(y.values.view(torch.int64), old_bits[0]) and
                                  torch.equal(dot.values.view(torch.int64), old_bits[1]))
tune(2)
out["row_segment_kernel_again_ms"] = timed(plain)
out["row_segment_kernel_fused_dot_again_ms"] = timed(fused)
tune(0)
out["offsets_kernel_again_ms"] = timed(plain)
out["offsets_kernel_fused_dot_again_ms"] = timed(fused)
if args.only_kernels:
    print(json.dumps(out, indent=1))
    sys.exit(0)

# every other segment made ineligible: the first two entries of its first row swapped (an unsorted row)
b = g.stencil_csr(ex, 3, grid)
rp = b.row_ptrs[64::128].long()
for arr in (b.col_idxs, b.values):
    first, second = arr[rp].clone(), arr[rp + 1].clone()
    arr[rp], arr[rp + 1] = second, first
torch.cuda.synchronize()
half = lambda: b.apply(x, y)                          # noqa: E731
tune(2)
out["half_eligible_row_segment_kernel_ms"] = timed(half)
y_old = y.values.clone()
tune(1)
out["half_eligible_plan_two_kernels_ms"] = timed(half)
out["half_eligible_plan"] = info(b)
out["half_eligible_same_bits"] = bool(torch.equal(y.values.view(torch.int64), y_old.view(torch.int64)))
tune(0)
print(json.dumps(out, indent=1))
