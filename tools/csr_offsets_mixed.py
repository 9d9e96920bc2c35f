"""The plain CSR product on a plan that MIXES narrow and wide segments (csrc/csr_offsets.hpp picks 8, 16, 28 or 32
diagonal slots per plan, from its largest D): 2^22 rows, one 64-row segment in SHARE has the 9 offsets 0 .. 8, the others the
3 offsets 0 .. 2; every segment is eligible.  HIP events, 30 launches per figure, the row-segment kernel
(GKOC_TUNE_CSR_OFFSETS = 2) and the offsets kernel, with the sum of y as a check.
--holes: a structure WITHOUT repetition instead - the band of the 9 offsets 0 .. 8 with every entry kept with
probability 3 / 4, so that no two segments have the same masks and the plan has one class per segment: what the class
ids cost where sharing buys nothing.
usage: python tools/csr_offsets_mixed.py [--share SHARE | --holes] [--lib PATH]      (--lib: as in
tools/csr_offsets_lab.py; a SHARE above the 65536 segments leaves no wide segment: the pure 3-offset plan)
prints one JSON object"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ginkgo_amd as g                      # noqa: E402
from ginkgo_amd import _lib                 # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--share", type=int, default=2)
ap.add_argument("--holes", action="store_true", help="a 9-offset band with random holes: one class per segment")
args = ap.parse_args()
if args.lib:
    _lib.LIB_PATH = os.path.abspath(args.lib)
import csr_offsets_cases as oc              # noqa: E402  (tests/: arena_csr, plan_info)

ex = g.Cdna4Executor.create(0)
n = 1 << 22
if args.holes:
    keep = np.random.default_rng(2).random((n, 9)) < 0.75
    rp = np.zeros(n + 1, np.int64)
    rp[1:] = np.cumsum(keep.sum(axis=1))
    ci = (np.arange(n)[:, None] + np.arange(9)[None, :])[keep].astype(np.int32)
else:
    seg = np.arange(n) // 64
    wide = (seg % args.share) == (args.share - 1)          # one segment in `share` has 9 offsets
    cnt = np.where(wide, 9, 3).astype(np.int64)
    rp = np.zeros(n + 1, np.int64)
    rp[1:] = np.cumsum(cnt)
    row_of = np.repeat(np.arange(n), cnt)
    ci = (row_of + (np.arange(rp[-1]) - rp[row_of])).astype(np.int32)
v = np.random.default_rng(0).uniform(0.5, 1.5, len(ci))
a = oc.arena_csr(ex, (n, n + 16), rp.astype(np.int32), ci, v)
x = g.Dense.from_numpy(ex, np.random.default_rng(1).uniform(-1, 1, n + 16))
y = g.Dense.create(ex, (n, 1))
out = {"lib": "--lib" if args.lib else "tree", "nnz": int(rp[-1]),
       "structure": "band of 9 with holes" if args.holes else "1/%d wide segments" % args.share}
for k, name in ((2, "row_segment_kernel_ms"), (1, "offsets_kernel_ms")):
    _lib.call("gkoc_tune_set", oc.C.c_int(18), oc.C.c_int64(k))
    for _ in range(5):
        a.apply(x, y)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(30):
        a.apply(x, y)
    e1.record()
    torch.cuda.synchronize()
    out[name] = round(e0.elapsed_time(e1) / 30, 5)
    out[name + "_sum"] = float(y.values.double().sum().item())
out["plan"] = oc.plan_info(a)
print(json.dumps(out))
