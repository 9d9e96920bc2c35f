"""HBM traffic and vector-L1 accesses per launch of the single-column CSR SpMV kernels on the bench matrix, from
`rocprofv3 --pmc` passes of their own (kernel trace only, one counter group per pass) over a short `bench.py` run.
usage: python tools/csr_offsets_pmc.py KEY [GRID]
  KEY = value of GKOC_TUNE_CSR_OFFSETS in the child: 1 = the plan from the first product on (every launch is
  csr_spmv_pipe3_kernel_offsets), 2 = the row-segment kernel csr_spmv_pipe3_kernel alone.
Prints one JSON object: read / written bytes (TCC_EA0 requests by size, as bench.py counts them), L1 accesses."""
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = (("TCC_EA0_RDREQ_sum", "TCC_EA0_RDREQ_32B_sum"), ("TCC_EA0_RDREQ_128B_sum", "TCC_EA0_RDREQ_64B_sum"),
          ("TCC_EA0_WRREQ_sum", "TCC_EA0_WRREQ_64B_sum"), ("TCP_TOTAL_CACHE_ACCESSES_sum", "TCP_TCC_READ_REQ_sum"),
          ("GRBM_GUI_ACTIVE",))


def main():
    key = sys.argv[1]
    grid = sys.argv[2] if len(sys.argv) > 2 else "256"
    want = "csr_spmv_pipe3_kernel_offsets" if key == "1" else "csr_spmv_pipe3_kernel<"
    mean, launches = {}, 0
    tmp = tempfile.mkdtemp(prefix="csr_offsets_pmc_")
    try:
        for i, grp in enumerate(GROUPS):
            out = os.path.join(tmp, f"p{i}")
            cmd = ["rocprofv3", "--pmc", *grp, "--kernel-trace", "--output-format", "csv", "-d", out, "-o", "p", "--",
                   sys.executable, os.path.join(ROOT, "bench.py"), "--grid", grid, "--steps", "4", "--warmup", "2",
                   "--no-pmc"]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=tmp,
                               env=dict(os.environ, GKOC_TUNE_18=key))
            files = glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True)
            if p.returncode != 0 or not files:
                print(json.dumps({"error": f"pass {i} failed", "stderr": p.stderr[-400:]}))
                return 1
            acc = {}
            for row in csv.DictReader(open(files[0])):
                if want in row.get("Kernel_Name", ""):
                    acc.setdefault(row["Counter_Name"], []).append(float(row["Counter_Value"]))
            for c in grp:
                if acc.get(c):
                    mean[c] = sum(acc[c]) / len(acc[c])
                    launches = len(acc[c])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    res = {"key": int(key), "kernel": want, "launches_per_pass": launches,
           "counters_mean_per_launch": {k: round(v, 1) for k, v in mean.items()}}
    try:
        r128, r64, rall = mean["TCC_EA0_RDREQ_128B_sum"], mean["TCC_EA0_RDREQ_64B_sum"], mean["TCC_EA0_RDREQ_sum"]
        w64, wall = mean["TCC_EA0_WRREQ_64B_sum"], mean["TCC_EA0_WRREQ_sum"]
        rd = r128 * 128 + r64 * 64 + max(rall - r128 - r64, 0.0) * 32
        wr = w64 * 64 + max(wall - w64, 0.0) * 32
        res.update(hbm_read_bytes=int(rd), hbm_write_bytes=int(wr), hbm_bytes_per_launch=int(rd + wr))
    except KeyError:
        pass
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
