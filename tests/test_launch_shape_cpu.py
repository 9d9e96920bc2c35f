"""The launch geometry every launcher of the library shares (ginkgo_amd/csrc/launch_shape.hpp) as a host program:
tests/host/launch_shape_test.cpp is compiled with g++, without any ROCm include, and run as a child process.  It
compares capped_grid with the formulas the launchers spelled out before, at every (items per workgroup, cap) pair in
use and at the sizes around one workgroup and around the cap, and checks that with_lanes picks 16 / 32 / 64 lanes at
and next to the limits of a table."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_shape_host_program(tmp_path):
    exe = str(tmp_path / "launch_shape_test")
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "ginkgo_amd", "csrc"),
                            os.path.join(ROOT, "tests", "host", "launch_shape_test.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "launch_shape_test OK" in run.stdout
