"""The mechanism of the two CSR structure caches (ginkgo_amd/csrc/structure_cache.hpp, used by csr_structure.hip) as
a host program: tests/host/structure_cache_test.cpp is compiled with g++ and run as a child process.  It checks
that the oldest ARRIVAL makes room however often it was looked up, that erase_if hands back exactly the matching
entries and the count follows, and that with four threads under the callers' discipline (look up and insert under
the lock, release after unlocking) every entry is handed back exactly once or is still cached at the end."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_structure_cache_host_program(tmp_path):
    exe = str(tmp_path / "structure_cache_test")
    build = subprocess.run(["g++", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "ginkgo_amd", "csrc"),
                            os.path.join(ROOT, "tests", "host", "structure_cache_test.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "structure_cache_test OK" in run.stdout
