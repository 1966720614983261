"""h-slam_amd/csrc/hs_host.h's allocation owner where every HIP allocation fails (no device): tests/c/host_pool_main.cpp
is built against the library and run.  With a device visible the allocations succeed and tests/test_gpu_lifetime.py
checks the counts instead."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "h-slam_amd", "lib")


def test_pool_failure_paths_without_a_device(tmp_path):
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if has_gpu:
        pytest.skip("a HIP device is visible: allocations do not fail (tests/test_gpu_lifetime.py covers the counts)")
    if not os.path.exists(os.path.join(LIBDIR, "libhslam_amd.so")):
        subprocess.run(["make", "-C", os.path.join(ROOT, "h-slam_amd", "csrc")], check=True, capture_output=True)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = tmp_path / "host_pool_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                    os.path.join(ROOT, "tests", "c", "host_pool_main.cpp"), "-o", str(exe),
                    "-L", LIBDIR, "-lhslam_amd", "-Wl,-rpath," + LIBDIR,
                    "-L", os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(rocm, "lib")],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 checks failed" in r.stdout
