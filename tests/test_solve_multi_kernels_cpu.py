"""The kernels of pg_hip_block_solve_multi.h, compiled as host C++ behind shims for the few device intrinsics they use and run
with one thread per work-item (tests/solve_multi_kernel_emulation.cpp), against dense substitution: every panel width, both sweeps,
real and complex values.  A check of indexing and arithmetic that needs no device.  The W = 1 instances are the kernels every
pangulu_gstrs on the HIP path launches (a single vector is a panel of width 1), so this is the device-free test of the default
single-vector solve as well."""
import os
import subprocess

import pytest

from .helpers import ROOT


@pytest.mark.parametrize("flags", [[], ["-DPANGULU_COMPLEX"]], ids=["real", "complex"])
def test_panel_kernels_against_dense_substitution(flags, tmp_path):
    exe = str(tmp_path / "emulation")
    subprocess.run(["g++", "-std=c++20", "-O1", "-pthread", "-I", os.path.join(ROOT, "pangulu_amd", "csrc", "platform"),
                    os.path.join(ROOT, "tests", "solve_multi_kernel_emulation.cpp"), "-o", exe] + flags, check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout
