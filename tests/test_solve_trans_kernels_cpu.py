"""The transposed sweeps of pg_hip_block_solve_multi.h (A^T X = B, A^H X = B), compiled as host C++ behind shims for the few device intrinsics
they use and run with one thread per work-item (tests/solve_trans_kernel_emulation.cpp), against dense substitution with U^T / L^T
(U^H / L^H): every panel width, both sweeps, real and complex values, conjugation on and off, block orders that are a multiple of
nothing, several chunks per diagonal half, an empty row record and a row of U whose only entry is a diagonal below the clamp.  A
check of indexing and arithmetic that needs no device."""
import os
import subprocess

import pytest

from .helpers import ROOT


@pytest.mark.parametrize("flags", [[], ["-DPANGULU_COMPLEX"]], ids=["real", "complex"])
def test_transposed_panel_kernels_against_dense_substitution(flags, tmp_path):
    exe = str(tmp_path / "emulation")
    subprocess.run(["g++", "-std=c++20", "-O1", "-pthread", "-I", os.path.join(ROOT, "pangulu_amd", "csrc", "platform"),
                    os.path.join(ROOT, "tests", "solve_trans_kernel_emulation.cpp"), "-o", exe] + flags, check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout
