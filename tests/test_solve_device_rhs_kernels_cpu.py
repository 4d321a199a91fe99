"""The pack / unpack kernels of pg_hip_solve_pack.h (right-hand sides on the device: the user's column-major matrix <-> one panel of
the solve kernels, through the handle's index/scale maps), compiled as host C++ behind the shims of tests/hip_emulation_shims.h and
run with one thread per work-item (tests/solve_device_rhs_kernel_emulation.cpp): every panel width, n no multiple of the workgroup,
fewer columns than the panel is wide, a panel that starts past column 0, ldb = n + 5, padding rows, with and without scale arrays.
Every value of the NaN-prefilled panel is defined after the pack and equals the formula bit for bit; the unpack changes nothing but
the rows it is told to; identity maps and unit scales give the input back.  A check of indexing and arithmetic that needs no device."""
import os
import subprocess

import pytest

from .helpers import ROOT


@pytest.mark.parametrize("flags", [[], ["-DPANGULU_COMPLEX"]], ids=["real", "complex"])
def test_pack_and_unpack_kernels_against_their_formulas(flags, tmp_path):
    exe = str(tmp_path / "emulation")
    subprocess.run(["g++", "-std=c++20", "-O1", "-pthread", "-I", os.path.join(ROOT, "pangulu_amd", "csrc", "platform"),
                    os.path.join(ROOT, "tests", "solve_device_rhs_kernel_emulation.cpp"), "-o", exe] + flags, check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0 and "0 failures OK" in out.stdout, out.stdout
