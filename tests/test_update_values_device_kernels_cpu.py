"""The clear and scatter kernels of pg_hip_values_refresh.h (new values from device memory into the device-resident records),
compiled as host C++ behind the shims of tests/hip_emulation_shims.h and run with one thread per work-item
(tests/values_refresh_kernel_emulation.cpp): an arena of three chunks with records of 0, 1, 3, 1000, 16 389 and 65 536 values, slice
boundaries inside records, counts that are no multiple of the 16-byte store, a place at the last value of a chunk and one at the
start of the next, constants, more entries than one grid stride, chunk lengths on the shift and on the division path.  Every value of
the NaN-prefilled value areas equals the serial formula bit for bit and no byte outside them changes.  A check of indexing and
stores that needs no device."""
import os
import subprocess

import pytest

from .helpers import ROOT


@pytest.mark.parametrize("flags", [[], ["-DPANGULU_COMPLEX"]], ids=["real", "complex"])
def test_clear_and_scatter_kernels_against_the_serial_formula(flags, tmp_path):
    exe = str(tmp_path / "emulation")
    subprocess.run(["g++", "-std=c++20", "-O1", "-pthread", "-I", os.path.join(ROOT, "pangulu_amd", "csrc", "platform"),
                    os.path.join(ROOT, "tests", "values_refresh_kernel_emulation.cpp"), "-o", exe] + flags, check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0 and "0 failures OK" in out.stdout, out.stdout
