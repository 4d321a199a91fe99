"""pangulu_amd_update_values_device on the device: new values as CUDA tensors through pa.update_values and as raw pointers through the
C call.  The two kernels of pg_hip_values_refresh.h write the device-resident records through a map the back-end keeps per handle
(pangulu_platform_0201001_values_refresh); nothing but the nnz values crosses the host link.  Every case first runs pangulu_gstrf, so
the records hold factors and the dense mirrors are in use.  Reference and bounds: tests/update_values_device_common.py (a twin handle
that takes the host path: records equal bit for bit)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pangulu_amd as pa
from pangulu_amd import matrices as M

from . import update_values_device_common as U
from .helpers import ROOT, library_for, max_rel_diff
from .solve_multi_common import open_handle

pytestmark = pytest.mark.gpu


def on_device(values):
    return torch.from_numpy(np.array(values)).cuda()  # (a copy: the shared inputs are read-only)


@pytest.mark.parametrize("name", ["fem27_12_nb64", "shell_40_nb256", "poisson_12_nb32", "cr64_conv12_nb32", "r32_rand1536", "cr32_conv10"])
def test_device_tensor_against_the_host_path(name, monkeypatch):
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
    mat, vtype, nb = U.case(name)
    m2 = U.new_values(name)
    n, cp, ri, va, _ = m2
    want = U.twin_records(name, "hip", va)  # (closed before h opens: a handle's recorded schedule is the back-end's last)
    h = open_handle(mat, nb, "hip", vtype)
    try:
        if name == "shell_40_nb256":
            assert pa.hip_memory(h)["dense_mode_blocks"] > 0
        pa.update_values(h, on_device(va))
        U.assert_records_bit_equal(U.records(h), want)
        info = U.factor_solve_and_compare(h, name, m2, "hip")
        assert info["replayed"] == 1
        U.assert_norms_describe(h, m2)
        # the new system through a right-hand side on the device
        b = M.rhs_of_ones(n, cp, ri, va).astype(va.dtype)
        x = pa.pangulu_gstrs(h, on_device(b))
        assert x.is_cuda
        res = M.relative_residual(n, cp, ri, va, x.cpu().numpy(), b)
        print("%s: residual of the device solve %.3g (%s)" % (name, res, pa.last_solve_path(h)))
        assert res <= U.CHECK_TOL[vtype]
    finally:
        pa.pangulu_finalize(h)


def test_several_arena_chunks():
    """PANGULU_AMD_ARENA_CHUNK_MB is read at pangulu_init: a process of its own with chunks of 1 MiB"""
    code = ("import pangulu_amd as pa; from tests import update_values_device_common as U; from tests.solve_multi_common import open_handle\n"
            "import numpy as np, torch\n"
            "name = 'fem27_12_nb64'; mat, vtype, nb = U.case(name); va = U.new_values(name)[3]\n"
            "want = U.twin_records(name, 'hip', va)\n"
            "h = open_handle(mat, nb, 'hip', vtype)\n"
            "assert h.info()['owned_bytes'] > 2 << 20\n"
            "pa.update_values(h, torch.from_numpy(np.array(va)).cuda())\n"
            "U.assert_records_bit_equal(U.records(h), want)\n"
            "pa.pangulu_gstrf(h); print('chunks OK', pa.factor_check(h) <= 1e-12, h.info()['replayed'])\n"
            "pa.pangulu_finalize(h)")
    env = dict(os.environ, PYTHONPATH=ROOT, PANGULU_AMD_ARENA_CHUNK_MB="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "chunks OK True 1" in out.stdout, (out.stdout[-500:], out.stderr[-1500:])


def test_snapshot_is_retaken_with_the_new_values():
    name = "fem27_12_nb64"
    mat, vtype, nb = U.case(name)
    m2 = U.new_values(name)
    h = open_handle(mat, nb, "hip", vtype, gstrf=False)
    try:
        assert h.lib.pangulu_amd_snapshot(h.ref) == 0
        pa.pangulu_gstrf(h)
        L0, U0 = pa.factors_as_scipy(h)
        pa.update_values(h, on_device(m2[3]))
        pa.pangulu_gstrf(h)
        L1, U1 = pa.factors_as_scipy(h)
        assert h.lib.pangulu_amd_reset_numeric(h.ref) == 0
        pa.pangulu_gstrf(h)
        assert h.info()["replayed"] == 1
        L2, U2 = pa.factors_as_scipy(h)
        check = pa.factor_check(h)  # (against Aperm: the new matrix)
    finally:
        pa.pangulu_finalize(h)
    assert max_rel_diff(U0, U1) > 1e-3  # the two matrices really differ
    assert max_rel_diff(L2, L1) <= 1e-12 and max_rel_diff(U2, U1) <= 1e-12
    assert check <= 1e-12


def test_call_is_ordered_behind_the_callers_stream():
    """The values are produced on a non-default stream by kernels that are still running when the call is made"""
    name = "fem27_12_nb64"
    mat, vtype, nb = U.case(name)
    base = U.new_values(name)[3]
    want = U.twin_records(name, "hip", base * 1.5)
    h = open_handle(mat, nb, "hip", vtype)
    try:
        d_base = on_device(base)
        work = torch.full((2048, 2048), 1.0 / 2048.0, dtype=torch.float64, device="cuda")  # (work @ work == work)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            for _ in range(40):
                work = work @ work
            scale = 1.5 + 0.0 * work[0, 0]  # (known only when the products are done)
            vals = d_base * scale
            pa.update_values(h, vals)
        U.assert_records_bit_equal(U.records(h), want)
    finally:
        pa.pangulu_finalize(h)


def test_refused_pointers_launch_nothing():
    name = "fem27_12_nb64"
    mat, vtype, nb = U.case(name)
    va = np.array(U.new_values(name)[3])
    nnz, isz = len(va), va.dtype.itemsize
    h = open_handle(mat, nb, "hip", vtype)
    try:
        before = U.records(h)
        assert U.raw_update_device(h, va.ctypes.data) == 2  # host memory
        assert U.raw_update_device(h, None) == 2
        # nnz - 1 values at the very end of an allocation: the nnz values the call would read do not lie in device memory.  (A block of
        # 20 MiB is a segment of its own for torch's allocator once its cache is empty.)
        torch.cuda.empty_cache()
        block = torch.zeros(20 << 20, dtype=torch.uint8, device="cuda")
        short = block[block.numel() - (nnz - 1) * isz:].view(torch.float64)
        assert short.numel() == nnz - 1
        seg = [s for s in torch.cuda.memory_snapshot() if s["address"] <= short.data_ptr() < s["address"] + s["total_size"]]
        assert len(seg) == 1 and short.data_ptr() + (nnz - 1) * isz == seg[0]["address"] + seg[0]["total_size"], "test set-up: the tensor does not end its allocation"
        assert U.raw_update_device(h, short.data_ptr()) == 2
        U.assert_records_bit_equal(U.records(h), before)
        assert pa.hip_memory(h)["values_refresh_bytes"] == 0  # (nothing was uploaded either)
        # a tensor on the right device of the wrong type or length never reaches the call
        with pytest.raises(TypeError):
            pa.update_values(h, on_device(va.astype(np.float32)))
        with pytest.raises(ValueError):
            pa.update_values(h, on_device(va[:-1]))
    finally:
        pa.pangulu_finalize(h)


def test_map_stays_on_the_device_until_finalize():
    name = "fem27_12_nb64"
    mat, vtype, nb = U.case(name)
    va = U.new_values(name)[3]
    lib = library_for("hip", vtype)
    h = open_handle(mat, nb, "hip", vtype)
    try:
        assert pa.hip_memory(h)["values_refresh_bytes"] == 0
        pa.update_values(h, on_device(va))
        held = pa.hip_memory(h)["values_refresh_bytes"]
        assert held >= 8 * len(va)  # (one 64-bit destination per user entry at least)
        pa.update_values(h, on_device(va))
        assert pa.hip_memory(h)["values_refresh_bytes"] == held
        pa.pangulu_gstrf(h)
        assert pa.hip_memory(h)["values_refresh_bytes"] == held
    finally:
        pa.pangulu_finalize(h)
    assert pa.hip_memory(lib)["values_refresh_bytes"] == 0
