"""pangulu_amd_gstrs_device: right-hand sides that already live on the device, as torch tensors through pa.pangulu_gstrs_multi and as
a raw device pointer through the C call.  Nothing passes through the host: pack kernel, the panel sweeps, unpack kernel
(pg_hip_solve_pack.h, pangulu_platform_0201001_block_trsm_multi_device) on a workspace the back-end keeps per handle.  Every case is
compared with SuperLU (tests/solve_trans_common.py) and with the host-pointer call of the same handle within TOL of
tests/solve_multi_common.py per column (the atomics' summation order differs from call to call: no bit-equality between the paths)."""
import ctypes

import numpy as np
import pytest
import torch

import pangulu_amd as pa
from pangulu_amd import _lib
from pangulu_amd import matrices as M

from . import slots
from .helpers import library_for
from .solve_trans_common import (TOL, assert_trans_columns_match, open_handle, relative_difference, rhs_block, scaled_saddle, splu_columns,
                                 transposed_residual)
from .test_gpu_solve_trans import case
from .test_solve_device_rhs import raw_gstrs_device

pytestmark = pytest.mark.gpu


def on_device(B):
    """B as a (row-major) tensor on the device"""
    return torch.from_numpy(np.array(B, order="C")).cuda()  # (a copy: the shared inputs are read-only)


def column_major(T):
    return T.t().contiguous().t()


@pytest.mark.parametrize("name,nb,trans,nrhs", [
    ("r64_conv10", 64, "N", 4), ("r64_conv10", 64, "T", 4),
    ("r64_conv14", 128, "T", 19),   # panels of 16 + 4
    ("cr64_conv12", 128, "H", 9),   # two panels of 8
    ("r32_rand1536", 64, "N", 7),
    ("cr32_conv10", 64, "H", 4),
])
def test_device_tensor_against_host_pointer_call_and_splu(name, nb, trans, nrhs, monkeypatch):
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
    mat, vtype, B = case(name)
    assert B.shape[1] == nrhs
    n = B.shape[0]
    ref = splu_columns(name, mat, B, trans)
    what = "%s nb=%d trans=%s nrhs=%d" % (name, nb, trans, nrhs)
    h = open_handle(mat, nb, "hip", vtype)
    try:
        Xh = pa.pangulu_gstrs_multi(h, B, trans=trans)
        path_h = pa.last_solve_path(h)
        T = on_device(B)
        keep = T.clone()
        X = pa.pangulu_gstrs_multi(h, T, trans=trans)  # (row-major in: one strided copy)
        path_d = pa.last_solve_path(h)
        Xc = pa.pangulu_gstrs_multi(h, column_major(T), trans=trans)  # (column-major in: one clone)
        x3 = pa.pangulu_gstrs(h, T[:, 3].contiguous(), trans=trans)
        assert h.info()["time_solve"] > 0
    finally:
        pa.pangulu_finalize(h)
    assert path_h["device_columns"] == nrhs and path_d == path_h, (path_d, path_h)
    for Y in (X, Xc):
        assert isinstance(Y, torch.Tensor) and Y.device == T.device and Y.dtype == T.dtype
        assert tuple(Y.shape) == (n, nrhs) and Y.stride() == (1, n)
    assert torch.equal(T, keep)  # the input is not modified
    X, Xc = X.cpu().numpy(), Xc.cpu().numpy()
    assert_trans_columns_match(X, ref, B, vtype, what + ", device tensor against splu")  # (the zero column exactly zero; the unit column: cross-talk)
    assert_trans_columns_match(X, Xh, B, vtype, what + ", device tensor against the host-pointer call")
    assert_trans_columns_match(Xc, ref, B, vtype, what + ", column-major device tensor against splu")
    assert tuple(x3.shape) == (n,) and x3.is_cuda
    assert_trans_columns_match(x3.cpu().numpy()[:, None], ref[:, 3:4], B[:, 3:4], vtype, what + ", one vector")


@pytest.mark.parametrize("trans", ["N", "T"])
def test_scaled_handle(trans, monkeypatch):
    """matching + scaling through the maps on the device; for T they swap roles"""
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
    mat = scaled_saddle()
    n, cp, ri, va, _ = mat
    B = rhs_block(mat, 3)
    h = open_handle(mat, 32, "hip", "r64", scaling=True)
    try:
        Xh = pa.pangulu_gstrs_multi(h, B, trans=trans)
        X = pa.pangulu_gstrs_multi(h, on_device(B), trans=trans)
        path = pa.last_solve_path(h)
        other = pa.pangulu_gstrs_multi(h, on_device(B), trans="T" if trans == "N" else "N").cpu().numpy()
    finally:
        pa.pangulu_finalize(h)
    X = X.cpu().numpy()
    assert path["device_columns"] == 3
    assert not X[:, 1].any()
    A = M.to_scipy(n, cp, ri, va)
    for j in (0, 2):
        res = transposed_residual(mat, X[:, j], B[:, j], "T") if trans == "T" else float(np.linalg.norm(A @ X[:, j] - B[:, j]) / np.linalg.norm(B[:, j]))
        print("trans=%s column %d: ||op(A) x - b|| / ||b|| = %.3g" % (trans, j, res))
        assert res <= 1e-10, (j, res)
    assert_trans_columns_match(X, Xh, B, "r64", "scaled saddle trans=%s, device tensor against the host-pointer call" % trans)
    assert relative_difference(X, other) > 1e-3


def test_raw_call_with_a_leading_dimension(monkeypatch):
    """the C call on a buffer of the back-end's own allocator, ldb = n + 5: the five spare rows of each column survive; a host
    pointer is refused on the host (2) before any launch"""
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
    mat, vtype, B = case("r64_conv10")
    n, nrhs = B.shape
    ref = splu_columns("r64_conv10", mat, B, "T")
    h = open_handle(mat, 64, "hip", vtype)
    f = slots.declare_platform(h.lib, "0201001")
    dev = ctypes.c_void_p()
    try:
        buf = np.full((n + 5, nrhs), -777.25, order="F")
        buf[:n] = B
        before = buf.copy(order="F")
        f("malloc")(ctypes.byref(dev), buf.nbytes)
        f("memcpy")(dev, buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes, 0)
        assert raw_gstrs_device(h, buf.ctypes.data_as(ctypes.c_void_p), nrhs, n + 5, 1) == 2  # host memory
        assert (buf == before).all()
        assert raw_gstrs_device(h, dev, 0, n + 5, 1) == 0
        assert raw_gstrs_device(h, dev, nrhs, n - 1, 1) == 2
        assert raw_gstrs_device(h, dev, nrhs, n + 5, 7) == 3
        out = np.empty_like(buf, order="F")
        f("memcpy")(out.ctypes.data_as(ctypes.c_void_p), dev, buf.nbytes, 1)
        assert (out == before).all()  # none of those touched the buffer
        assert raw_gstrs_device(h, dev, nrhs, n + 5, 1) == 0  # (stream NULL: the legacy default stream)
        assert pa.last_solve_path(h) == {"device_columns": nrhs, "panel_width": 4, "panels": 1}
        f("memcpy")(out.ctypes.data_as(ctypes.c_void_p), dev, buf.nbytes, 1)
    finally:
        if dev:
            f("free")(dev)
        pa.pangulu_finalize(h)
    assert (out[n:] == -777.25).all()
    assert_trans_columns_match(out[:n], ref, B, vtype, "raw call, ldb = n + 5")


def test_workspace_lifetime(monkeypatch):
    """the workspace is built once, dropped by update_values / gstrf and by finalize; the back-end's memory figures say so"""
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
    mat, vtype, B = case("r64_conv10")
    n, cp, ri, va, coords = mat
    va2 = va * (1.0 + 0.05 * np.cos(np.arange(len(va))))  # same pattern, every entry moved by up to 5 %
    mat2 = (n, cp, ri, va2, coords)
    lib = library_for("hip", vtype)
    pa.pangulu_finalize(open_handle(mat, 64, "hip", vtype))  # (what the back-end keeps from handle to handle is there after this one)
    m0 = pa.hip_memory(lib)
    assert m0["solve_workspace_bytes"] == 0
    h = open_handle(mat, 64, "hip", vtype)
    try:
        T = on_device(B)
        X1 = pa.pangulu_gstrs_multi(h, T)
        X2 = pa.pangulu_gstrs_multi(h, T)
        m2 = pa.hip_memory(h)
        X3 = pa.pangulu_gstrs_multi(h, T)
        m3 = pa.hip_memory(h)
        assert m2["solve_workspace_bytes"] > 0 and m3 == m2, (m2, m3)
        pa.update_values(h, va2)
        assert pa.hip_memory(h)["solve_workspace_bytes"] == 0
        pa.pangulu_gstrf(h)
        X4 = pa.pangulu_gstrs_multi(h, T)
        assert pa.last_solve_path(h)["device_columns"] == B.shape[1]
        assert pa.hip_memory(h)["solve_workspace_bytes"] == m2["solve_workspace_bytes"]
        Xh = pa.pangulu_gstrs_multi(h, B)
    finally:
        pa.pangulu_finalize(h)
    assert pa.hip_memory(lib) == m0, (pa.hip_memory(lib), m0)
    X1, X2, X3, X4 = (x.cpu().numpy() for x in (X1, X2, X3, X4))
    for X in (X1, X2, X3):
        assert_trans_columns_match(X, splu_columns("r64_conv10", mat, B, "N"), B, vtype, "first factorisation")
    assert_trans_columns_match(X4, splu_columns("r64_conv10_new_values", mat2, B, "N"), B, vtype, "after update_values")
    assert_trans_columns_match(Xh, X4, B, vtype, "host-pointer call after all that")
    assert relative_difference(X4[:, 0], X1[:, 0]) > 1e-3  # (the two systems do differ)


def test_ordered_behind_the_callers_stream(monkeypatch):
    """B is still being computed on a stream of the caller's when the solve is called: the solve waits for it on the device"""
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
    mat, vtype, B = case("r64_conv10")
    h = open_handle(mat, 64, "hip", vtype)
    try:
        B0 = on_device(B)
        W = torch.rand(4096, 4096, device="cuda", dtype=torch.float32)

        def produce():
            Z = W
            for _ in range(6):  # tens of milliseconds of work ahead of the chain that makes B
                Z = (Z @ W) * (1.0 / 4096)
            T = B0 + 0.0 * Z[0, 0].double()
            for k in range(20):
                T = T * 1.5 - B0 * 0.5 if k % 2 == 0 else (T + B0 * 0.5) / 1.5
            return T

        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            T1 = produce()
            s.synchronize()
            X1 = pa.pangulu_gstrs_multi(h, T1)
            T2 = produce()
            X2 = pa.pangulu_gstrs_multi(h, T2)  # no host synchronisation in between
        torch.cuda.synchronize()
    finally:
        pa.pangulu_finalize(h)
    assert torch.equal(T1, T2)
    X1, X2 = X1.cpu().numpy(), X2.cpu().numpy()
    assert_trans_columns_match(X2, X1, T1.cpu().numpy(), vtype, "unsynchronised producer against the synchronised one")
    assert_trans_columns_match(X2, splu_columns("r64_conv10", mat, B, "N"), B, "r32", "the chain gives B back up to rounding")


def test_no_device_path_from_python(monkeypatch):
    """PANGULU_AMD_DEVICE_SOLVE=0 (read per call): return code 4, the wrapper stages through the host and still hands back a device tensor"""
    mat, vtype, B = case("r64_conv10")
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
    h = open_handle(mat, 64, "hip", vtype)
    try:
        T = on_device(B)
        monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "0")
        Tc = column_major(T)
        assert raw_gstrs_device(h, ctypes.c_void_p(Tc.data_ptr()), B.shape[1], B.shape[0], 1) == 4
        assert torch.equal(Tc, T)
        X = pa.pangulu_gstrs_multi(h, T, trans="T")
        path = pa.last_solve_path(h)
    finally:
        pa.pangulu_finalize(h)
    assert isinstance(X, torch.Tensor) and X.is_cuda and tuple(X.shape) == B.shape
    assert path["device_columns"] == 0
    assert_trans_columns_match(X.cpu().numpy(), splu_columns("r64_conv10", mat, B, "T"), B, vtype, "staged through the host")
