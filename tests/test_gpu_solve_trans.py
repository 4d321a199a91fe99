"""pangulu_amd_gstrs_trans on the device: A^T X = B and A^H X = B in panels through pangulu_platform_0201001_block_trsm_multi_trans
(pg_hip_block_solve_trans.h) on the factors of A where they lie.  Every case is compared with SuperLU's transposed solve and with
the host sweep of the same handle on the same factors, within TOL of tests/solve_multi_common.py per column; the inputs are
unsymmetric (tests/solve_trans_common.py), and every case shows that T, N and H give different answers."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import pangulu_amd as pa
from pangulu_amd import _lib

from . import slots
from .solve_trans_common import (TOL, assert_trans_columns_match, assert_trans_is_honoured, conv, open_handle, rand, relative_difference,
                                 rhs_block, scaled_saddle, splu_columns, transposed_residual)
from .test_gpu_solve_multi import _SolveRow, _SolveSweep

pytestmark = pytest.mark.gpu

INPUTS = {
    # name: (vtype, generator, columns of the case's right-hand sides)
    "r64_conv14": ("r64", lambda dt: conv(14, dt), 19),
    "r64_rand3000": ("r64", lambda dt: rand(3000, 0.002, dt), 5),
    "cr64_conv12": ("cr64", lambda dt: conv(12, dt), 9),
    "cr64_rand1536": ("cr64", lambda dt: rand(1536, 0.004, dt), 5),
    "r32_rand1536": ("r32", lambda dt: rand(1536, 0.004, dt), 7),
    "cr32_conv10": ("cr32", lambda dt: conv(10, dt), 4),
    "r64_conv10": ("r64", lambda dt: conv(10, dt), 4),
}
_mats = {}


def case(name):
    vtype, gen, ncol = INPUTS[name]
    if name not in _mats:
        mat = gen(_lib.VALUE_TYPES[vtype][0])
        B = rhs_block(mat, ncol)
        B.setflags(write=False)
        _mats[name] = (mat, B)
    mat, B = _mats[name]
    return mat, vtype, B


def device_then_host(h, B, trans, monkeypatch):
    """the transposed solve on the device, what it reports, and the host sweep of the same handle on the same factors"""
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
    X = pa.pangulu_gstrs_multi(h, B, trans=trans)
    path = pa.last_solve_path(h)
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "0")
    Xh = pa.pangulu_gstrs_multi(h, B, trans=trans)
    assert pa.last_solve_path(h)["device_columns"] == 0
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
    return X, path, Xh


# (nrhs, widest panel, panels): a tile row is at most 128 bytes -- 16 real values, 8 double-complex ones; a panel is as wide as the
# smallest power of two that holds the columns left, at most that
@pytest.mark.parametrize("name,nb,trans,nrhs,width,panels", [
    ("r64_conv14", 128, "T", 1, 1, 1), ("r64_conv14", 128, "T", 3, 4, 1), ("r64_conv14", 128, "T", 19, 16, 2),
    ("r64_conv14", 256, "T", 16, 16, 1),
    ("r64_rand3000", 64, "T", 5, 8, 1),
    ("cr64_conv12", 128, "T", 9, 8, 2), ("cr64_conv12", 128, "H", 9, 8, 2),
    ("cr64_conv12", 256, "H", 8, 8, 1),
    ("cr64_rand1536", 64, "H", 5, 8, 1),
    ("r32_rand1536", 64, "T", 7, 8, 1),
    ("cr32_conv10", 64, "H", 4, 4, 1),
])
def test_transposed_block_solve(name, nb, trans, nrhs, width, panels, monkeypatch):
    mat, vtype, B = case(name)
    ref = splu_columns(name, mat, B, trans)[:, :nrhs]
    B = B[:, :nrhs]
    what = "%s nb=%d trans=%s nrhs=%d" % (name, nb, trans, nrhs)
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
    h = open_handle(mat, nb, "hip", vtype)
    try:
        X, path, Xh = device_then_host(h, B, trans, monkeypatch)
        assert path == {"device_columns": nrhs, "panel_width": width, "panels": panels}, path
        assert_trans_columns_match(X, ref, B, vtype, what + ", device against splu")
        assert_trans_columns_match(X, Xh, B, vtype, what + ", device against the host sweep")
        assert_trans_is_honoured(h, B, X, trans)
    finally:
        pa.pangulu_finalize(h)


def test_scaled_handle(monkeypatch):
    """matching + scaling swap roles: dc and the matching go onto b, dr onto x"""
    mat = scaled_saddle()
    B = rhs_block(mat, 3)
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
    h = open_handle(mat, 32, "hip", "r64", scaling=True)
    try:
        X, path, Xh = device_then_host(h, B, "T", monkeypatch)
        XN = pa.pangulu_gstrs_multi(h, B)
    finally:
        pa.pangulu_finalize(h)
    assert path["device_columns"] == 3
    assert not X[:, 1].any()
    for j in (0, 2):
        res = transposed_residual(mat, X[:, j], B[:, j], "T")
        print("column %d: ||A^T x - b|| / ||b|| = %.3g" % (j, res))
        assert res <= 1e-10, (j, res)
    assert_trans_columns_match(X, Xh, B, "r64", "scaled saddle, device against the host sweep")
    assert relative_difference(X, XN) > 1e-3


def test_second_factorisation_on_the_same_handle(monkeypatch):
    """update_values + gstrf keep the cached transposed plans: the second solve is that of the NEW matrix"""
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
    mat, vtype, B = case("r64_conv10")
    n, cp, ri, va, coords = mat
    va2 = va * (1.0 + 0.05 * np.cos(np.arange(len(va))))  # same pattern, every entry moved by up to 5 %
    mat2 = (n, cp, ri, va2, coords)
    h = open_handle(mat, 64, "hip", vtype)
    try:
        X1 = pa.pangulu_gstrs_multi(h, B, trans="T")
        pa.update_values(h, va2)
        pa.pangulu_gstrf(h)
        X2 = pa.pangulu_gstrs_multi(h, B, trans="T")
        path = pa.last_solve_path(h)
    finally:
        pa.pangulu_finalize(h)
    assert path["device_columns"] == B.shape[1]
    assert_trans_columns_match(X1, splu_columns("r64_conv10", mat, B, "T"), B, vtype, "first factorisation")
    assert_trans_columns_match(X2, splu_columns("r64_conv10_new_values", mat2, B, "T"), B, vtype, "after update_values")
    assert relative_difference(X2[:, 0], X1[:, 0]) > 1e-3  # (the two systems do differ)


def _trans_level_plan(bm, forward):
    """One transposed sweep as the operator takes it: segment i with the upper (forward, U^T) / lower (backward, L^T) diagonal half and
    the blocks (k, i) of its block COLUMN, k < i / k > i, whose block rows k are the source segments; levels by those dependencies."""
    nbk = bm.nblk
    side = {i: sorted(k for (k, c, _) in bm.blocks if c == i and (k < i if forward else k > i)) for i in range(nbk)}
    level = [0] * nbk
    for i in (range(nbk) if forward else reversed(range(nbk))):
        level[i] = 1 + max((level[k] for k in side[i]), default=-1)
    nlevel = 1 + max(level)
    order = sorted(range(nbk), key=lambda i: (level[i], i))
    level_ptr = (ctypes.c_uint64 * (nlevel + 1))(*np.concatenate(([0], np.cumsum(np.bincount(level, minlength=nlevel)))).tolist())
    nblk = sum(len(v) for v in side.values())
    rows = (_SolveRow * nbk)()
    blk_slots = (ctypes.POINTER(slots.Slot) * max(nblk, 1))()
    blk_bcol = (ctypes.c_uint32 * max(nblk, 1))()
    j = 0
    for pos, i in enumerate(order):
        rows[pos].brow, rows[pos].nblk, rows[pos].first = i, len(side[i]), j
        rows[pos].diag = ctypes.pointer(bm.blocks[(i, i, 1 if forward else 0)].slot)
        for k in side[i]:
            blk_slots[j] = ctypes.pointer(bm.get(k, i).slot)
            blk_bcol[j] = k
            j += 1
    return _SolveSweep(nlevel, level_ptr, rows, blk_slots, blk_bcol)


def _declare_trans_operator(hip):
    f = hip.pangulu_platform_0201001_block_trsm_multi_trans
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_uint16, ctypes.POINTER(_SolveSweep), ctypes.POINTER(_SolveSweep), ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64,
                  ctypes.c_uint64, ctypes.POINTER(ctypes.c_int)]
    return f


def test_backend_operator_called_directly():
    """block_trsm_multi_trans with one panel of width 1 on hand-built slots of the oracle's factor records: SuperLU's solution of
    A^T x = b in the factors' ordering (no scaling: z[i] = x[perm[i]], padding rows 0)."""
    mat, vtype, B = case("r64_conv10")
    nb, n = 64, mat[0]
    ref = splu_columns("r64_conv10", mat, B, "T")
    hip = _lib.load(vtype)
    hip.pangulu_amd_use_builtin_platform()
    slots.declare_platform(hip, "0201001")
    hip.pangulu_platform_0201001_set_default_device(0)
    recs, perm = slots.exported_records(mat, nb, vtype, factorise=True)
    bm = slots.BlockMatrix(recs, nb, np.float64, hip)
    try:
        xlen = bm.nblk * nb
        real = perm < n  # (the others are padding rows: 1 * x = 0)
        b = np.zeros(xlen)
        want = np.zeros(xlen)
        b[:len(perm)][real] = B[perm[real], 3]  # the seeded random column
        want[:len(perm)][real] = ref[perm[real], 3]
        sw = [_trans_level_plan(bm, True), _trans_level_plan(bm, False)]
        multi_trans = _declare_trans_operator(hip)
        x = b.copy()
        assert multi_trans(nb, None, None, 0, None, 0, 0, None) == 16  # (npanel = 0 only asks)
        assert multi_trans(nb, ctypes.byref(sw[0]), ctypes.byref(sw[1]), 0, x.ctypes.data_as(ctypes.c_void_p), xlen, 1, (ctypes.c_int * 1)(1)) == 16
    finally:
        bm.free()
    err = np.abs(x - want).max() / np.abs(want).max()
    print("block_trsm_multi_trans, one panel of width 1: max |dx| / max |x| = %.3g" % err)
    assert err <= TOL[vtype], err


def test_host_sweep_where_the_operator_is_not_offered(tmp_path):
    """PANGULU_HIP_SOLVE_CHUNKED=0 leaves the column-by-column kernels, which have no transposed twin: the operator returns 0 and the
    public call answers through the host sweep (a process of its own: the switch is read once)"""
    mat, vtype, B = case("r64_conv10")
    out = str(tmp_path / "out.npz")
    env = dict(os.environ, PANGULU_HIP_SOLVE_CHUNKED="0", PANGULU_AMD_DEVICE_SOLVE="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    run = subprocess.run([sys.executable, os.path.join(root, "tests", "solve_trans_by_column_worker.py"), "r64_conv10", "64", "3", out], env=env,
                         cwd=root, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    z = np.load(out)
    assert int(z["operator_widest_panel"]) == 0
    assert int(z["device_columns"]) == 0
    assert int(z["untransposed_device_columns"]) == 3  # (the untransposed solve of the same process still runs on the device)
    assert_trans_columns_match(z["X"], splu_columns("r64_conv10", mat, B, "T")[:, :3], B[:, :3], vtype, "host sweep under SOLVE_CHUNKED=0")
