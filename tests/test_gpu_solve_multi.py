"""pangulu_amd_gstrs_multi on the device: panels of right-hand sides through pangulu_platform_0201001_block_trsm_multi
(pg_hip_block_solve_multi.h).  Column j of the block solve must be what pangulu_gstrs gives for that column alone -- the oracle
library's and the HIP path's own -- within the bounds of test_device_solve_matches_host_sweep.  pangulu_gstrs on the HIP path is
the same solve with one panel of width 1 (same kernels, same launch routine, same cached plans): the tests at the end hold it
across a refactorisation, call the two back-end operators directly, and send width-1 panels through the column-by-column kernels."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import pangulu_amd as pa
from pangulu_amd import _lib
from pangulu_amd import matrices as M

from . import slots
from .solve_multi_common import TOL, assert_columns_match, open_handle, oracle_columns, raw_gstrs_multi, rhs_block, solve_columns

pytestmark = pytest.mark.gpu

CASES = {
    # name: (vtype, generator, nb, columns of the case's reference)
    "r64_shell40": ("r64", lambda dt: M.shell(40, 40, dtype=dt), 256, 19),  # n = 9 600: padding rows, 38 block rows
    "r64_kkt8": ("r64", lambda dt: M.kkt(8, dtype=dt), 64, 5),
    "cr64_poisson12": ("cr64", lambda dt: M.poisson3d(12, dtype=dt, shift=0.5j), 128, 9),
    "r32_fem27_10": ("r32", lambda dt: M.fem27(10, dtype=dt), 64, 7),
    "cr32_poisson10": ("cr32", lambda dt: M.poisson3d(10, dtype=dt, shift=0.5j), 64, 4),
}
_mats = {}


def case(name):
    """matrix, nb, vtype, the case's right-hand sides and the oracle's column-by-column solutions (made once, read-only)"""
    vtype, gen, nb, ncol = CASES[name]
    if name not in _mats:
        mat = gen(_lib.VALUE_TYPES[vtype][0])
        B = rhs_block(mat, ncol)
        B.setflags(write=False)
        _mats[name] = (mat, B)
    mat, B = _mats[name]
    return mat, nb, vtype, B, oracle_columns(name, mat, nb, vtype, B)


# (nrhs, widest panel, panels): a tile row is at most 128 bytes -- 16 real values, 8 double-complex ones; a panel is as wide as the
# smallest power of two that holds the columns left, at most that
@pytest.mark.parametrize("name,nrhs,width,panels", [
    ("r64_shell40", 1, 1, 1), ("r64_shell40", 3, 4, 1), ("r64_shell40", 16, 16, 1), ("r64_shell40", 19, 16, 2),
    ("r64_kkt8", 5, 8, 1),
    ("cr64_poisson12", 5, 8, 1), ("cr64_poisson12", 9, 8, 2),
    ("r32_fem27_10", 7, 8, 1),
    ("cr32_poisson10", 4, 4, 1),
])
def test_block_solve_matches_single_vector_solves(name, nrhs, width, panels, monkeypatch):
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
    mat, nb, vtype, B, ref = case(name)
    B, ref = B[:, :nrhs], ref[:, :nrhs]
    h = open_handle(mat, nb, "hip", vtype)
    try:
        X = pa.pangulu_gstrs_multi(h, B)
        path = pa.last_solve_path(h)
        own = solve_columns(h, B)
    finally:
        pa.pangulu_finalize(h)
    assert path == {"device_columns": nrhs, "panel_width": width, "panels": panels}, path
    assert_columns_match(X, ref, B, vtype, "against the oracle")
    assert_columns_match(X, own, B, vtype, "against pangulu_gstrs on the HIP path")


def test_leading_dimension_and_memory_order(monkeypatch):
    """ldb = n + 5: the slack rows keep their sentinel; the binding takes B in either memory order"""
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
    mat, nb, vtype, B, ref = case("r64_kkt8")
    n, nrhs = B.shape
    h = open_handle(mat, nb, "hip", vtype)
    try:
        buf = np.full((n + 5, nrhs), -777.25, dtype=B.dtype, order="F")
        buf[:n] = B
        assert raw_gstrs_multi(h, buf, nrhs, n + 5) == 0
        Xc = pa.pangulu_gstrs_multi(h, np.ascontiguousarray(B))
        Xf = pa.pangulu_gstrs_multi(h, np.asfortranarray(B))
    finally:
        pa.pangulu_finalize(h)
    assert (buf[n:] == -777.25).all()
    assert_columns_match(buf[:n], ref, B, vtype, "ldb = n + 5")
    assert_columns_match(Xc, ref, B, vtype, "C-ordered B")
    assert_columns_match(Xf, ref, B, vtype, "Fortran-ordered B")


def test_scaled_handle(monkeypatch):
    """matching + scaling are applied per column: residuals against the oracle's on the same scaled matrix"""
    from .test_scaling import saddle

    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
    mat = saddle(6)
    n, cp, ri, va, _ = mat
    B = rhs_block(mat, 3)
    ref = oracle_columns("saddle6_scaled", mat, 32, "r64", B, scaling=True)
    h = open_handle(mat, 32, "hip", "r64", scaling=True)
    try:
        X = pa.pangulu_gstrs_multi(h, B)
        path = pa.last_solve_path(h)
    finally:
        pa.pangulu_finalize(h)
    assert path["device_columns"] == 3
    assert not X[:, 1].any()
    for j in (0, 2):
        res = M.relative_residual(n, cp, ri, va, X[:, j], B[:, j])
        res_ref = M.relative_residual(n, cp, ri, va, ref[:, j], B[:, j])
        assert res <= 1e-10 and abs(res - res_ref) <= 1e-10, (j, res, res_ref)


def test_second_factorisation_on_the_same_handle(monkeypatch):
    """update_values + gstrf keep the cached sweep plan: the second block solve is that of the NEW matrix"""
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
    mat, nb, vtype, B, ref = case("r64_kkt8")
    n, cp, ri, va, coords = mat
    va2 = va * (1.0 + 0.05 * np.cos(np.arange(len(va))))  # same pattern, every entry moved by up to 5 %
    mat2 = (n, cp, ri, va2, coords)
    ref2 = oracle_columns("r64_kkt8_new_values", mat2, nb, vtype, B)
    h = open_handle(mat, nb, "hip", vtype)
    try:
        X1 = pa.pangulu_gstrs_multi(h, B)
        pa.update_values(h, va2)
        pa.pangulu_gstrf(h)
        X2 = pa.pangulu_gstrs_multi(h, B)
        path = pa.last_solve_path(h)
    finally:
        pa.pangulu_finalize(h)
    assert path["device_columns"] == B.shape[1]
    assert_columns_match(X1, ref, B, vtype, "first factorisation")
    assert_columns_match(X2, ref2, B, vtype, "after update_values")
    assert np.abs(X2[:, 0] - X1[:, 0]).max() > 1e-3 * np.abs(X1[:, 0]).max()  # (the two systems do differ)


def test_host_sweep_when_the_device_solve_is_off(monkeypatch):
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "0")
    mat, nb, vtype, B, ref = case("r64_kkt8")
    h = open_handle(mat, nb, "hip", vtype)
    try:
        X = pa.pangulu_gstrs_multi(h, B)
        path = pa.last_solve_path(h)
    finally:
        pa.pangulu_finalize(h)
    assert path["device_columns"] == 0, path
    assert_columns_match(X, ref, B, vtype, "host sweep")


def test_return_codes():
    mat, nb, vtype, B, _ = case("r64_kkt8")
    n, nrhs = B.shape
    h = open_handle(mat, nb, "hip", vtype, gstrf=False)
    try:
        buf = np.asfortranarray(B).copy(order="F")
        assert raw_gstrs_multi(h, buf, nrhs, n) == 1  # not factorised
        assert (buf == B).all()
        pa.pangulu_gstrf(h)
        assert raw_gstrs_multi(h, buf, nrhs, n - 1) == 2
        assert raw_gstrs_multi(h, None, nrhs, n) == 2
        assert raw_gstrs_multi(h, buf, 0, n) == 0
        assert (buf == B).all()
    finally:
        pa.pangulu_finalize(h)


@pytest.mark.parametrize("name", ["r64_kkt8", "cr64_poisson12"])
def test_single_vector_solves_across_a_refactorisation(name, monkeypatch):
    """pangulu_gstrs sweeps on the plans cached on the handle: after update_values + gstrf they must give the NEW matrix's solution
    (a stale plan or stale descriptor pointers would show here first)"""
    monkeypatch.setenv("PANGULU_AMD_DEVICE_SOLVE", "1")
    mat, nb, vtype, B, ref = case(name)
    n, cp, ri, va, coords = mat
    va2 = va * (1.0 + 0.05 * np.cos(np.arange(len(va))))  # same pattern, every entry moved by up to 5 %
    ref2 = oracle_columns(name + "_new_values", (n, cp, ri, va2, coords), nb, vtype, B)
    B, ref, ref2 = B[:, :4], ref[:, :4], ref2[:, :4]
    h = open_handle(mat, nb, "hip", vtype)
    try:
        X1 = solve_columns(h, B)
        pa.update_values(h, va2)
        pa.pangulu_gstrf(h)
        X2 = solve_columns(h, B)
    finally:
        pa.pangulu_finalize(h)
    assert_columns_match(X1, ref, B, vtype, "first factorisation")
    assert_columns_match(X2, ref2, B, vtype, "after update_values")
    assert np.abs(X2[:, 0] - X1[:, 0]).max() > 1e-3 * np.abs(X1[:, 0]).max()  # (the two systems do differ)


class _SolveRow(ctypes.Structure):  # pangulu_hip_solve_row_t
    _fields_ = [("brow", ctypes.c_uint32), ("nblk", ctypes.c_uint32), ("first", ctypes.c_uint64), ("diag", ctypes.POINTER(slots.Slot))]


class _SolveSweep(ctypes.Structure):  # pangulu_hip_solve_sweep_t
    _fields_ = [("nlevel", ctypes.c_uint64), ("level_ptr", ctypes.POINTER(ctypes.c_uint64)), ("rows", ctypes.POINTER(_SolveRow)),
                ("blk_slots", ctypes.POINTER(ctypes.POINTER(slots.Slot))), ("blk_bcol", ctypes.POINTER(ctypes.c_uint32))]


def _level_plan(bm, lower):
    """One sweep as the operators take it: block rows grouped by level (1 + the highest level among the rows a row's off-diagonal
    blocks on the sweep's side read), each with its diagonal half and those blocks."""
    nbk = bm.nblk
    side = {r: sorted(c for (br, c, _) in bm.blocks if br == r and (c < r if lower else c > r)) for r in range(nbk)}
    level = [0] * nbk
    for r in (range(nbk) if lower else reversed(range(nbk))):
        level[r] = 1 + max((level[c] for c in side[r]), default=-1)
    nlevel = 1 + max(level)
    order = sorted(range(nbk), key=lambda r: (level[r], r))
    level_ptr = (ctypes.c_uint64 * (nlevel + 1))(*np.concatenate(([0], np.cumsum(np.bincount(level, minlength=nlevel)))).tolist())
    nblk = sum(len(v) for v in side.values())
    rows = (_SolveRow * nbk)()
    blk_slots = (ctypes.POINTER(slots.Slot) * max(nblk, 1))()
    blk_bcol = (ctypes.c_uint32 * max(nblk, 1))()
    k = 0
    for i, r in enumerate(order):
        rows[i].brow, rows[i].nblk, rows[i].first = r, len(side[r]), k
        rows[i].diag = ctypes.pointer(bm.blocks[(r, r, 0 if lower else 1)].slot)
        for c in side[r]:
            blk_slots[k] = ctypes.pointer(bm.get(r, c).slot)
            blk_bcol[k] = c
            k += 1
    return _SolveSweep(nlevel, level_ptr, rows, blk_slots, blk_bcol)


def test_backend_operators_called_directly():
    """block_trsv (one sweep, one host vector: the native host no longer calls it) lower then upper, and block_trsm_multi with one
    panel of width 1 on the same plans, on hand-built slots of the oracle's factor records: both give the oracle's pangulu_gstrs
    solution of the same right-hand side in the factors' ordering.  Not compared bitwise: several blocks add into one row with
    floating-point atomics, in an order that varies."""
    mat, nb, vtype, B, ref = case("r64_kkt8")
    n = mat[0]
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
        sw = [_level_plan(bm, True), _level_plan(bm, False)]
        vp = ctypes.c_void_p
        trsv, multi = hip.pangulu_platform_0201001_block_trsv, hip.pangulu_platform_0201001_block_trsm_multi
        trsv.restype = None
        trsv.argtypes = [ctypes.c_uint16, ctypes.c_int, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(_SolveRow),
                         ctypes.POINTER(ctypes.POINTER(slots.Slot)), ctypes.POINTER(ctypes.c_uint32), vp, ctypes.c_uint64]
        multi.restype = ctypes.c_int
        multi.argtypes = [ctypes.c_uint16, ctypes.POINTER(_SolveSweep), ctypes.POINTER(_SolveSweep), vp, ctypes.c_uint64, ctypes.c_uint64,
                          ctypes.POINTER(ctypes.c_int)]
        x1 = b.copy()
        for upper, s in enumerate(sw):
            trsv(nb, upper, s.nlevel, s.level_ptr, s.rows, s.blk_slots, s.blk_bcol, x1.ctypes.data_as(vp), xlen)
        x2 = b.copy()
        assert multi(nb, None, None, None, 0, 0, None) == 16  # (npanel = 0 only asks)
        assert multi(nb, ctypes.byref(sw[0]), ctypes.byref(sw[1]), x2.ctypes.data_as(vp), xlen, 1, (ctypes.c_int * 1)(1)) == 16
    finally:
        bm.free()
    scale = np.abs(want).max()
    for what, x in (("block_trsv, lower then upper", x1), ("block_trsm_multi, one panel of width 1", x2)):
        err = np.abs(x - want).max()
        assert err <= TOL[vtype] * scale, "%s: differs from the oracle by %g (scale %g)" % (what, err, scale)


def test_width_one_panels_through_the_column_by_column_kernels(tmp_path):
    """PANGULU_HIP_SOLVE_CHUNKED=0 leaves the kernels that take single vectors: the back-end offers panels of width 1 only, and the
    block solve sends its columns through them one panel each, in one call (a process of its own: the switch is read once)"""
    mat, nb, vtype, B, ref = case("r64_kkt8")
    out = str(tmp_path / "out.npz")
    env = dict(os.environ, PANGULU_HIP_SOLVE_CHUNKED="0", PANGULU_AMD_DEVICE_SOLVE="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    run = subprocess.run([sys.executable, os.path.join(root, "tests", "solve_by_column_worker.py"), "r64_kkt8", "3", out], env=env, cwd=root,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    z = np.load(out)
    assert {k: int(z[k]) for k in ("device_columns", "panel_width", "panels")} == {"device_columns": 3, "panel_width": 1, "panels": 3}
    assert_columns_match(z["X"], ref[:, :3], B[:, :3], vtype, "column-by-column kernels against the oracle")
